"""Compressed point sets through the JavaScript host (js/parallel.mjs pointsFromBytes {compressed} /
pointsToCompressedBytes over napi/msmz_napi.c importPointsCompressed / downloadPointsCompressed)."""
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-compressed.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "compressed_js_fixture.json")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_compressed_addon_and_script(addon):
    """CPU: the addon exports the two calls, both refuse bad arguments without a device, importPoints keeps its arity,
    and the script parses"""
    js = ("const a=require(%r); const t=[a.importPointsCompressed,a.downloadPointsCompressed,a.importPoints].map((f)=>typeof f);"
          "let refused=0; for (const f of [()=>a.importPointsCompressed(), ()=>a.importPointsCompressed(null,Buffer.alloc(48),null,1,false),"
          "()=>a.importPointsCompressed({},Buffer.alloc(48),null,1,false), ()=>a.downloadPointsCompressed(),"
          "()=>a.downloadPointsCompressed(null,1,0,1,48,false), ()=>a.importPoints(null,Buffer.alloc(96),null,1,false)])"
          "{ try { f(); } catch (e) { refused += e.code === '1' ? 1 : 0; } }"
          "console.log(JSON.stringify([t, refused]))" % addon)
    assert json.loads(subprocess.check_output([NODE, "-e", js], text=True)) == [["function"] * 3, 6]
    subprocess.run([NODE, "--check", SCRIPT], check=True)


def test_fixture_is_what_its_maker_builds():
    """CPU: the committed fixture equals what tests/golden/make_compressed_fixture.py builds from Python integers today"""
    spec = importlib.util.spec_from_file_location("make_compressed_fixture",
                                                  os.path.join(ROOT, "tests", "golden", "make_compressed_fixture.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    fx = json.load(open(FIXTURE))
    assert fx == maker.build()
    assert fx["n"] == 48 and sum(fx["isInf"]) == 7 and len(fx["largest"]["records"]) == 2 * 48 * 48
    assert fx["largest"]["records"] != fx["parity"]["records"]


@pytest.mark.gpu
def test_js_compressed(addon):
    """GPU: node decompresses the fixture's records under both conventions, reads the points back, downloads them
    compressed under both, runs an MSM over the set, and is refused the bad records with the right status"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["points"] == {"largest": True, "parity": True}
    for a in ("largest", "parity"):
        for b in ("largest", "parity"):
            assert got["download"][a + ">" + b] == fx[b]["download"], (a, b)
        fb = fx["feBytes"]
        assert got["range"][a] == fx[a]["download"][2 * fb * 5:2 * fb * 25]
    assert got["isInf"] == fx["isInf"] and got["msm"] is True
    assert (got["noRoot"], got["tooBig"], got["signedZeroRoot"]) == ("7", "6", "7")
    assert got["refusedArgs"] == 9 and got["after"] is True

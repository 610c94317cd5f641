"""Exports through the JavaScript host (js/parallel.mjs scalarsToBytes / pointsToBytes over napi/msmz_napi.c
exportScalars / exportPoints: msmz_export_scalars / msmz_export_points on the host route)."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-export.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "export_js_fixture.json")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_export_addon_and_script(addon):
    """CPU: the addon exports both functions, a call without arguments (or without a context) is refused by name, and
    the script parses"""
    js = ("const a=require(%r); const t=[a.exportScalars,a.exportPoints].map((f)=>typeof f); const msgs=[];"
          "for (const f of [()=>a.exportScalars(), ()=>a.exportPoints(), ()=>a.exportScalars(null,1,0,1,32,false),"
          "()=>a.exportScalars({},1,0,1,32,false), ()=>a.exportPoints(null,1,0,1,48,false), ()=>a.exportPoints({},1,0,1,48,false)])"
          "{ try { f(); msgs.push('accepted'); } catch (e) { msgs.push(e.code + ' ' + e.message.split(':')[0]); } }"
          "console.log(JSON.stringify([t, msgs]))" % addon)
    t, msgs = json.loads(subprocess.check_output([NODE, "-e", js], text=True))
    assert t == ["function"] * 2
    assert msgs == ["1 exportScalars", "1 exportPoints", "1 exportScalars", "1 exportScalars", "1 exportPoints", "1 exportPoints"]
    subprocess.run([NODE, "--check", SCRIPT], check=True)


def test_declarations_name_the_methods_and_their_options():
    dts = open(os.path.join(ROOT, "js", "parallel.d.ts")).read()
    m = re.search(r"scalarsToBytes\(scalars: DeviceArray, options\?: \{([^}]*)\}\): Promise<Uint8Array>;", dts)
    assert m and [o.split("?")[0].strip() for o in m.group(1).split(";")] == ["first", "n", "width", "montgomery"]
    m = re.search(r"pointsToBytes\(points: DeviceArray, options\?: \{([^}]*)\}\): Promise<\{ records: Uint8Array; isInf: Uint8Array \}>;", dts)
    assert m and [o.split("?")[0].strip() for o in m.group(1).split(";")] == ["first", "n", "montgomery"]
    mjs = open(os.path.join(ROOT, "js", "parallel.mjs")).read()
    assert "async scalarsToBytes(scalars, { first = 0, n, width = 32, montgomery = false } = {})" in mjs
    assert "async pointsToBytes(points, { first = 0, n, montgomery = false } = {})" in mjs


def test_fixture_is_what_its_maker_builds():
    """CPU: the committed fixture equals what tests/golden/make_export_fixture.py builds from Python integers today, and
    its records are what the definitions say"""
    spec = importlib.util.spec_from_file_location("make_export_fixture",
                                                  os.path.join(ROOT, "tests", "golden", "make_export_fixture.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    fx = json.load(open(FIXTURE))
    assert fx == maker.build()
    from msm_zprize_amd import curves
    c = curves.BY_LABEL[fx["curve"]]
    p, q, fb, n = c["modulus"], c["order"], c["fe_bytes"], fx["n"]
    assert (n, fx["feBytes"], sum(fx["isInf"])) == (65, fb, 7)
    s = [int(v) for v in fx["scalars"]]
    assert s[:4] == [0, 1, q - 1, (1 << 256) % q] and all(0 <= v < q for v in s)
    mont = bytes.fromhex(fx["montgomery"])
    assert [int.from_bytes(mont[32 * i:32 * i + 32], "little") for i in range(n)] == [v * (1 << 256) % q for v in s]
    assert bytes.fromhex(fx["narrow"]) == b"".join(int(v).to_bytes(8, "little") for v in fx["scalars64"])
    pm, pc = bytes.fromhex(fx["pointsMontgomery"]), bytes.fromhex(fx["pointsCanonical"])
    assert len(pm) == len(pc) == 2 * fb * n
    for i, pt in enumerate(fx["points"]):
        for k, name in enumerate("xy"):
            v = int(pt[name])
            at = (2 * i + k) * fb
            assert int.from_bytes(pc[at:at + fb], "little") == v
            assert int.from_bytes(pm[at:at + fb], "little") == v * (1 << (8 * fb)) % p
        assert pt["isZero"] == bool(fx["isInf"][i])
        if not pt["isZero"]:
            assert (int(pt["y"]) ** 2 - int(pt["x"]) ** 3 - c["b"]) % p == 0


@pytest.mark.gpu
def test_js_export(addon):
    """GPU: node exports canonical, narrow and Montgomery scalars and canonical and Montgomery points equal to the
    fixture, reads the Montgomery records back, and the error cases arrive"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for key in ("canonical", "narrow", "montgomery", "pointsCanonical", "pointsMontgomery", "isInf"):
        assert got[key] == fx[key], key
    fb = fx["feBytes"]
    assert got["range"] == fx["montgomery"][2 * 32 * 5:2 * 32 * 25]
    assert got["pointsRange"] == fx["pointsMontgomery"][2 * 2 * fb * 5:2 * 2 * fb * 25]
    assert got["roundTrip"] is True and got["tooWide"] == "6"
    assert got["refusedArgs"] == 12 and got["after"] is True

"""The JavaScript host's segmented MSM (js/parallel.mjs Parallel.msmSegments over napi/msmz_napi.c msmSegments)."""
import json
import os
import shutil
import subprocess

import pytest

from oracle import c_oracle
from oracle import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-segments.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "segments_js_fixture.json")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def _pt(d):
    return {"x": int(d["x"]), "y": int(d["y"]), "isZero": bool(d["isZero"])}


def test_addon_exports_msm_segments(addon):
    """CPU: the addon exposes msmSegments and the script parses"""
    js = "const a=require(%r); console.log(JSON.stringify(typeof a.msmSegments))" % addon
    assert json.loads(subprocess.check_output([NODE, "-e", js], text=True)) == "function"
    subprocess.run([NODE, "--check", SCRIPT], check=True)


def test_fixture_is_the_oracles():
    """CPU: the committed fixture holds several length classes with overlaps and repeats and, spot-checked, what the
    oracle says today"""
    fx = json.load(open(FIXTURE))
    c = P.CURVES[fx["curve"]]
    pts, s, segs = [_pt(p) for p in fx["points"]], [int(v) for v in fx["scalars"]], fx["segments"]
    assert len(fx["results"]) == len(segs) and len(fx["ipa"]) == 2
    assert len({n.bit_length() for _, _, n in segs}) >= 4 and len({tuple(g) for g in segs}) < len(segs)
    assert all(fp + n <= len(pts) and fs + n <= len(s) and n >= 1 for fp, fs, n in segs)
    for k in (0, 1, 3, 6, 9):
        fp, fs, n = segs[k]
        r = c_oracle.msm(c, s[fs:fs + n], pts[fp:fp + n])
        assert _pt(fx["results"][k]) == {"x": r["x"], "y": r["y"], "isZero": bool(r.get("isZero", False))}
    assert fx["results"][1] == fx["results"][4]


@pytest.mark.gpu
def test_js_msm_segments(addon):
    """GPU: node reproduces the fixture, with safe and unsafe additions, and the L and R of an IPA round"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])

    def canon(ps):   # an infinity result carries no coordinates worth comparing
        return [{"isZero": True} if p["isZero"] else p for p in ps]

    assert canon(got["safe"]) == canon(fx["results"])
    assert canon(got["unsafe"]) == canon(fx["results"])
    assert canon(got["ipa"]) == canon(fx["ipa"])
    assert got["refused"]

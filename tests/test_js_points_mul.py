"""Per-point scalar multiplication through the JavaScript host (js/parallel.mjs mulPoints over napi/msmz_napi.c)."""
import json
import os
import shutil
import subprocess

import pytest

import points_mul_util as M
from oracle import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-mul-points.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "points_mul_js_fixture.json")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def _pt(d):
    return {"x": int(d["x"]), "y": int(d["y"]), "isZero": bool(d["isZero"])}


def test_js_mul_points_script_parses(addon):
    """CPU: the addon exports mulPoints and the script parses"""
    js = "const a=require(%r); console.log(JSON.stringify(typeof a.mulPoints))" % addon
    assert json.loads(subprocess.check_output([NODE, "-e", js], text=True)) == "function"
    subprocess.run([NODE, "--check", SCRIPT], check=True)


def test_fixture_is_the_oracles():
    """CPU: the committed fixture holds the planted rows and, spot-checked, what the oracle says today"""
    fx = json.load(open(FIXTURE))
    params = P.CURVES[fx["curve"]]
    n, q = fx["n"], params["order"]
    assert n == 65 and all(len(fx[k]) == n for k in ("scalars", "points", "addend", "plain", "added", "broadcast"))
    assert len(fx["fold"]) == n // 2
    s = [int(v) for v in fx["scalars"]]
    assert {0, 1, q - 1} <= set(s) and any(p["isZero"] for p in fx["points"]) and any(p["isZero"] for p in fx["addend"])
    assert sum(p["isZero"] for p in fx["added"]) >= 1 and sum(p["isZero"] for p in fx["plain"]) >= 2
    for i in (0, 5, 6, 7, 8, 40, 64):
        p, a = _pt(fx["points"][i]), _pt(fx["addend"][i])
        assert _pt(fx["plain"][i]) == M.expected(params, s[i], p)
        assert _pt(fx["added"][i]) == M.expected(params, s[i], p, a)
        assert _pt(fx["broadcast"][i]) == M.expected(params, int(fx["u"]), p, a)
    assert _pt(fx["fold"][3]) == M.expected(params, int(fx["u"]), _pt(fx["points"][35]), _pt(fx["points"][3]))


@pytest.mark.gpu
def test_js_mul_points(addon):
    """GPU: node multiplies the fixture's 65 rows without and with the addend, with the broadcast scalar, and folds the
    set's halves; every point is the fixture's"""
    fx = json.load(open(FIXTURE))
    params = P.CURVES[fx["curve"]]
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for mode in ("plain", "added", "broadcast", "fold"):
        g = [M.canon(params, _pt(p)) for p in got[mode]]
        w = [_pt(p) for p in fx[mode]]
        assert g == w, (mode, [i for i, (a, b) in enumerate(zip(g, w)) if a != b][:5])
    assert got["refused"] and got["msm"]

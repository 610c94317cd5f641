"""Per-point scalar multiplication with options through the JavaScript host (js/parallel.mjs mulPoints {scalarBits,
subgroup} over napi/msmz_napi.c, msmz_points_mul_opts)."""
import json
import os
import shutil
import subprocess

import pytest

import check_points_util as U
import points_mul_util as M
from oracle import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-mul-points-opts.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "points_mul_opts_js_fixture.json")
MODES = ("subgroup", "broadcast", "fold128", "bounded64")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def _pt(d):
    return {"x": int(d["x"]), "y": int(d["y"]), "isZero": bool(d["isZero"])}


def test_js_mul_points_opts_script_parses(addon):
    """CPU: the addon exports mulPoints with the two option arguments (the eight-argument form is refused), the script
    parses, and the declaration file names the options"""
    js = ("const a=require(%r); let e=''; try { a.mulPoints(null,0,0,0,0,0,0,1) } catch (x) { e=x.message } "
          "console.log(JSON.stringify([typeof a.mulPoints, e]))" % addon)
    kind, err = json.loads(subprocess.check_output([NODE, "-e", js], text=True))
    assert kind == "function" and "mulPoints" in err
    subprocess.run([NODE, "--check", SCRIPT], check=True)
    with open(os.path.join(ROOT, "js", "parallel.d.ts")) as f:
        dts = f.read()
    assert "scalarBits?: number; subgroup?: boolean" in dts


def test_fixture_is_the_oracles():
    """CPU: the committed fixture holds subgroup points only and the planted rows, and, spot-checked, what the oracle
    says today"""
    fx = json.load(open(FIXTURE))
    params = P.CURVES[fx["curve"]]
    n, q = fx["n"], params["order"]
    assert n == 65 and all(len(fx[k]) == n for k in ("scalars", "scalars64", "points", "addend", "subgroup", "broadcast", "bounded64"))
    assert len(fx["fold128"]) == n // 2
    s, s64 = [int(v) for v in fx["scalars"]], [int(v) for v in fx["scalars64"]]
    assert {0, 1, q - 1} <= set(s) and any(p["isZero"] for p in fx["points"]) and any(p["isZero"] for p in fx["addend"])
    assert max(s64) == (1 << 64) - 1 and s64[-1] == max(s64) and 1 << 127 <= int(fx["u128"]) < 1 << 128
    assert all(U.verdict_fast(params, _pt(p)) == 0 for p in fx["points"])
    for i in (0, 2, 5, 6, 7, 8, 40, 64):
        p, a = _pt(fx["points"][i]), _pt(fx["addend"][i])
        assert _pt(fx["subgroup"][i]) == M.expected(params, s[i], p, a)
        assert _pt(fx["broadcast"][i]) == M.expected(params, int(fx["u"]), p, a)
        assert _pt(fx["bounded64"][i]) == M.expected(params, s64[i], p)
    assert _pt(fx["fold128"][3]) == M.expected(params, int(fx["u128"]), _pt(fx["points"][35]), _pt(fx["points"][3]))


@pytest.mark.gpu
def test_js_mul_points_opts(addon):
    """GPU: node multiplies the fixture's 65 rows under the vouch (per-lane and broadcast scalars), folds the halves with
    a 128-bit challenge under scalarBits = 128, and multiplies by 64-bit scalars under scalarBits = 64; every point is
    the fixture's, the vouched results are the plain calls', and the bound's errors arrive"""
    fx = json.load(open(FIXTURE))
    params = P.CURVES[fx["curve"]]
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for mode in MODES:
        g = [M.canon(params, _pt(p)) for p in got[mode]]
        w = [_pt(p) for p in fx[mode]]
        assert g == w, (mode, [i for i, (a, b) in enumerate(zip(g, w)) if a != b][:5])
    assert got["same"] and got["refused"] and got["range"]

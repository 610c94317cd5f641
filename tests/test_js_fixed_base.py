"""Fixed-base multiplication through the JavaScript host (js/parallel.mjs fixedBaseMul over napi/msmz_napi.c,
msmz_points_fixed_base)."""
import json
import os
import shutil
import subprocess

import pytest

import check_points_util as U
import fixed_base_util as FB
import points_mul_util as M
from oracle import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-fixed-base.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "fixed_base_js_fixture.json")
MODES = ("generator", "affine", "resident", "bounded64", "srs")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def _pt(d):
    return {"x": int(d["x"]), "y": int(d["y"]), "isZero": bool(d["isZero"])}


def test_js_fixed_base_script_parses(addon):
    """CPU: the addon exports fixedBaseMul (a call without its arguments is refused by name), the script parses, and the
    declaration file names the method and its options"""
    js = ("const a=require(%r); let e=''; try { a.fixedBaseMul(null,0,0) } catch (x) { e=x.message } "
          "console.log(JSON.stringify([typeof a.fixedBaseMul, e]))" % addon)
    kind, err = json.loads(subprocess.check_output([NODE, "-e", js], text=True))
    assert kind == "function" and "fixedBaseMul" in err
    subprocess.run([NODE, "--check", SCRIPT], check=True)
    with open(os.path.join(ROOT, "js", "parallel.d.ts")) as f:
        dts = f.read()
    assert "fixedBaseMul(scalars: DeviceArray, n?: number," in dts and "baseIndex?: number" in dts


def test_fixture_is_the_oracles():
    """CPU: the committed fixture holds the planted scalars and, spot-checked, what the oracle says today"""
    fx = json.load(open(FIXTURE))
    params = P.CURVES[fx["curve"]]
    n, q = fx["n"], params["order"]
    assert n == 65 and all(len(fx[k]) == n for k in ("scalars", "scalars64", "generator", "affine", "bounded64", "srs"))
    assert len(fx["resident"]) == n - n // 2
    s, s64 = [int(v) for v in fx["scalars"]], [int(v) for v in fx["scalars64"]]
    assert {0, 1, 2, q - 1, (1 << 13) - 1, 1 << 13, (1 << 13) + 1} <= set(s)
    assert max(s64) == (1 << 64) - 1 and max(s) >> 64
    g, b = U.generator(params), _pt(fx["base"])
    assert U.verdict_fast(params, b) == 0 and b != g
    tau = int(fx["tau"])
    for i in (0, 1, 3, 5, 40, 64):
        assert _pt(fx["generator"][i]) == FB.expected(fx["curve"], s[i], g)
        assert _pt(fx["affine"][i]) == FB.expected(fx["curve"], s[i], b)
        assert _pt(fx["bounded64"][i]) == FB.expected(fx["curve"], s64[i], b)
        assert _pt(fx["srs"][i]) == FB.expected(fx["curve"], pow(tau, i, q), g)
    assert fx["resident"] == fx["affine"][n // 2:]
    assert _pt(fx["generator"][0])["isZero"] and _pt(fx["srs"][0]) == M.canon(params, g)


@pytest.mark.gpu
def test_js_fixed_base(addon):
    """GPU: node multiplies the fixture's scalars by the generator, by an affine base, by a resident base over a range,
    by 64-bit scalars under scalarBits = 64, and makes an SRS from scalarPowers; every point is the fixture's, mulPoints
    over copies of the base agrees, and the argument and bound errors arrive"""
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

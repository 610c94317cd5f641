"""The JavaScript host's precomputed point sets (js/parallel.mjs Parallel.precomputePoints over napi/msmz_napi.c
precomputePoints / precomputedInfo)."""
import json
import os
import shutil
import subprocess

import pytest

from oracle import c_oracle
from oracle import params as P
from oracle import prng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-precompute.mjs")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_addon_exports_precompute(addon):
    """CPU: the addon exposes precomputePoints / precomputedInfo, they refuse a missing context, and the script parses"""
    js = ("const a=require(%r); let r=[typeof a.precomputePoints, typeof a.precomputedInfo];"
          "try { a.precomputePoints(null, 1, 1, {}, 0); r.push('no'); } catch (e) { r.push(e.code); }"
          "console.log(JSON.stringify(r))") % addon
    assert json.loads(subprocess.check_output([NODE, "-e", js], text=True)) == ["function", "function", "1"]
    subprocess.run([NODE, "--check", SCRIPT], check=True)


@pytest.mark.gpu
@pytest.mark.parametrize("glv,factor", [(0, 0), (1, 0), (0, 3)])
def test_js_precomputed_closed_form(addon, glv, factor):
    """GPU: single and batched MSMs over a precomputed set from node == (sum_i s_ki a_i) G == the plain set's"""
    lg, B = 12, 3
    out = subprocess.run([NODE, SCRIPT, str(lg), str(B), "--glv", str(glv), "--factor", str(factor)],
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    c = P.BLS12_377
    q, n = c["order"], 1 << lg
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    a = prng.multipliers_np(1, n)

    def want(t):
        r = c_oracle.scale(c, t % q, gen)
        return {"x": str(r["x"]), "y": str(r["y"]), "isZero": bool(r.get("isZero", False))}

    res = [want(prng.sum_of_products_mod(prng.scalars_np(2, n, q, first=k * n), a, q)) for k in range(B)]
    assert got["batch"] == res
    assert got["batchPlain"] == res
    assert got["single"] == res[0] == got["plain"]
    info = got["info"]
    assert info["glv"] == glv
    assert info["factor"] == factor if factor else info["factor"] >= info["K"]   # (0: the GLV retry's windows too)
    assert info["records"] == info["factor"] * n * (2 if glv else 1)
    assert got["refused"]

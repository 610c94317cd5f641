"""The scalar bit bound through the JavaScript host (js/parallel.mjs options.scalarBits over napi/msmz_napi.c)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import c_oracle
from oracle import params as P
from oracle import prng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-scalar-bits.mjs")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_scalar_bits_script_parses(addon):
    """CPU: the addon loads and the script parses"""
    js = "const a=require(%r); console.log(JSON.stringify(typeof a.precomputedInfo))" % addon
    assert json.loads(subprocess.check_output([NODE, "-e", js], text=True)) == "function"
    subprocess.run([NODE, "--check", SCRIPT], check=True)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 33])
def test_js_scalar_bits_closed_form(addon, bits):
    """GPU: bounded single, batched and precomputed MSMs from node == (sum_i s_ki a_i) G; fewer windows ran; a bad bound
    and a scalar equal to 2^bits are refused and the context stays usable"""
    lg, B = 12, 3
    out = subprocess.run([NODE, SCRIPT, str(lg), str(B), str(bits)], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    c = P.BLS12_377
    q, n = c["order"], 1 << lg
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    a = prng.multipliers_np(1, n)

    def want(k):
        s = np.zeros((n, 4), dtype=np.uint64)
        s[:, 0] = np.arange(n, dtype=np.uint64) + np.uint64(k * 1000 + 1)
        r = c_oracle.scale(c, prng.sum_of_products_mod(s, a, q) % q, gen)
        return {"x": str(r["x"]), "y": str(r["y"]), "isZero": bool(r.get("isZero", False))}

    res = [want(k) for k in range(B)]
    assert got["bounded"] == res[0] and got["plain"] == res[0] and got["pre"] == res[0] and got["after"] == res[0]
    assert got["batch"] == res
    assert got["K"] < got["Kplain"]
    info = got["info"]
    assert info["scalarBits"] == bits and info["K"] == -(-(bits + 1) // info["c"]) and info["factor"] == info["K"]
    assert got["refused"] and got["range"]

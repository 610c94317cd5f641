"""The JavaScript host's batched MSM (js/parallel.mjs Parallel.msmBatch over napi/msmz_napi.c msmBatch)."""
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


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_addon_exports_msm_batch(addon):
    """CPU: the addon exposes msmBatch and the batch script parses"""
    js = "const a=require(%r); console.log(JSON.stringify(typeof a.msmBatch))" % addon
    assert json.loads(subprocess.check_output([NODE, "-e", js], text=True)) == "function"
    subprocess.run([NODE, "--check", os.path.join(ROOT, "js", "scripts", "msm-batch.mjs")], check=True)


@pytest.mark.gpu
@pytest.mark.parametrize("glv", [0, 1])
def test_js_msm_batch_closed_form(addon, glv):
    """GPU: resident and host-list batches from node == (sum_i s_ki a_i) G per vector"""
    lg, B = 12, 5
    out = subprocess.run([NODE, os.path.join(ROOT, "js", "scripts", "msm-batch.mjs"), str(lg), str(B), "--glv", str(glv)],
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
    assert got["resident"] == res
    host = []
    for k in range(B):
        s = np.zeros((n, 4), dtype=np.uint64)
        s[:, 0] = np.arange(n, dtype=np.uint64) + np.uint64(k * 1000 + 1)
        host.append(want(prng.sum_of_products_mod(s, a, q)))
    assert got["host"] == host
    assert got["refused"]

"""Narrow and Montgomery inputs through the JavaScript host (js/parallel.mjs scalarsFromBytes / pointsFromBytes options
over napi/msmz_napi.c importScalars / importPoints)."""
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
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-import.mjs")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_import_script_parses(addon):
    """CPU: the addon exports the two import functions and the script parses"""
    js = "const a=require(%r); console.log(JSON.stringify([typeof a.importScalars, typeof a.importPoints]))" % addon
    assert json.loads(subprocess.check_output([NODE, "-e", js], text=True)) == ["function", "function"]
    subprocess.run([NODE, "--check", SCRIPT], check=True)
    subprocess.run([NODE, "--check", os.path.join(ROOT, "js", "parallel.mjs")], check=True)


@pytest.mark.gpu
def test_js_import_closed_form(addon):
    """GPU: MSMs from node over 8-byte scalars and over Montgomery scalars with Montgomery points == (sum_i s_i a_i) G ==
    the plain route; the imported sets read back canonical; bad widths are refused before the device, a Montgomery
    record equal to q by it, and the context stays usable"""
    lg = 12
    out = subprocess.run([NODE, SCRIPT, str(lg)], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    c = P.BLS12_377
    q, n = c["order"], 1 << lg
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    a = prng.multipliers_np(1, n)
    s = np.zeros((n, 4), dtype=np.uint64)
    s[:, 0] = np.arange(n, dtype=np.uint64) + np.uint64(1)
    r = c_oracle.scale(c, prng.sum_of_products_mod(s, a, q) % q, gen)
    want = {"x": str(r["x"]), "y": str(r["y"]), "isZero": bool(r.get("isZero", False))}
    assert got["plain"] == want and got["narrow"] == want and got["mont"] == want and got["after"] == want
    assert got["scalarsEqual"] and got["pointsEqual"]
    # the byte route without n (and Scalar.fromBigints, which calls it so) still uploads bytes.length / 32 scalars
    assert got["defaults"] is True and got["shortBuffer"] is True
    assert got["refusedWidth"] and got["refusedMont"] and got["range"]

"""Point-set validation through the JavaScript host (js/parallel.mjs checkPoints over napi/msmz_napi.c)."""
import json
import os
import random
import shutil
import subprocess

import pytest

import check_points_util as U
from oracle import params as P
from oracle import prng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-check-points.mjs")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_check_points_script_parses(addon):
    """CPU: the addon exports checkPoints and the script parses"""
    js = "const a=require(%r); console.log(JSON.stringify(typeof a.checkPoints))" % addon
    assert json.loads(subprocess.check_output([NODE, "-e", js], text=True)) == "function"
    subprocess.run([NODE, "--check", SCRIPT], check=True)


@pytest.mark.gpu
def test_js_check_points_counts(addon, tmp_path):
    """GPU: node checks a generated set of 2^12 and one with planted points; counts, first_bad and every verdict byte are
    the oracle's"""
    lg = 12
    n = 1 << lg
    params = P.BLS12_377
    bad = U.bad_points("bls12-377", random.Random(12))
    where = [7, 63, 64, 255, 256, 1500, 1501, n - 1] + [2000 + 37 * k for k in range(len(bad) - 8)]
    plant = [{"i": i, "x": str(q["x"]), "y": str(q["y"])} for i, q in zip(where, bad)]
    path = tmp_path / "plant.json"
    path.write_text(json.dumps(plant))
    out = subprocess.run([NODE, SCRIPT, str(lg), str(path)], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["good"] == {"ok": True, "offCurve": 0, "offSubgroup": 0, "firstBad": None, "verdicts": [0] * n}
    # the generated points are a_i G (oracle/prng.py restates the generator): spot-check that claim with the oracle
    a = prng.multipliers_np(1, n)
    g = U.generator(params)
    for i in (0, 1, n - 2):
        assert U.verdict(params, U.scale(params, int(a[i]), g)) == 0
    want = [0] * n
    for i, q in zip(where, bad):
        want[i] = U.verdict(params, q)

    def shape(v, first=0):
        s = U.summary(v, first)
        return {"ok": s[2] == U.NO_INDEX, "offCurve": s[0], "offSubgroup": s[1], "firstBad": None if s[2] == U.NO_INDEX else s[2],
                "verdicts": v}

    print(got["planted"]["offCurve"], got["planted"]["offSubgroup"], got["planted"]["firstBad"])
    assert got["planted"] == shape(want)
    assert got["curveOnly"] == shape([v & 1 for v in want])
    first = got["range"].pop("first")
    assert first == 0 and got["range"] == shape(want[:64])
    assert got["refused"] and got["msm"]

"""Writes tests/golden/fixed_base_js_fixture.json: the inputs of js/scripts/msm-fixed-base.mjs (65 BLS12-377 scalars with
0, 1, 2, q - 1 and both sides of the boundaries of 13-bit windows in front, 65 scalars below 2^64, a base B = [k]G, a
second point, tau) and what this repository's oracle (tests/fixed_base_util.py over oracle/) says
msmz_points_fixed_base owes for them.  Run from the repository root:
    python tests/golden/make_fixed_base_fixture.py"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import check_points_util as U   # noqa: E402
import fixed_base_util as FB   # noqa: E402
from oracle import params as P   # noqa: E402

LABEL, N = "bls12-377", 65


def enc(q):
    return {"x": str(q["x"]), "y": str(q["y"]), "isZero": bool(q["isZero"])}


def main():
    params = P.CURVES[LABEL]
    q = params["order"]
    rng = random.Random(2026)
    g = U.generator(params)
    base = U.scale(params, rng.randrange(1, q), g)
    other = U.scale(params, rng.randrange(1, q), g)
    tau = rng.randrange(2, q)
    s = FB.gpu_scalars(params, 40, 9)[:40] + [rng.randrange(q) for _ in range(N - 40)]
    s64 = [0, 1, (1 << 64) - 1, 1 << 63] + [rng.randrange(1 << 64) for _ in range(N - 5)] + [(1 << 64) - 1]
    half = N // 2
    fx = {
        "curve": LABEL, "n": N, "tau": str(tau), "base": enc(base), "other": enc(other),
        "scalars": [str(v) for v in s], "scalars64": [str(v) for v in s64],
        "generator": [enc(FB.expected(LABEL, v, g)) for v in s],
        "affine": [enc(FB.expected(LABEL, v, base)) for v in s],
        "resident": [enc(FB.expected(LABEL, v, base)) for v in s[half:]],
        "bounded64": [enc(FB.expected(LABEL, v, base)) for v in s64],
        "srs": [enc(FB.expected(LABEL, pow(tau, i, q), g)) for i in range(N)],
    }
    with open(os.path.join(HERE, "fixed_base_js_fixture.json"), "w") as f:
        json.dump(fx, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

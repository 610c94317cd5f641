"""Writes tests/golden/points_mul_opts_js_fixture.json: the inputs of js/scripts/msm-mul-points-opts.mjs (65 rows of
BLS12-377 with the planted rows of tests/points_mul_opts_util.py: every point in the prime-order subgroup, s = 0, 1,
q - 1, P and Q at infinity, Q = +-[s]P) and what the oracle (oracle/bigint_ref.py) says msmz_points_mul_opts owes for
them.  Run from the repository root:
    python tests/golden/make_points_mul_opts_fixture.py"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import points_mul_opts_util as O   # noqa: E402
import points_mul_util as M   # noqa: E402
from oracle import params as P   # noqa: E402

LABEL, N = "bls12-377", 65


def enc(q):
    return {"x": str(q["x"]), "y": str(q["y"]), "isZero": bool(q["isZero"])}


def main():
    params = P.CURVES[LABEL]
    rows = O.subgroup_set(LABEL, N, 2025)
    rng = random.Random(66)
    u = rng.randrange(1, params["order"])
    u128 = rng.randrange(1 << 127, 1 << 128)
    s64 = [0, 1, (1 << 64) - 1, 1 << 63] + [rng.randrange(1 << 64) for _ in range(N - 5)] + [(1 << 64) - 1]
    pts = [p for _, p, _ in rows]
    half = N // 2
    fx = {
        "curve": LABEL, "n": N, "u": str(u), "u128": str(u128),
        "scalars": [str(s) for s, _, _ in rows], "scalars64": [str(s) for s in s64],
        "points": [enc(p) for p in pts], "addend": [enc(q) for _, _, q in rows],
        "subgroup": [enc(M.expected(params, s, p, q)) for s, p, q in rows],
        "broadcast": [enc(M.expected(params, u, p, q)) for _, p, q in rows],
        "fold128": [enc(M.expected(params, u128, pts[half + i], pts[i])) for i in range(half)],
        "bounded64": [enc(M.expected(params, s, p)) for s, p in zip(s64, pts)],
    }
    with open(os.path.join(HERE, "points_mul_opts_js_fixture.json"), "w") as f:
        json.dump(fx, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

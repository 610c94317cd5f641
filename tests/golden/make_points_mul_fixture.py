"""Writes tests/golden/points_mul_js_fixture.json: the inputs of js/scripts/msm-mul-points.mjs (65 rows of BLS12-377 with
the planted rows of tests/points_mul_util.py: s = 0, 1, q - 1, P and Q at infinity, Q = +-[s]P, a point of order 3) and
what the oracle (oracle/bigint_ref.py) says msmz_points_mul owes for them.  Run from the repository root:
    python tests/golden/make_points_mul_fixture.py"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import points_mul_util as M   # noqa: E402
from oracle import params as P   # noqa: E402

LABEL, N = "bls12-377", 65


def enc(q):
    return {"x": str(q["x"]), "y": str(q["y"]), "isZero": bool(q["isZero"])}


def main():
    params = P.CURVES[LABEL]
    rows = M.build_set(LABEL, N, 2024)
    u = random.Random(65).randrange(1, params["order"])
    pts = [p for _, p, _ in rows]
    half = N // 2
    fx = {
        "curve": LABEL, "n": N, "u": str(u),
        "scalars": [str(s) for s, _, _ in rows], "points": [enc(p) for p in pts], "addend": [enc(q) for _, _, q in rows],
        "plain": [enc(M.expected(params, s, p)) for s, p, _ in rows],
        "added": [enc(M.expected(params, s, p, q)) for s, p, q in rows],
        "broadcast": [enc(M.expected(params, u, p, q)) for _, p, q in rows],
        "fold": [enc(M.expected(params, u, pts[half + i], pts[i])) for i in range(half)],
    }
    with open(os.path.join(HERE, "points_mul_js_fixture.json"), "w") as f:
        json.dump(fx, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

"""Writes tests/golden/export_js_fixture.json, the input of js/scripts/msm-export.mjs, from Python integers only: 65
BLS12-377 scalars (0, 1, q - 1 and 2^256 mod q in front), 65 scalars below 2^64, 65 points [k]G with every ninth a point at
infinity, and what msmz_export_scalars / msmz_export_points owe for them: the canonical, narrow and Montgomery scalar
records and the canonical and Montgomery point records, hex.  Run from the repository root:
    python tests/golden/make_export_fixture.py"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import check_points_util as U   # noqa: E402
from oracle import params as P   # noqa: E402

LABEL, N = "bls12-377", 65
R256 = 1 << 256


def enc(vals, width):
    return b"".join(int(v).to_bytes(width, "little") for v in vals)


def build():
    params = P.CURVES[LABEL]
    p, q, fb = params["modulus"], params["order"], params["fe_bytes"]
    rng = random.Random(2323)
    s = [0, 1, q - 1, R256 % q] + [rng.randrange(q) for _ in range(N - 4)]
    s64 = [0, 1, (1 << 64) - 1, 1 << 63] + [rng.randrange(1 << 64) for _ in range(N - 4)]
    g = U.generator(params)
    flags = [1 if i % 9 == 4 else 0 for i in range(N)]
    pts = [{"x": 0, "y": 0, "isZero": True} if flags[i] else U.scale(params, rng.randrange(1, 1 << 20), g) for i in range(N)]
    rstd = 1 << (8 * fb)
    coords = [c for pt in pts for c in (pt["x"], pt["y"])]
    return {
        "curve": LABEL, "n": N, "feBytes": fb, "isInf": flags,
        "scalars": [str(v) for v in s], "scalars64": [str(v) for v in s64],
        "points": [{"x": str(pt["x"]), "y": str(pt["y"]), "isZero": bool(pt["isZero"])} for pt in pts],
        "canonical": enc(s, 32).hex(), "narrow": enc(s64, 8).hex(), "montgomery": enc([v * R256 % q for v in s], 32).hex(),
        "pointsCanonical": enc(coords, fb).hex(), "pointsMontgomery": enc([c * rstd % p for c in coords], fb).hex(),
    }


if __name__ == "__main__":
    path = os.path.join(HERE, "export_js_fixture.json")
    with open(path, "w") as f:
        json.dump(build(), f, indent=0)
        f.write("\n")
    print("wrote", path)

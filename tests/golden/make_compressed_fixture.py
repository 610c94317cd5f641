"""Writes tests/golden/compressed_js_fixture.json, the input of js/scripts/msm-compressed.mjs, from Python integers only:
48 points of BLS12-377 (named points with zero roots and small orders, raw points from random x, multiples of G; every
seventh a flagged infinity whose record is junk), their compressed records under both sign conventions, what the
compressed download owes, and records that must be refused.  Run from the repository root:
    python tests/golden/make_compressed_fixture.py"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import compressed_util as Z    # noqa: E402
from oracle import params as P   # noqa: E402

LABEL, N = "bls12-377", 48


def build():
    params = P.CURVES[LABEL]
    p, fb = params["modulus"], params["fe_bytes"]
    pts, flags = Z.round_trip_points(LABEL, N, seed=23)
    rng = random.Random(29)
    out = {"curve": LABEL, "n": N, "feBytes": fb, "isInf": list(flags),
           "points": [{"x": str(q["x"]), "y": str(q["y"]), "isZero": q["isZero"]} for q in pts]}
    for sign in Z.SIGNS:
        out[sign] = {"records": Z.records(params, pts, flags, sign, rng).hex(),
                     "download": Z.want_compressed(params, pts, sign)[0].hex()}
    out["noRoot"] = Z.non_residue_wire(params, rng).to_bytes(fb, "little").hex()
    out["tooBig"] = p.to_bytes(fb, "little").hex()
    out["signedZeroRoot"] = ((p - 1) | (1 << (8 * fb - 1))).to_bytes(fb, "little").hex()   # (-1, 0) with a sign bit
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "compressed_js_fixture.json")
    with open(path, "w") as f:
        json.dump(build(), f, indent=1)
        f.write("\n")
    print("wrote", path)

"""Writes tests/golden/segments_js_fixture.json: the inputs of js/scripts/msm-segments.mjs (96 points and 120 scalars of
BLS12-377, segments of several length classes that overlap and repeat) and what the oracle (oracle/c_oracle.py) says
msmz_msm_segments owes for them, plus the L and R of an IPA round over the halves of the point set.  Run from the
repository root:
    python tests/golden/make_segments_fixture.py"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE))]

from oracle import c_oracle   # noqa: E402
from oracle import params as P   # noqa: E402

LABEL, NP, NS = "bls12-377", 96, 120
SEGMENTS = [[0, 0, 1], [10, 20, 5], [30, 7, 33], [0, 24, 96], [10, 20, 5], [40, 60, 50], [95, 119, 1], [48, 0, 48],
            [3, 3, 63], [64, 88, 32]]


def enc(q):
    return {"x": str(q["x"]), "y": str(q["y"]), "isZero": bool(q.get("isZero", False))}


def main():
    c = P.CURVES[LABEL]
    rng = random.Random(1717)
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    pts = [c_oracle.scale(c, rng.randrange(1, c["order"]), gen) for _ in range(NP)]
    s = [rng.randrange(c["order"]) for _ in range(NS)]
    s[20], s[119] = 0, c["order"] - 1
    msm = lambda fp, fs, n: enc(c_oracle.msm(c, s[fs:fs + n], pts[fp:fp + n]))
    h = NP // 2
    fx = {"curve": LABEL, "points": [enc(p) for p in pts], "scalars": [str(v) for v in s], "segments": SEGMENTS,
          "results": [msm(*seg) for seg in SEGMENTS], "ipa": [msm(h, 0, h), msm(0, h, h)]}
    with open(os.path.join(HERE, "segments_js_fixture.json"), "w") as f:
        json.dump(fx, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

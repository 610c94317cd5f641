"""Writes tests/golden/scalar_scan_js_fixture.json: the inputs of js/scripts/msm-scalar-scan.mjs (65 scalars x, y of
BLS12-377 with the planted pairs of tests/scalar_ops_util.py: 0, 1, q - 1, the carry-chain values) and what Python
integers mod oracle.params' group order say the recurrences and the inversion owe for them.  Run from the repository
root:
    python tests/golden/make_scalar_scan_fixture.py"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import scalar_ops_util as S    # noqa: E402
import scalar_scan_util as U   # noqa: E402

LABEL, N = "bls12-377", 65


def build():
    q = S.order(LABEL)
    xs, ys = S.build_vectors(LABEL, N, 2027)
    rng = random.Random(67)
    z, init = rng.randrange(2, q), rng.randrange(2, q)
    half = N // 2
    text = lambda pair: [[str(v) for v in pair[0]], str(pair[1])]
    quotient, value = U.synthetic_division(q, ys, z)
    inverse, zeros = U.inverse(q, xs)
    return {
        "curve": LABEL, "n": N, "z": str(z), "init": str(init),
        "x": [str(v) for v in xs], "y": [str(v) for v in ys],
        "sums": text(U.recurrence(q, N, None, ys)),
        "products": text(U.recurrence(q, N, xs, None)),
        "grand": text(U.recurrence(q, N, xs, None, exclusive=True)),
        "quotient": [str(v) for v in quotient], "value": str(value),
        "general": text(U.recurrence(q, N, xs, ys, init, reverse=True)),
        "inverse": [str(v) for v in inverse], "zeros": zeros,
        "inplace": [str(v) for v in inverse[:half] + xs[half:]],
    }


def main():
    with open(os.path.join(HERE, "scalar_scan_js_fixture.json"), "w") as f:
        json.dump(build(), f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

"""Writes tests/golden/scalar_ops_js_fixture.json: the inputs of js/scripts/msm-scalar-ops.mjs (65 scalars x, y, c of
BLS12-377 with the planted pairs of tests/scalar_ops_util.py: 0, 1, q - 1, the carry-chain values, pairs that sum to q)
and what Python integers mod oracle.params' group order say the three calls owe for them.  Run from the repository root:
    python tests/golden/make_scalar_ops_fixture.py"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import scalar_ops_util as S   # noqa: E402

LABEL, N = "bls12-377", 65


def main():
    q = S.order(LABEL)
    xs, ys = S.build_vectors(LABEL, N, 2025)
    _, cs = S.build_vectors(LABEL, N, 2026)
    rng = random.Random(66)
    a, b, z = rng.randrange(2, q), rng.randrange(2, q), rng.randrange(2, q)
    half = N // 2
    fold = [(xs[i] + a * xs[half + i]) % q for i in range(half)] + xs[half:]
    fx = {
        "curve": LABEL, "n": N, "a": str(a), "b": str(b), "z": str(z),
        "x": [str(v) for v in xs], "y": [str(v) for v in ys], "c": [str(v) for v in cs],
        "scaled": [str(a * v % q) for v in xs],
        "hadamard": [str(w * v % q) for w, v in zip(cs, xs)],
        "combined": [str((w * u + b * v) % q) for w, u, v in zip(cs, xs, ys)],
        "fold": [str(v) for v in fold],
        "dot": str(sum(u * v for u, v in zip(xs, ys)) % q),
        "sum": str(sum(xs) % q),
        "cross": str(sum(xs[i] * ys[half + i] for i in range(half)) % q),
        "powers": [str(b * pow(z, i, q) % q) for i in range(N)],
    }
    with open(os.path.join(HERE, "scalar_ops_js_fixture.json"), "w") as f:
        json.dump(fx, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

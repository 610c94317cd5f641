#!/usr/bin/env python3
"""Writes tests/golden/dot_many_js_fixture.json, the input and expected output of js/scripts/msm-dot-many.mjs
(tests/test_js_dot_many.py): BLS12-377, 6 rows x 3 columns of n = 70 scalars drawn from the operands of the scalar-set
tests (0 and q - 1 among them) and random values, two evaluation points.  Expected, from Python integers
(tests/dot_many_util.py): "values", the 6 x 3 inner products, and "evals", the rows as polynomials at the points.  All
scalars as decimal strings.

    python tests/golden/make_dot_many_fixture.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import dot_many_util as U          # noqa: E402
import scalar_ops_util as S        # noqa: E402


def main():
    label, n_rows, n_cols, n = "bls12-377", 6, 3, 70
    q = S.order(label)
    rows, cols = U.fixture_values(label, n_rows, n_cols, n, 3232)
    points = [q - 1, S.operands(label, 9)[20]]
    dec = lambda m: [[str(v) for v in r] for r in m]   # noqa: E731
    fx = {"curve": label, "n": n, "rows": dec(rows), "cols": dec(cols), "values": dec(U.products(rows, cols, q)),
          "points": [str(z) for z in points], "evals": dec([[U.horner(r, z, q) for z in points] for r in rows])}
    with open(os.path.join(HERE, "dot_many_js_fixture.json"), "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in fx.items()) + "\n}\n")   # (one key a line)


if __name__ == "__main__":
    main()

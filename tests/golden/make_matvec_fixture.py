#!/usr/bin/env python3
"""Writes tests/golden/matvec_js_fixture.json, the input and expected output of js/scripts/msm-matvec.mjs
(tests/test_js_matvec.py): BLS12-377, a 40 x 48 matrix of 150 triples in shuffled order with an empty row, an empty
column, a duplicate (row, col) pair and the values 0, 1 and q - 1 among random ones, a vector for each orientation with
0 and q - 1 planted; the expected products with values and without, both orientations, from Python integers
(tests/matrix_util.py), all scalars as decimal strings.

    python tests/golden/make_matvec_fixture.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import matrix_util as M         # noqa: E402
import scalar_ops_util as S     # noqa: E402


def main():
    label, n_rows, n_cols, nnz = "bls12-377", 40, 48, 150
    q = S.order(label)
    rng = random.Random(707)
    empty_row, empty_col = 17, 29
    rows = [rng.choice([r for r in range(n_rows) if r != empty_row]) for _ in range(nnz)]
    cols = [rng.choice([c for c in range(n_cols) if c != empty_col]) for _ in range(nnz)]
    rows[60], cols[60] = rows[3], cols[3]                     # a duplicate pair, far apart in the caller's order
    vals = M.values_for(nnz, q, rng)
    x, y = M.x_for(n_cols, q, rng), M.x_for(n_rows, q, rng)
    fx = {"curve": label, "shape": [n_rows, n_cols], "rows": rows, "cols": cols, "values": vals, "x": x, "y": y,
          "mx": M.matvec(rows, cols, vals, x, n_rows, q), "mty": M.matvec(rows, cols, vals, y, n_cols, q, transpose=True),
          "mxOnes": M.matvec(rows, cols, None, x, n_rows, q), "mtyOnes": M.matvec(rows, cols, None, y, n_cols, q, transpose=True)}
    out = {k: v if k in ("curve", "shape", "rows", "cols") else [str(e) for e in v] for k, v in fx.items()}
    with open(os.path.join(HERE, "matvec_js_fixture.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

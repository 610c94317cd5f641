#!/usr/bin/env python3
"""Writes tests/golden/lookup_js_fixture.json, the input and expected output of js/scripts/msm-lookup.mjs
(tests/test_js_lookup.py): BLS12-377, a table of 48 entries over 30 distinct values -- some twice, some three times, 0, 1
and q - 1 among them, in shuffled order -- and a column of 200 entries drawn from the table with 7 entries that are in
no table, the first of them at index 5; the multiplicities, the positions and the result words from Python integers
(tests/lookup_util.py), all scalars as decimal strings.

    python tests/golden/make_lookup_fixture.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lookup_util as L         # noqa: E402
import scalar_ops_util as S     # noqa: E402


def main():
    label = "bls12-377"
    q = S.order(label)
    rng = random.Random(909)
    values = [0, 1, q - 1] + L.distinct(27, q, rng, avoid=(0, 1, q - 1))
    table = values + values[:12] + values[:6]                 # 30 + 12 + 6 = 48: six values three times, six twice
    rng.shuffle(table)
    column = [rng.choice(table) for _ in range(200)]
    for at, v in zip((5, 63, 64, 100, 128, 177, 199), L.distinct(7, q, rng, avoid=table)):
        column[at] = v
    m, positions, info = L.model(table, column)
    fx = {"curve": label, "table": [str(v) for v in table], "column": [str(v) for v in column],
          "multiplicities": [str(v) for v in m], "positions": positions, "missing": info["missing"],
          "firstMissing": info["firstMissing"], "distinct": info["distinct"]}
    with open(os.path.join(HERE, "lookup_js_fixture.json"), "w") as f:
        json.dump(fx, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

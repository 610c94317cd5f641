#!/usr/bin/env python3
"""Writes tests/golden/mle_js_fixture.json, the input and expected output of js/scripts/msm-mle.mjs
(tests/test_js_mle.py): BLS12-377, v = 6, three tables with the planted rows of the scalar-set tests, a point with a 0, a
1 and q - 1 among its values, a scale, a challenge and two terms of mixed degree; the expected eq table, evaluations, both
binds and the round values in both orders from Python integers (tests/mle_util.py), all as decimal strings.

    python tests/golden/make_mle_fixture.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mle_util as M            # noqa: E402
import scalar_ops_util as S     # noqa: E402


def main():
    label, v = "bls12-377", 6
    q = S.order(label)
    rng = random.Random(606)
    n = 1 << v
    a, b = S.build_vectors(label, n, 61)
    c, _ = S.build_vectors(label, n, 62)
    tables = [a, b, c]
    point = [rng.randrange(2, q), 0, q - 1, rng.randrange(2, q), 1, rng.randrange(2, q)]
    scale, r = rng.randrange(2, q), rng.randrange(2, q)
    terms = [(None, 0b011), (q - 1, 0b100)]          # A B - C: degree 2 and degree 1 in one call
    fx = {"curve": label, "nVars": v, "tables": tables, "point": point, "scale": scale, "r": r,
          "terms": [[None if co is None else str(co), m] for co, m in terms],
          "eq": M.eq(point, q, scale), "evals": [M.mle_eval(t, point, q) for t in tables],
          "bindHigh": sum((M.bind(t, r, q) for t in tables), []), "bindLow": sum((M.bind(t, r, q, True) for t in tables), []),
          "inPlace": M.bind(a, r, q) + a[n // 2:],
          "roundHigh": M.round_poly(tables, terms, q), "roundLow": M.round_poly(tables, terms, q, True)}

    def dec(x):
        """scalars as decimal strings, lists kept"""
        return [dec(e) for e in x] if isinstance(x, list) else str(x)

    out = {k: val if k in ("curve", "nVars", "terms") else dec(val) for k, val in fx.items()}
    with open(os.path.join(HERE, "mle_js_fixture.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

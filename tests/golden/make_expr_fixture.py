#!/usr/bin/env python3
"""Writes tests/golden/expr_js_fixture.json, the input and expected output of js/scripts/msm-expr.mjs
(tests/test_js_expr.py): BLS12-377, eight columns of 70 entries over {0, 1, q - 1, random}, and five expressions from
tests/expr_util.py -- the PLONK arithmetic gate, one wire of the permutation step (a rotated operand), the S-box gate (a
repeated factor), one column at three rotations in one term with rotations of 2^31 - 1 and -2^31 beside it, and -a^8
next to a constant -- each with the values of the Python-integer model; then y and the values of out = y out + gate over
the first three, evaluated in place.  All scalars as decimal strings; a term is [coefficient or null, [[column, rot]]].

    python tests/golden/make_expr_fixture.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import expr_util as E           # noqa: E402
import scalar_ops_util as S     # noqa: E402


def main():
    label = "bls12-377"
    q = S.order(label)
    rng = random.Random(2909)
    n = 70
    columns = E.edge_columns(8, n, q, rng)
    r = lambda: rng.randrange(q)   # noqa: E731
    exprs = {
        "plonk": E.plonk_gate(),
        "permutation": E.permutation_wire(r(), r(), q),
        "sbox": E.sbox_gate(r(), q),
        "rotations": [(r(), [(0, 1), (0, -1), (0, 2), 1]), (None, [(2, E.INT32_MAX), (3, E.INT32_MIN)]), (0, [4])],
        "a8": [(q - 1, [6] * 8), (r(), [])],
    }
    y = r()
    acc = [0] * n
    for name in ("plonk", "permutation", "sbox"):
        acc = [(y * a + g) % q for a, g in zip(acc, E.model(columns, exprs[name], n, q))]
    fx = {"curve": label, "n": n, "columns": [[str(v) for v in col] for col in columns],
          "expressions": {name: {"terms": [[None if c is None else str(c), [list(E.factor(f)) for f in fs]] for c, fs in terms],
                                 "expected": [str(v) for v in E.model(columns, terms, n, q)]} for name, terms in exprs.items()},
          "y": str(y), "accumulated": [str(v) for v in acc]}
    with open(os.path.join(HERE, "expr_js_fixture.json"), "w") as f:
        json.dump(fx, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/sumcheck_step_js_fixture.json, the input and expected output of js/scripts/msm-sumcheck-step.mjs
(tests/test_js_sumcheck_step.py): BLS12-377, v = 6, three tables with the planted rows of the scalar-set tests, two terms
of mixed degree and six challenges (a 0-free mix with q - 1 and 1 among them).  Expected, from Python integers
(tests/sumcheck_step_util.py), per order "high" and "low": the values of three consecutive steps, the three tables of 2^3
entries they leave, the last-variable step on entries [0, 2) of those tables (its value and the bound entries), and a
whole protocol over the six challenges (round polynomials and final claim).  All scalars as decimal strings.

    python tests/golden/make_sumcheck_step_fixture.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import scalar_ops_util as S        # noqa: E402
import sumcheck_step_util as U     # noqa: E402


def main():
    label, v = "bls12-377", 6
    q = S.order(label)
    rng = random.Random(3030)
    n = 1 << v
    a, b = S.build_vectors(label, n, 63)
    c, _ = S.build_vectors(label, n, 64)
    tables = [a, b, c]
    terms = [(None, 0b011), (q - 1, 0b100)]          # A B - C: degree 2 and degree 1 in one call
    challenges = [rng.randrange(2, q), q - 1, rng.randrange(2, q), 1, rng.randrange(2, q), rng.randrange(2, q)]
    fx = {"curve": label, "nVars": v, "tables": tables, "challenges": challenges,
          "terms": [[None if co is None else str(co), m] for co, m in terms]}
    for low in (False, True):
        cur, steps = tables, []
        for k in range(3):
            cur, _, values = U.step(cur, terms, challenges[k], q, low)
            steps.append(values)
        last_tables, degree, last = U.step([t[:2] for t in cur], terms, challenges[3], q, low)
        assert degree == 0
        polys, _, claim, _ = U.prove(tables, terms, q, lambda values, it=iter(challenges): next(it), low)
        fx["low" if low else "high"] = {"steps": steps, "tables": cur, "last": last[0], "lastTables": [t[0] for t in last_tables],
                                        "polys": polys, "claim": claim}

    def dec(x):
        """scalars as decimal strings, lists and dicts kept"""
        if isinstance(x, dict):
            return {k: dec(e) for k, e in x.items()}
        return [dec(e) for e in x] if isinstance(x, list) else str(x)

    out = {k: val if k in ("curve", "nVars", "terms") else dec(val) for k, val in fx.items()}
    with open(os.path.join(HERE, "sumcheck_step_js_fixture.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

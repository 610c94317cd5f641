"""The yardstick of the sumcheck-step tests (tests/test_sumcheck_step_cpu.py, tests/test_sumcheck_step_gpu.py,
tests/test_js_sumcheck_step.py, tests/golden/make_sumcheck_step_fixture.py): Python integers mod q over lists, on top of
tests/mle_util.py.  A step binds one variable of every table to r and returns the round polynomial over the bound
tables (include/msmz.h, msmz_scalars_sumcheck_step)."""
import mle_util as M


def claim(bound, terms, q):
    """sum_T c_T prod_(j in T) bound_j[0] over one-entry tables: what is left when no variable is"""
    total = 0
    for c, mask in terms:
        p = 1 if c is None else c
        for j, f in enumerate(bound):
            if (mask >> j) & 1:
                p = p * f[0] % q
        total += p
    return total % q


def step(tables, terms, r, q, low=False):
    """-> (bound tables, degree, [g(0) .. g(degree)]): bind of every table, then the round over what it gave; tables of one
    variable: degree 0 and the claim"""
    bound = [M.bind(f, r, q, low) for f in tables]
    if len(bound[0]) == 1:
        return bound, 0, [claim(bound, terms, q)]
    values = M.round_poly(bound, terms, q, low)
    return bound, len(values) - 1, values


def prove(tables, terms, q, challenge, low=False):
    """the prover of a whole sumcheck by the two-call route of the model -> (polys, challenges, claim, final tables)"""
    cur = [list(f) for f in tables]
    polys, challenges = [M.round_poly(cur, terms, q, low)], []
    while True:
        r = challenge(list(polys[-1]))
        challenges.append(r)
        cur, _, values = step(cur, terms, r, q, low)
        if len(cur[0]) == 1:
            return polys, challenges, values[0], cur
        polys.append(values)


def mixed_terms(nt, q, rng):
    """terms of mixed degree over nt tables: a product of up to four tables with a random coefficient, one table alone with
    coefficient NULL (1), and with three tables or more a pair with coefficient q - 1"""
    top = min(nt, 4)
    terms = [(rng.randrange(2, q), ((1 << top) - 1) << (nt - top)), (None, 1)]
    if nt >= 3:
        terms.append((q - 1, 0b110))
    return terms

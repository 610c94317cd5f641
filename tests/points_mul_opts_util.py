"""Shared by the msmz_points_mul_opts tests (tests/test_points_mul_opts_cpu.py, tests/test_points_mul_opts_gpu.py,
tests/test_js_points_mul_opts.py, tests/golden/make_points_mul_opts_fixture.py): the scalars and bounds of the issue,
sets of subgroup points, and the chain the engine owes a call.  What [s]P (+ Q) is stays with points_mul_util (the
oracle)."""
import random

import check_points_util as U
import points_mul_util as M
from oracle import params as P

ALL = M.ALL
WEIER = [label for label in ALL if P.CURVES[label]["kind"] == "weierstrass"]
MSMZ_MUL_SUBGROUP = 1
PLAIN, GLV = 0, 1
# Fr::GLV_PROVEN_BITS (csrc/constants_gen.h): the length of the GLV chain; 0 = the curve has no endomorphism
GLV_PROVEN_BITS = {"bls12-377": 126, "pallas": 128, "bls12-381": 128, "ed-on-bls12-377": 0}
BOUNDS = [1, 31, 32, 33, 64, 128, 129, 200]   # and the bit length of q


def order_bits(label):
    return P.CURVES[label]["order"].bit_length()


def lam(label):
    return P.CURVES[label]["endomorphism"]["lambda_"]


def glv_scalars(label, rng):
    """0, 1, 2, 3, q - 1, lambda, lambda +- 1, q - lambda, the powers of two at the word boundaries of both walks, 16 random"""
    q, l = P.CURVES[label]["order"], lam(label)
    return ([0, 1, 2, 3, q - 1, l, l + 1, l - 1, q - l] + [1 << k for k in (31, 32, 63, 64, 95, 96, 125, 126, 127, 128, 224)] +
            [rng.randrange(q) for _ in range(16)])


def bounded_scalars(label, b, rng, count=3):
    """scalars below 2^b (and below q): 0, 1, the largest, the top bit alone, `count` random"""
    top = min(1 << b, P.CURVES[label]["order"])
    return sorted({0, 1 % top, top - 1, 1 << (min(b, order_bits(label)) - 1)}) + [rng.randrange(top) for _ in range(count)]


def subgroup_set(label, n, seed):
    """rows (s, P, Q) like points_mul_util.build_set -- s = 0, 1, q - 1, P and Q at infinity, Q = +-[s]P in the first
    wave and in the last one -- with every P in the prime-order subgroup: the rows of a named small-order point give
    way to multiples of G (Q is not constrained and stays)"""
    params = P.CURVES[label]
    rng = random.Random(seed + 99)
    g = U.generator(params)
    small = [pt for pt, _, _ in M.small_order_rows(label)]
    rows = []
    for s, p, q in M.build_set(label, n, seed):
        if p in small:
            p = U.scale(params, rng.randrange(1, params["order"]), g)
        rows.append((s, p, q))
    return rows


def chain(label, subgroup, b):
    """(kind, steps) of a call, by the three rules of the issue"""
    bits, h = order_bits(label), GLV_PROVEN_BITS[label]
    eff = bits if b == 0 or b >= bits else b
    if eff < bits and eff <= h:
        return PLAIN, eff
    if subgroup and h:
        return GLV, h
    return PLAIN, eff

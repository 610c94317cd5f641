"""What the transform tests share: the roots of unity and the number-theoretic transform over Python integers, the input
vectors, and the plan as the library reports it.  Nothing here touches a GPU."""
import ctypes as C
import random

import scalar_ops_util as S
from oracle import params as P

# the multiplicative generators of the scalar fields that arkworks, pasta_curves and bls12_381 use
GENERATOR = {"bls12-377": 22, "pallas": 5, "bls12-381": 7, "ed-on-bls12-377": 5}
INVERSE, COSET = 1, 2


def two_adicity(label):
    q = S.order(label)
    return ((q - 1) & -(q - 1)).bit_length() - 1


def root_max(label):
    q = S.order(label)
    return pow(GENERATOR[label], (q - 1) >> two_adicity(label), q)


def root(label, log_n):
    return pow(root_max(label), 1 << (two_adicity(label) - log_n), S.order(label))


def ntt(q, x, w):
    """sum_i x_i w^(i k) for k < len(x), a power of two: the textbook recursion on Python integers"""
    n = len(x)
    if n == 1:
        return list(x)
    w2 = w * w % q
    even, odd = ntt(q, x[0::2], w2), ntt(q, x[1::2], w2)
    out, t, h = [0] * n, 1, n // 2
    for k in range(h):
        v = t * odd[k] % q
        out[k], out[k + h] = (even[k] + v) % q, (even[k] - v) % q
        t = t * w % q
    return out


def transform(q, x, n, w, inverse=False, shift=None):
    """what msmz_scalars_ntt computes for ONE vector x of at most n entries"""
    x = list(x) + [0] * (n - len(x))
    g = 1 if shift is None else shift
    if not inverse:
        return ntt(q, [v * pow(g, i, q) % q for i, v in enumerate(x)], w)
    ninv, ginv = pow(n, -1, q), pow(g, -1, q)
    return [v * ninv * pow(ginv, i, q) % q for i, v in enumerate(ntt(q, x, pow(w, -1, q)))]


def inputs(label, n, seed):
    """n scalars: 0, 1, q - 1, the value with full low words (as far as n goes), then random values"""
    q = S.order(label)
    rng = random.Random(seed)
    head = [0, 1, q - 1, S.low_words_full(q), q - 2]
    return (head + [rng.randrange(q) for _ in range(max(0, n - len(head)))])[:n]


def plan(lib, curve_id, log_n):
    """(status, stages per pass) of msmz_test_ntt_plan"""
    n, stages = C.c_uint32(0), (C.c_uint32 * 8)()
    st = lib.msmz_test_ntt_plan(curve_id, log_n, C.byref(n), stages)
    return st, list(stages)[:n.value]


def pass_log(lib):
    v = C.c_uint32(0)
    lib.msmz_test_ntt_geometry(C.byref(v))
    return v.value


def curve_id(label):
    return P.CURVES[label]["curve_id"]

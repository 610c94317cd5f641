"""Shared by the msmz_points_fixed_base tests (tests/test_fixed_base_cpu.py, tests/test_fixed_base_gpu.py,
tests/test_js_fixed_base.py, tests/golden/make_fixed_base_fixture.py): the digit rule restated in Python integers, the
scalars the issue asks for at every window boundary, the bases, and what [s]B is by the oracle (the C oracle's scale,
oracle/msm_oracle.c, which tests/test_oracle.py holds to oracle/bigint_ref.py)."""
import random

import check_points_util as U
import points_mul_util as M
from oracle import c_oracle
from oracle import params as P

ALL = U.ALL
WIDTHS = [4, 5, 13, 16]          # the window widths of the issue: the narrowest, an odd one, the generators', the widest
BOUNDS = [1, 64, 128, 0]         # scalar_bits; 0 = none


def order_bits(params):
    return params["order"].bit_length()


def bound_bits(params, scalar_bits):
    """fixed_base_bits: the caller's bound, at most the bit length of the group order"""
    b = order_bits(params)
    return b if scalar_bits <= 0 or scalar_bits >= b else scalar_bits


def windows(bits, c):
    """K = ceil((bits + 1) / c)"""
    return -(-(bits + 1) // c)


def digits(s, c, K):
    """the signed digits of the 256-bit value s, bottom first, by the rule of fixed_base.h: every window masked to c bits,
    raw > 2^(c-1) borrows 2^c from the window above, the carry out of window K - 1 dropped"""
    out, carry = [], 0
    for k in range(K):
        raw = ((s >> (c * k)) & ((1 << c) - 1)) + carry
        carry = 1 if raw > (1 << (c - 1)) else 0
        out.append(raw - (carry << c))
    return out


def edge_scalars(params, c, scalar_bits, rng, n_random=16):
    """the scalars of the issue for one (c, bound), every one below min(q, 2^bits): 0, 1, 2, q - 1; 2^(ck) - 1, 2^(ck),
    2^(ck) + 1 at every window boundary; every digit 2^(c-1) and every digit 2^(c-1) + 1 (a carry through every window);
    random ones.  What does not fit the bound is cut to it (mod 2^bits), what is not below q is dropped."""
    q = params["order"]
    bits = bound_bits(params, scalar_bits)
    K = windows(bits, c)
    top = min(q, 1 << bits)
    vals = [0, 1, 2, q - 1]
    for k in range(1, K + 1):
        vals += [(1 << (c * k)) - 1, 1 << (c * k), (1 << (c * k)) + 1]
    half = 1 << (c - 1)
    vals += [sum(half << (c * k) for k in range(K)), sum((half + 1) << (c * k) for k in range(K))]
    vals = [v % (1 << bits) for v in vals]
    vals += [rng.randrange(top) for _ in range(n_random)]
    seen, out = set(), []
    for v in vals:
        if v < top and v not in seen:
            seen.add(v)
            out.append(v)
    return out


def bases(label, rng):
    """(name, point): the generator, a random multiple of it, every on-curve named point of the check-points tests (small
    orders on the cofactor curves), the point at infinity / the twisted Edwards identity"""
    params = P.CURVES[label]
    g = U.generator(params)
    out = [("G", g), ("[k]G", U.scale(params, rng.randrange(1, params["order"]), g))]
    out += [(f"named {i}", q) for i, q in enumerate(M.on_curve_named(label))]
    out.append(("neutral", M.neutral(params)))
    return out


_scaled = {}


def expected(label, s, base):
    """[s]base as msmz_download_points gives it, by the C oracle; remembered per (curve, s, base)"""
    params = P.CURVES[label]
    key = (label, s, base["x"], base["y"], base["isZero"])
    if key not in _scaled:
        if params["kind"] == "weierstrass" and base["isZero"]:
            r = M.neutral(params)
        else:
            r = c_oracle.scale(params, s, base)
            r = U.pt(r["x"] % params["modulus"], r["y"] % params["modulus"], r["isZero"])
        _scaled[key] = M.canon(params, r)
    return _scaled[key]


def gpu_scalars(params, n, seed):
    """n scalars for a GPU set: the edge scalars of the widths 4 and 13 without a bound in the first positions, then
    seeded random ones"""
    rng = random.Random(seed)
    head = []
    for c in (13, 4):
        for v in edge_scalars(params, c, 0, rng, 0):
            if v not in head:
                head.append(v)
    q = params["order"]
    return (head + [rng.randrange(q) for _ in range(max(0, n - len(head)))])[:n]

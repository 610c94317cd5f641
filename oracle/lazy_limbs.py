"""Register-limb forms of the lazy field arithmetic (msm_zprize_amd/csrc/fp.h) in plain Python integers, and the edge
cases of its contract.  Shared by the host contract test (tests/test_fp_contract.py) and the device test
(tests/test_lazy_contract_gpu.py), so both feed the same limbs to the same routines.

A register value is sum l[j] * 2^(W*j) over N signed 32-bit limbs; limbs may be negative or wider than W bits."""
import math
import random

from oracle import params as P

# label -> (modulus, N limbs, W bits); the Montgomery radix is R = 2^(N*W)
FIELDS = {
    "bls12-377": (P.BLS12_377["modulus"], 14, 28),
    "bls12-381": (P.BLS12_381["modulus"], 14, 28),
    "pallas": (P.PALLAS["modulus"], 9, 29),
    "ed-on-bls12-377": (P.ED_ON_BLS12_377["modulus"], 9, 29),
}
DRIVER_NAME = {"bls12-377": "bls377", "bls12-381": "bls381", "pallas": "pallas", "ed-on-bls12-377": "ed377"}

# ops of msmz_test_field_limbs / field_limbs_op (csrc/test_ops.h)
(TFL_MUL, TFL_SQR, TFL_REDUCE_SMALL, TFL_STORE, TFL_STORE_MULOUT, TFL_IS_ZERO, TFL_CARRY, TFL_NORMALIZE, TFL_INVERSE,
 TFL_INVERSE_WAVE, TFL_SLOT_MULOUT, TFL_SLOT_POINT) = range(12)

I32 = 1 << 31


def mul_bound(label):
    """fe_mul / fe_sqr accept |v| < MUL_BOUND * p"""
    return 32 if FIELDS[label][1] == 14 else 8


def max_limb_product_limb(label):
    """largest A with N*A*A + N*2^(2W) < 2^63: the widest limbs two mul operands may both have"""
    _, n, w = FIELDS[label]
    return math.isqrt(((1 << 63) - 1 - n * (1 << (2 * w))) // n)


def value(limbs, w):
    return sum(l << (w * j) for j, l in enumerate(limbs))


def normalized(v, n, w):
    """limbs 0..N-2 in [0, 2^W), signed top limb (fe_normalize form; also a mul output's form)"""
    mask = (1 << w) - 1
    out = []
    for _ in range(n - 1):
        out.append(v & mask)
        v >>= w
    out.append(v)
    assert -I32 <= out[-1] < I32
    return out


def carry(limbs, w):
    """fe_carry: one parallel carry pass"""
    n = len(limbs)
    mask = (1 << w) - 1
    c = [limbs[j] >> w for j in range(n - 1)]
    r = list(limbs)
    for j in range(n - 2, 0, -1):
        r[j] = (limbs[j] & mask) + c[j - 1]
    r[0] = limbs[0] & mask
    r[n - 1] = limbs[n - 1] + c[n - 2]
    return r


def widened(v, n, w, amax, rng):
    """limbs of v as wide as |l| <= amax allows: each low limb pushed towards +-amax by borrowing from the next"""
    limbs = normalized(v, n, w)
    for j in range(n - 1):
        target = amax if rng.random() < 0.5 else -amax
        k = (target - limbs[j]) >> w
        lo = limbs[j] + (k << w)
        if abs(lo) > amax:
            k += 1 if lo < 0 else -1
            lo = limbs[j] + (k << w)
        limbs[j] = lo
        limbs[j + 1] -= k
    assert value(limbs, w) == v and max(abs(l) for l in limbs) <= max(amax, abs(limbs[-1]))
    return limbs


def lazy_sum(v, label, rng, terms=4):
    """v as the limb-wise sum / difference of `terms` values in mul-output form (-1.5p, 0.5p), no carry -- what a
    chain of fe_add / fe_sub between products leaves; the last term absorbs the rest in normalized form"""
    p, n, w = FIELDS[label]
    acc = [0] * n
    rest = v
    for _ in range(terms - 1):
        t = rng.randrange(-3 * p // 2 + 1, p // 2)
        s = rng.choice((1, -1))
        acc = [a + s * l for a, l in zip(acc, normalized(t, n, w))]
        rest -= s * t
    acc = [a + l for a, l in zip(acc, normalized(rest, n, w))]
    assert value(acc, w) == v
    return acc


def forms(v, label, rng):
    """the three limb forms of the issue: normalized, fe_carry output, uncarried sum of mul outputs"""
    p, n, w = FIELDS[label]
    lazy = lazy_sum(v, label, rng)
    return {"normalized": normalized(v, n, w), "carried": carry(lazy, w), "lazy": lazy}


def reduce_cases(label, seed=1):
    """fe_reduce_small / fe_store inputs: k p - 1, k p, k p + 1 for k in [-16, 15] (|v| < 16 p only), three forms"""
    p, n, w = FIELDS[label]
    rng = random.Random(seed)
    out = []
    for k in range(-16, 16):
        for d in (-1, 0, 1):
            v = k * p + d
            if abs(v) >= 16 * p:
                continue
            for name, limbs in forms(v, label, rng).items():
                out.append((f"{k}p{d:+d}/{name}", limbs))
    for e in (-16 * p + 1, 16 * p - 1, -(1 << (w * (n - 1))), 15 * p + p // 2, -15 * p - p // 2):
        for name, limbs in forms(e, label, rng).items():
            out.append((f"{e / p:.3f}p/{name}", limbs))
    return out


def is_zero_cases(label, seed=2):
    """fe_is_zero: k p for |k| <= 15 spread over the limbs in several ways, near misses k p +- 1 and k p +- 2^W, and
    k p + m 2^(W j) (limb 0 passes the quick filter, the full reduction has to answer)"""
    p, n, w = FIELDS[label]
    rng = random.Random(seed)
    amax = (1 << (w + 2))
    out = []
    for k in range(-15, 16):
        for v, want in [(k * p, True), (k * p + 1, False), (k * p - 1, False), (k * p + (1 << w), False),
                        (k * p - (1 << w), False), (k * p + (rng.randrange(1, 64) << (w * rng.randrange(1, n - 1))), False)]:
            if abs(v) >= 16 * p:
                continue
            fs = forms(v, label, rng)
            fs["widened"] = widened(v, n, w, amax, rng)
            for name, limbs in fs.items():
                out.append((f"{v - k * p:+d}+{k}p/{name}", limbs, want))
    return out


def mul_cases(label, seed=3):
    """fe_mul / fe_sqr operands at +-(bound p - 1) and random values, limbs widened to the product limit"""
    p, n, w = FIELDS[label]
    rng = random.Random(seed)
    vb = mul_bound(label)
    amax = max_limb_product_limb(label)
    edge = [vb * p - 1, -(vb * p - 1), vb * p - 2, 0, 1, -1, p, -p]
    vals = edge + [rng.randrange(-vb * p + 1, vb * p) for _ in range(24)]
    out = []
    for i, a in enumerate(vals):
        b = vals[(i * 7 + 3) % len(vals)]
        out.append((a, widened(a, n, w, amax, rng), b, widened(b, n, w, amax, rng)))
        out.append((a, normalized(a, n, w), b, widened(b, n, w, amax, rng)))
    return out


def mulout_cases(label, seed=4):
    """fe_store_mulout inputs: mul-output form, value in (-1.5p, 0.5p) incl. both ends"""
    p, n, w = FIELDS[label]
    rng = random.Random(seed)
    vals = [-3 * p // 2 + 1, p // 2, 0, -1, 1, -p, -p + 1, -p - 1]   # p odd: p // 2 is the largest value < p / 2
    vals += [rng.randrange(-3 * p // 2 + 1, p // 2) for _ in range(24)]
    return [(v, normalized(v, n, w)) for v in vals]


def field_limb_cases(label):
    """(op, a limbs, b limbs) for every edge case above, on the ops the host driver and the device both run"""
    _, n, _ = FIELDS[label]
    zero = [0] * n
    cases = []
    for _, la, _, lb in mul_cases(label):
        cases.append((TFL_MUL, la, lb))
        cases.append((TFL_SQR, la, zero))
        cases.append((TFL_SQR, lb, zero))
    for _, limbs in reduce_cases(label):
        for op in (TFL_REDUCE_SMALL, TFL_STORE, TFL_CARRY, TFL_NORMALIZE):
            cases.append((op, limbs, zero))
    for _, limbs, _ in is_zero_cases(label):
        cases.append((TFL_IS_ZERO, limbs, zero))
    for _, limbs in mulout_cases(label):
        cases.append((TFL_STORE_MULOUT, limbs, zero))
    for _, limbs in reduce_cases(label)[::7]:
        cases.append((TFL_INVERSE, limbs, zero))
    return cases


def check_field_limb_result(label, op, a, b, raw, canon):
    """the contract of each routine on raw limbs, against Python integers"""
    p, n, w = FIELDS[label]
    R = 1 << (n * w)
    va, vb = value(a, w), value(b, w)
    nwords = 12 if n == 14 else 8
    if op in (TFL_MUL, TFL_SQR):
        want = (va * (vb if op == TFL_MUL else va)) * pow(R, -1, p) % p
        v = value(raw, w)
        assert -3 * p < 2 * v < p and all(0 <= l < (1 << w) for l in raw[:-1])
        assert v % p == want and canon == want
    elif op in (TFL_REDUCE_SMALL, TFL_INVERSE, TFL_INVERSE_WAVE):
        v = value(raw, w)
        if op == TFL_REDUCE_SMALL:
            assert 0 <= v < 3 * p and all(0 <= l < (1 << w) for l in raw) and (v - va) % p == 0
            assert canon == va % p
        else:
            assert canon == (0 if va % p == 0 else R * R * pow(va, -1, p) % p)
    elif op in (TFL_STORE, TFL_STORE_MULOUT, TFL_SLOT_MULOUT):
        if op == TFL_SLOT_MULOUT:
            v = value(raw, w)
        else:
            assert all(x == 0 for x in raw[nwords:])
            v = sum((x & 0xffffffff) << (32 * i) for i, x in enumerate(raw[:nwords]))
        assert 0 <= v < 3 * p and (v - va) % p == 0 and canon == va % p
    elif op == TFL_IS_ZERO:
        assert raw[0] == (1 if va % p == 0 else 0) and all(x == 0 for x in raw[1:])
    elif op in (TFL_CARRY, TFL_NORMALIZE):
        assert value(raw, w) == va
        lim = (1 << w) if op == TFL_NORMALIZE else (1 << w) + 64
        assert all(0 <= l < lim for l in raw[:-1]) if op == TFL_NORMALIZE else all(-64 <= l < lim for l in raw[:-1])
    elif op == TFL_SLOT_POINT:
        vy = value(raw, w)
        assert 0 <= vy < 3 * p and (vy - vb) % p == 0 and canon == va % p
    else:
        raise AssertionError(op)

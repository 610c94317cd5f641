"""The row form of the field arithmetic (msm_zprize_amd/csrc/fp_rows.h) on the device: one element per DPP row, limb j
in lane j, four elements per wave.  msmz_test_field_rows loads caller-chosen RAW limbs unchanged, so the row product
runs on the edges of its contract -- operands 0, 1, p - 1, p, 3p - 1, mul outputs with a negative top limb, lazy sums
and differences up to the mul bound, limbs widened to the product limit, limbs outside [0, 2^W) -- and on 2 000 random
pairs.  Every result is checked against Python integers (oracle/bigint_ref.py arithmetic on the limb values), must meet
the output contract of fe_mul limb by limb, and must equal what the per-lane fe_mul returns for the same limbs: the
same limbs, not only the same residue, because a normalized value has one limb form."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import lazy_limbs as LZ

pytestmark = pytest.mark.gpu

CURVES = ["bls12-377", "pallas", "bls12-381", "ed-on-bls12-377"]
TFR_MUL, TFR_ROUNDTRIP, TFR_IS_ZERO = range(3)


@pytest.fixture(scope="module")
def ctxs():
    import msm_zprize_amd as m
    m.startThreads()
    cache = {}

    def get(label):
        if label not in cache:
            params = m.curves.BY_LABEL[label]
            cache[label] = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
        return cache[label]

    yield get
    for c in cache.values():
        c.close()


def _run(curve, label, hook, op, a, b, live_rows=None):
    """one launch of msmz_test_field_rows (live_rows given) or msmz_test_field_limbs on the limb lists a, b"""
    from msm_zprize_amd import _native
    _, n, _ = LZ.FIELDS[label]
    fb = curve.fe_bytes
    A = np.ascontiguousarray(np.array(a, dtype=np.int64).astype(np.int32))
    Bv = np.ascontiguousarray(np.array(b, dtype=np.int64).astype(np.int32))
    raw = np.zeros((len(a), n), dtype=np.int32)
    canon = C.create_string_buffer(fb * len(a))
    lib = _native.lib()
    if hook == "rows":
        st = lib.msmz_test_field_rows(curve._ctx, op, A.ctypes.data, Bv.ctypes.data, len(a), live_rows, raw.ctypes.data,
                                      canon)
    else:
        st = lib.msmz_test_field_limbs(curve._ctx, op, A.ctypes.data, Bv.ctypes.data, len(a), raw.ctypes.data, canon)
    assert st == 0, st
    return ([[int(x) for x in r] for r in raw],
            [int.from_bytes(canon.raw[fb * k:fb * (k + 1)], "little") for k in range(len(a))])


def _mul_pairs(label):
    """(a limbs, b limbs): the edges of the product's contract, then 2 000 random pairs"""
    p, n, w = LZ.FIELDS[label]
    rng = random.Random(77 + CURVES.index(label))
    vb = LZ.mul_bound(label)
    amax = LZ.max_limb_product_limb(label)
    norm = lambda v: LZ.normalized(v, n, w)
    pairs = []
    # 0, 1, p - 1, p, 3p - 1 against each other, normalized
    small = [0, 1, p - 1, p, 3 * p - 1]
    pairs += [(norm(x), norm(y)) for x in small for y in small]
    # mul outputs: (-1.5p, 0.5p), negative top limb
    mulout = [l for _, l in LZ.mulout_cases(label)]
    pairs += [(mulout[i], mulout[(i * 5 + 2) % len(mulout)]) for i in range(len(mulout))]
    # the edge and random cases of the per-lane product: +-(bound p - 1), limbs widened to the product limit
    pairs += [(la, lb) for _, la, _, lb in LZ.mul_cases(label)]
    # lazy sums and differences of mul outputs, up to the bound, uncarried and after one carry pass
    # (as many terms on the two sides as the limb-product limit N A B + N 2^(2W) < 2^63 leaves room for)
    ta, tb = (4, 2) if n == 14 else (2, 1)
    for v in [vb * p - 1, -(vb * p - 1), 4 * p, -4 * p + 1] + [rng.randrange(-vb * p + 1, vb * p) for _ in range(12)]:
        u = rng.randrange(-vb * p + 1, vb * p)
        la, lb = LZ.lazy_sum(v, label, rng, ta), LZ.lazy_sum(u, label, rng, tb)
        pairs += [(la, lb), (lb, la), (LZ.carry(la, w), lb)]
    # limbs outside [0, 2^W): negative and wider -- the widest limbs the limit allows against normalized ones, and
    # the widest that both operands may have
    big = min((1 << 31) - 1, (((1 << 63) - 1 - n * (1 << (2 * w))) // n) >> w)
    for v in [p - 1, -p, 3 * p - 1, rng.randrange(p)]:
        pairs.append((LZ.widened(v, n, w, big, rng), norm(rng.randrange(p))))
        pairs.append((norm(rng.randrange(p)), LZ.widened(v, n, w, big, rng)))
        pairs.append((LZ.widened(v, n, w, amax, rng), LZ.widened(-v, n, w, amax, rng)))
    edge = len(pairs)
    pairs += [(norm(rng.randrange(3 * p)), norm(rng.randrange(3 * p))) for _ in range(2000)]
    for la, lb in pairs:   # inside the contract of fe_mul (fp.h), which the row product's contains
        A, Bm = max(abs(x) for x in la), max(abs(x) for x in lb)
        assert n * A * Bm + n * (1 << (2 * w)) < (1 << 63) and abs(LZ.value(la, w)) < vb * p > abs(LZ.value(lb, w))
        assert all(-(1 << 31) <= x < (1 << 31) for x in la + lb)
    return pairs, edge


@pytest.mark.parametrize("label", CURVES)
def test_row_product(ctxs, label):
    """every row of every wave live: four different products in the four rows of one wave"""
    curve = ctxs(label)
    pairs, edge = _mul_pairs(label)
    assert edge > 100 and len(pairs) == edge + 2000
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    raw, canon = _run(curve, label, "rows", TFR_MUL, a, b, 15)
    lraw, lcanon = _run(curve, label, "limbs", LZ.TFL_MUL, a, b)
    for k, (la, lb) in enumerate(pairs):
        try:
            LZ.check_field_limb_result(label, LZ.TFL_MUL, la, lb, raw[k], canon[k])   # value, output contract, canon
        except AssertionError as e:
            raise AssertionError(f"pair {k} a={la} b={lb} -> raw {raw[k]} canon {canon[k]:x}") from e
        assert raw[k] == lraw[k] and canon[k] == lcanon[k], (k, la, lb)


@pytest.mark.parametrize("live_rows", [1, 2, 4, 8, 5, 10, 14, 7])
@pytest.mark.parametrize("label", ["bls12-377", "ed-on-bls12-377"])
def test_row_product_some_rows_live(ctxs, label, live_rows):
    """waves with only some rows holding an element, the others running on zeros (both limb shapes)"""
    curve = ctxs(label)
    pairs, edge = _mul_pairs(label)
    pairs = pairs[:edge:3] + pairs[edge:edge + 61]   # a count that fills the last wave only partly
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    raw, canon = _run(curve, label, "rows", TFR_MUL, a, b, live_rows)
    for k, (la, lb) in enumerate(pairs):
        LZ.check_field_limb_result(label, LZ.TFL_MUL, la, lb, raw[k], canon[k])


@pytest.mark.parametrize("label", CURVES)
def test_row_load_store_round_trip(ctxs, label):
    """fe_load_row -> fe_store_row on memory words in [0, 3p) and on the all-zero record: the words come back in THE
    memory range, the same residue, and exactly the words the per-lane fe_store writes for the same limbs"""
    curve = ctxs(label)
    p, n, w = LZ.FIELDS[label]
    nwords = 12 if n == 14 else 8
    rng = random.Random(5 + CURVES.index(label))
    vals = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 3 * p - 1] + [rng.randrange(3 * p) for _ in range(119)]
    words = [[(v >> (32 * i)) & 0xffffffff for i in range(nwords)] + [0] * (n - nwords) for v in vals]
    zero = [[0] * n] * len(vals)
    for live_rows in (15, 6):
        raw, canon = _run(curve, label, "rows", TFR_ROUNDTRIP, words, zero, live_rows)
        sraw, _ = _run(curve, label, "limbs", LZ.TFL_STORE, [LZ.normalized(v, n, w) for v in vals], zero)
        for k, v in enumerate(vals):
            got = sum((x & 0xffffffff) << (32 * i) for i, x in enumerate(raw[k][:nwords]))
            assert all(x == 0 for x in raw[k][nwords:]) and 0 <= got < 3 * p and (got - v) % p == 0, (k, v)
            assert canon[k] == v % p and raw[k] == sraw[k], (k, v)   # (k = 0: the all-zero record, stored as fe_store does)


@pytest.mark.parametrize("label", CURVES)
def test_row_is_zero(ctxs, label):
    """fe_is_zero_row on k p for |k| <= 15 in several limb forms (0, p, 2p, -p among them) and on the near misses"""
    curve = ctxs(label)
    _, n, _ = LZ.FIELDS[label]
    cases = LZ.is_zero_cases(label)
    assert sum(1 for _, _, want in cases if want) >= 31 * 4
    limbs = [l for _, l, _ in cases]
    zero = [[0] * n] * len(cases)
    for live_rows in (15, 9):
        raw, canon = _run(curve, label, "rows", TFR_IS_ZERO, limbs, zero, live_rows)
        for (name, _, want), r, cv in zip(cases, raw, canon):
            assert r == [1 if want else 0] + [0] * (n - 1) and cv == 0, name

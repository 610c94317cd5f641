"""The GLV split at its rounding thresholds and longest halves, on the device.  The scalars of oracle/glv_edges.py --
both sides of the rounding thresholds of x_0 and x_1 (with the carry rippling through one, two and three words), the
halves +-2^32 .. +-2^96 at which the sign conversion borrows, the named corners of the older tests and the 64 scalars
whose halves come closest to the supremum -- go through every place glv_decompose is compiled into: k_test_glv, the digit
slicer of k_hist / k_coarse / k_digits (msmz_test_digits, msmz_test_sort_ex and whole MSMs), k_points_mul_glv and the
host's split of a broadcast scalar.  The expected halves come from the integer model, never from the device
(tests/test_glv_edges_cpu.py pins the model and the supremum without a GPU)."""
import ctypes as C

import numpy as np
import pytest

import test_sort_gpu as TS
from oracle import bigint_ref as B
from oracle import c_oracle
from oracle import glv_edges as E
from oracle import params as P
from oracle import prng
from oracle import sort_ref as S

pytestmark = pytest.mark.gpu

PSEED = 4201
BLOCK = 1 << 16   # a multi-engine context deals a set out in blocks of this many entries (csrc/multi.h)


@pytest.fixture(scope="module")
def mod():
    import msm_zprize_amd as m
    m.startThreads()
    return m


@pytest.fixture(scope="module")
def curves(mod):
    cache = {}

    def get(label):
        if label not in cache:
            cache[label] = mod.Weierstrass.create(mod.curves.BY_LABEL[label])
        return cache[label]

    yield get
    for c in cache.values():
        c.close()


def _lib():
    from msm_zprize_amd._native import lib
    return lib()


class Edges:
    """the edge set of one curve and the model's halves, computed once"""

    def __init__(self, label):
        self.named = E.edge_scalars(label)
        self.scalars = E.edge_set(label)
        self.n = len(self.scalars)
        self.halves = [E.model(label, s) for s in self.scalars]
        self.raw = b"".join(s.to_bytes(32, "little") for s in self.scalars)
        self.words = S.to_words(self.scalars, 8)
        # magnitudes as words and sign bytes, half after half
        self.mag = [S.to_words([abs(h[j]) for h in self.halves], 4) for j in range(2)]
        self.neg = [np.array([h[j] < 0 for h in self.halves], dtype=np.uint8) for j in range(2)]


_edges = {}


def edges(label):
    if label not in _edges:
        _edges[label] = Edges(label)
    return _edges[label]


def _strip(p):
    """a result or a downloaded record; infinity in one form, whatever coordinates it came with"""
    if p.get("isZero"):
        return {"x": 0, "y": 0, "isZero": True}
    return {"x": p["x"], "y": p["y"], "isZero": False}


def _multiple(label, t):
    """[t]G as the downloads give it"""
    c = P.CURVES[label]
    if t == 0:
        return _strip({"isZero": True})
    return _strip(c_oracle.scale(c, t, {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}))


def _rows(label, scalars, mult):
    """[s_i a_i mod q]G, row by row"""
    q = P.CURVES[label]["order"]
    return [_multiple(label, s * int(a) % q) for s, a in zip(scalars, mult)]


def _download(curve, arr, first=0, count=None):
    return [_strip(p) for p in curve.Affine.toBigints(arr, first, count)]


# ---------------------------------------------------------------------------------------------- k_test_glv
@pytest.mark.parametrize("label", E.LABELS)
def test_device_split_equals_model(curves, label):
    """k_test_glv == the model: 16-byte magnitudes and both sign bytes of every edge scalar"""
    curve, e = curves(label), edges(label)
    n = e.n
    s0b, s1b, neg = C.create_string_buffer(16 * n), C.create_string_buffer(16 * n), C.create_string_buffer(2 * n)
    assert _lib().msmz_test_glv(curve._ctx, e.raw, n, s0b, s1b, neg) == 0
    for i, (s, (s0, s1)) in enumerate(zip(e.scalars, e.halves)):
        got = (int.from_bytes(s0b.raw[16 * i:16 * i + 16], "little"), neg.raw[2 * i],
               int.from_bytes(s1b.raw[16 * i:16 * i + 16], "little"), neg.raw[2 * i + 1])
        assert got == (abs(s0), int(s0 < 0), abs(s1), int(s1 < 0)), hex(s)


# ---------------------------------------------------------------------------------------------- the digit slicer
@pytest.mark.parametrize("label", E.LABELS)
def test_digits_of_model_halves(curves, label):
    """msmz_test_digits with glv = 1: every digit of every edge scalar == signed_digits of the MODEL's halves, the half's
    sign folded in"""
    curve, e = curves(label), edges(label)
    n = e.n
    for c in (2, 7, 13, 16, 17, 21):
        K = -(-(128 + 1) // c)
        digits = np.zeros(2 * n * K, dtype=np.uint32)
        assert _lib().msmz_test_digits(curve._ctx, e.raw, n, c, K, 1, digits.ctypes.data_as(C.c_void_p)) == 0
        want = np.zeros((2, n, K), dtype=np.uint32)
        for i, hs in enumerate(e.halves):
            for h, sv in enumerate(hs):
                sd = B.signed_digits(abs(sv), c, K)
                assert sum((-l if ng else l) << (c * k) for k, (l, ng) in enumerate(sd)) == abs(sv)
                want[h, i] = [l | ((ng ^ int(sv < 0)) << 31 if l else 0) for l, ng in sd]
        bad = np.argwhere(digits.reshape(2, n, K) != want)
        assert bad.size == 0, (label, c, "half, scalar, window", bad[0].tolist(), hex(e.scalars[int(bad[0][1])]))


# ---------------------------------------------------------------------------------------------- the sort
@pytest.mark.parametrize("label", E.LABELS)
def test_sort_of_model_halves(curves, label):
    """msmz_test_sort_ex with glv = 1 and the fold allowed: no error, and entry count, largest bucket, every offset and
    the contents of every bucket -- those of the top window, spread or folded, named apart -- are what the model's halves
    give; the longest halves put an entry into the top window"""
    curve, e = curves(label), edges(label)
    n = e.n
    words = e.words.reshape(1, n, 8)
    for c in (0, 9, 13, 16, 17):
        cs = TS.case(f"edges-c{c}", label, n, c, [], glv=1, fold=1)
        st, g, meta, off, refs, bins, packed = TS.sort_ex(curve, words, cs)
        assert st == 0, (c, st)
        pr = S.problem_entries([(e.mag[0], e.neg[0]), (e.mag[1], e.neg[1])], np.zeros(n, dtype=bool), g, n, detail=True)
        m = S.sort_model([pr], g)
        err, n_entries, max_bucket = (int(x) for x in meta)
        print(f"{label} c={c}: geometry {g} entries {n_entries} largest {m['largest']}")
        assert m["error"] == 0 and err == 0, (c, err, m["error"])
        assert n_entries == m["n_entries"], c
        assert max_bucket == S.expected_max_bucket(m["largest"], g["two_level"]), c
        o64 = off.astype(np.int64)
        assert (o64 == m["off"]).all(), (c, int(np.nonzero(o64 != m["off"])[0][0]))
        got = S.keyed_ranges(o64, refs)
        # the top window's buckets: sets K - 1 and up (its sub-windows when it is spread; one set when it is folded)
        first_top = (g["K"] - 1) * g["L"]
        top = pr["window"] == g["K"] - 1
        assert (pr["bucket"][top] >= first_top).all() and (pr["bucket"][~top] < first_top).all()
        want_top = S.keyed(pr["bucket"][top], pr["ref"][top])
        d = S.first_difference(got[(got >> np.uint64(32)) >= np.uint64(first_top)], want_top)
        assert d is None, (c, "top window: bucket, got, model", d)
        d = S.first_difference(got, m["by_bucket"])
        assert d is None, (c, "bucket, got, model", d)
        # the top window holds digits up to that of the supremum (and a carry), the `longest` halves come within 1 % of
        # it, and it fits a folded window
        top_digit = int(max(dg[0][:, g["K"] - 1].max() for dg in pr["digits"]))
        shift = g["c"] * (g["K"] - 1)
        sup = E.supremum(label)
        assert (int(min(sup) * 99 / 100) >> shift) <= top_digit <= (int(max(sup)) >> shift) + 1, (g["c"], top_digit)
        assert bool(top.any()) == (top_digit > 0)
        if g["fold_shift"]:
            assert top_digit <= 1 << g["fold_shift"]


# ---------------------------------------------------------------------------------------------- whole MSMs
@pytest.mark.parametrize("label", E.LABELS)
def test_msm_over_the_edge_scalars(curves, label):
    """msmUnsafe and msm with GLV over exactly the edge scalars == (sum s_i a_i mod q) G; no MSM is redone"""
    curve, e = curves(label), edges(label)
    n, q = e.n, P.CURVES[label]["order"]
    pts = curve.Parallel.randomPointsFast(n, PSEED)
    sc = curve.Parallel.scalarsFromBigints(e.scalars)
    a = prng.multipliers_np(PSEED, n)
    want = _multiple(label, sum(s * int(m) for s, m in zip(e.scalars, a)) % q)
    before = _lib().msmz_test_retries(curve._ctx)
    for c in (0, 9, 13, 16, 17):
        assert _strip(curve.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 1, "c": c})["result"]) == want, ("unsafe", c)
        assert _strip(curve.Parallel.msm(sc, pts, n, False, {"glv": 1, "c": c})["result"]) == want, ("safe", c)
    assert _lib().msmz_test_retries(curve._ctx) == before   # a real scalar never overflows the windows
    pts.free(); sc.free()


# ---------------------------------------------------------------------------------------------- k_points_mul_glv
@pytest.mark.parametrize("label", E.LABELS)
def test_per_point_glv_chain(curves, label):
    """mulPoints(..., subgroup=True) with the edge scalars as a resident set: row i == [s_i a_i mod q]G"""
    curve, e = curves(label), edges(label)
    n = e.n
    if label == "bls12-377":   # 126 steps there: bit 125 of a half is the first step of the chain
        assert any(abs(h) >> 125 for s in e.named["longest"] for h in E.model(label, s))
    pts = curve.Parallel.randomPointsFast(n, PSEED)
    sc = curve.Parallel.scalarsFromBigints(e.scalars)
    out = curve.Parallel.mulPoints(sc, pts, subgroup=True)
    got = _download(curve, out)
    want = _rows(label, e.scalars, prng.multipliers_np(PSEED, n))
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, (len(bad), [hex(e.scalars[i]) for i in bad[:3]])
    for arr in (pts, sc, out):
        arr.free()


@pytest.mark.parametrize("label", E.LABELS)
def test_broadcast_scalar_is_split_on_the_host(curves, label):
    """mulPoints with ONE scalar for 64 points (the host's glv_decompose): 8 longest, 8 ripple thresholds, 8 small"""
    curve, e = curves(label), edges(label)
    n = 64
    small = [s for a, b, s in E.small_pairs(label) if abs(a) in (1 << 32, 1 << 64, 1 << 96) and abs(b) in (1 << 32, (1 << 64) - 1)]
    us = e.named["longest"][:8] + e.named["ripple"][:8] + small[:8]
    assert len(set(us)) == 24
    pts = curve.Parallel.randomPointsFast(n, PSEED + 1)
    a = prng.multipliers_np(PSEED + 1, n)
    for u in us:
        out = curve.Parallel.mulPoints(u, pts, subgroup=True)
        assert _download(curve, out) == _rows(label, [u] * n, a), hex(u)
        out.free()
    pts.free()


# ---------------------------------------------------------------------------------------------- two engines
def test_two_engine_context(mod):
    """devices = [0, 0]: a block of random scalars for the first engine, the edge scalars in the second engine's block;
    the MSM and the per-point rows equal the closed forms"""
    label = "bls12-377"
    e, q = edges(label), P.CURVES[label]["order"]
    n = BLOCK + e.n
    head = prng.scalars_np(PSEED + 2, BLOCK, q)
    a = prng.multipliers_np(PSEED + 3, n)
    t = (prng.sum_of_products_mod(head, a[:BLOCK], q) + sum(s * int(m) for s, m in zip(e.scalars, a[BLOCK:]))) % q
    mod.startThreads(devices=[0, 0])
    multi = mod.Weierstrass.create(mod.curves.BY_LABEL[label])
    mod.startThreads()
    try:
        pts = multi.Parallel.randomPointsFast(n, PSEED + 3)
        sc = multi.Parallel.scalarsFromBytes(head.astype("<u8").tobytes() + e.raw, n)
        before = _lib().msmz_test_retries(multi._ctx)
        assert _strip(multi.Parallel.msm(sc, pts, n, False, {"glv": 1})["result"]) == _multiple(label, t)
        assert _strip(multi.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 1, "c": 13})["result"]) == _multiple(label, t)
        assert _lib().msmz_test_retries(multi._ctx) == before
        out = multi.Parallel.mulPoints(sc, pts, subgroup=True)
        assert _download(multi, out, BLOCK, e.n) == _rows(label, e.scalars, a[BLOCK:])
    finally:
        multi.close()

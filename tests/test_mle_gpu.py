"""Multilinear polynomials over resident scalar sets on the GPU (k_scalars_eq_table / _mle_eval / _mle_bind /
_sumcheck_round, csrc/mle_kernels.h) through the C ABI and the Python methods, bit-exact against Python integers mod the
group order (tests/mle_util.py) and against the older calls they must agree with (innerProduct, combineScalars).  Sizes
come from msmz_test_mle_geometry: fewer than one run, one run, two, a partial wave, a block, one tile and its
neighbours, and once a size whose tile count makes the second level loop.  Then a whole sumcheck protocol that moves
nothing but 32-byte values to the host, the errors, and a multi-engine context."""
import ctypes as C
import random

import pytest

import mle_util as M
import scalar_ops_util as S
from mle_util import mask_sets

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
MAX_TABLES, MAX_DEGREE, MAX_TERMS = 6, 4, 8
BIG_LABEL = "bls12-377"   # the one curve that runs the sizes whose second level loops


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
            params = mod.curves.BY_LABEL[label]
            cache[label] = (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)
        return cache[label]

    yield get
    for c in cache.values():
        c.close()


def _lib():
    from msm_zprize_amd._native import lib
    return lib()


def _geometry():
    """(RUN, log2 TILE_E, log2 TILE_P, partial sums the second level takes per pass)"""
    r, e, p, t, pp = (C.c_uint32(0) for _ in range(5))
    _lib().msmz_test_mle_geometry(C.byref(r), C.byref(e), C.byref(p))
    _lib().msmz_test_scalar_dot_geometry(C.byref(t), C.byref(pp))
    assert e.value & (e.value - 1) == 0 and p.value & (p.value - 1) == 0
    return r.value, e.value.bit_length() - 1, p.value.bit_length() - 1, pp.value


def _eval_vars():
    """fewer than one run (0, 1, 2), one run, two runs, a partial wave (2^5 entries: 4 threads), 2^6, a block's worth of
    runs and the tile edges of mle_eval"""
    run, le, _, _ = _geometry()
    lr = run.bit_length() - 1
    return sorted({0, 1, 2, lr, lr + 1, 5, 6, 8, le - 1, le, le + 1})


def _round_vars():
    """the tile edges of sumcheck_round: 2^(v-1) pair indices are half a tile, one tile, two tiles"""
    _, _, lp, _ = _geometry()
    return [lp, lp + 1, lp + 2]


def _big_vars():
    """the smallest sizes whose tile counts exceed one pass of the second level: (mle_eval, sumcheck_round)"""
    _, le, lp, pp = _geometry()
    return le + pp.bit_length(), lp + 1 + pp.bit_length()


def _point(q, v, rng):
    """r_j over {0, 1, q - 1, random, ...}: the constants in the low, register-expanded variables and in high ones"""
    return [(rng.randrange(2, q), 0, q - 1, 1, rng.randrange(2, q))[(j + v) % 5] for j in range(v)]


def _random_point(q, v, rng):
    return [rng.randrange(2, q) for _ in range(v)]


def _upload(curve, vals):
    return curve.Parallel.scalarsFromBytes(S.encode(vals), len(vals))


def _le(v):
    return int(v).to_bytes(32, "little")


def _plant(curve, arr, index, value):
    """make `value` (>= q) entry `index` of a resident set: msmz_import_scalars_into converts before it reports, so after
    its MSMZ_ERR_RANGE the refused value is what the handle holds (as tests/test_scalar_ops_gpu.py does)"""
    from msm_zprize_amd._native import MsmzSrc
    raw = S.encode([value])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, arr.handle, index, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert curve.Scalar.toBigints(arr, index, 1) == [value]


# -- the C ABI, status and outputs as they are ------------------------------------------------------------------
def _c_eq(curve, point, scale=None, h0=0, n_vars=None):
    h = C.c_uint64(h0)
    raw = b"".join(_le(r) for r in point) if point is not None else None
    st = _lib().msmz_scalars_eq_table(curve._ctx, raw, len(point) if n_vars is None else n_vars,
                                      None if scale is None else _le(scale), C.byref(h))
    return st, h.value


def _c_eval(curve, f, first, point, n_vars=None):
    buf = C.create_string_buffer(b"\xaa" * 32, 32)
    raw = b"".join(_le(r) for r in point) if point is not None else None
    fh = f if isinstance(f, int) else f.handle
    st = _lib().msmz_scalars_mle_eval(curve._ctx, fh, first, len(point) if n_vars is None else n_vars, raw, buf)
    return st, buf.raw


def _c_bind(curve, f, first, n_vars, r, count=1, flags=0, first_out=0, out=0):
    from msm_zprize_amd._native import MsmzMleBind
    fh = f if isinstance(f, int) else f.handle
    b = MsmzMleBind(fh, first, n_vars, count, flags, None if r is None else _le(r))
    h = C.c_uint64(out if isinstance(out, int) else out.handle)
    st = _lib().msmz_scalars_mle_bind(curve._ctx, C.byref(b), first_out, C.byref(h))
    return st, h.value


def _c_round(curve, tables, n_vars, terms, flags=0):
    """tables: [(array or raw handle, first)], terms: [(coeff or None, mask)] -> (status, *degree, the 160 bytes)"""
    from msm_zprize_amd import _native as N
    tabs = (N.MsmzSumcheckTable * max(1, len(tables)))(
        *[N.MsmzSumcheckTable(a if isinstance(a, int) else a.handle, f) for a, f in tables])
    trms = (N.MsmzSumcheckTerm * max(1, len(terms)))(*[N.MsmzSumcheckTerm(None if c is None else _le(c), m) for c, m in terms])
    s = N.MsmzSumcheck(tabs, len(tables), n_vars, trms, len(terms), flags)
    d = C.c_uint32(99)
    ev = C.create_string_buffer(b"\xaa" * 160, 160)
    st = _lib().msmz_scalars_sumcheck_round(curve._ctx, C.byref(s), C.byref(d), ev)
    return st, d.value, ev.raw


_tables = {}


def _table(label, v, k=0):
    """table k of 2^v values of a curve, made once: the planted rows of the scalar-set tests (0, 1, q - 1, the value with
    seven full low words, pairs summing to q) in its first 64 entries and at its end"""
    if (label, v, k) not in _tables:
        _tables[(label, v, k)] = S.build_vectors(label, 1 << v, 9000 + 100 * v + k)[k % 2]
    return _tables[(label, v, k)]


# ---------------------------------------------------------------------------------------------- eq tables
@pytest.mark.parametrize("label", S.ALL)
def test_eq_table(curves, label):
    """the download == the Python model at every small size for scale over {NULL, 0, q - 1, random}, and the sum of the
    table (innerProduct without a second operand) == scale"""
    from msm_zprize_amd.parallel import DeviceArray
    curve, q = curves(label), S.order(label)
    rng = random.Random(S.ALL.index(label) + 1)
    for v in _eval_vars():
        for scale in (None, 0, q - 1, rng.randrange(2, q)):
            point = _point(q, v, rng) if scale is None else _random_point(q, v, rng)
            st, h = _c_eq(curve, point, scale)
            assert st == 0 and h != 0, (v, scale)
            arr = DeviceArray(curve, h, 1 << v, "scalars")
            want = M.eq(point, q, 1 if scale is None else scale)
            got = curve.Scalar.toBigints(arr)
            bad = [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
            assert not bad, (v, scale, bad[:3])
            assert curve.Parallel.innerProduct(arr) == (1 if scale is None else scale), v
            arr.free()
    arr = curve.Parallel.eqTable([0, 1, 1], 5)      # a 0/1 point: the indicator of index 0b110
    assert curve.Scalar.toBigints(arr) == [0, 0, 0, 0, 0, 0, 5, 0]
    arr.free()
    arr = curve.Parallel.eqTable([], 9)
    assert curve.Scalar.toBigints(arr) == [9]
    arr.free()


def test_eq_table_largest(curves):
    """at the size whose tile count makes the second level of the sum loop: sum eq == scale, no host model needed"""
    curve, q = curves(BIG_LABEL), S.order(BIG_LABEL)
    v, _ = _big_vars()
    rng = random.Random(77)
    scale = rng.randrange(2, q)
    arr = curve.Parallel.eqTable(_random_point(q, v, rng), scale)
    assert len(arr) == 1 << v and curve.Parallel.innerProduct(arr) == scale
    arr.free()


# ---------------------------------------------------------------------------------------------- evaluation
@pytest.mark.parametrize("label", S.ALL)
def test_evaluate_mle(curves, label):
    """f(r) == the Python model == innerProduct(f, eqTable(r)) at every small size; == the one entry left after v
    successive bindMle calls, the high variable first (r read backwards) and variable 0 first (r in order)"""
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    rng = random.Random(S.ALL.index(label) + 11)
    for v in _eval_vars():
        vals = _table(label, v)
        f = _upload(curve, vals)
        for point in (_point(q, v, rng), _random_point(q, v, rng)):
            want = M.mle_eval(vals, point, q)
            got = par.evaluateMle(f, point)
            assert got == want, (v, hex(got), hex(want))
            e = par.eqTable(point)
            assert par.innerProduct(f, e) == got, v
            e.free()
            assert _c_eval(curve, f, 0, point) == (0, _le(want))
        if 1 <= v <= 8:
            point = _point(q, v, rng)
            want = par.evaluateMle(f, point)
            hi = f
            for r in reversed(point):
                nxt = par.bindMle(hi, r)
                if hi is not f:
                    hi.free()
                hi = nxt
            lo = f
            for r in point:
                nxt = par.bindMle(lo, r, low=True)
                if lo is not f:
                    lo.free()
                lo = nxt
            assert len(hi) == len(lo) == 1
            assert curve.Scalar.toBigints(hi) == curve.Scalar.toBigints(lo) == [want], v
            hi.free(); lo.free()
        f.free()


@pytest.mark.parametrize("label", S.ALL)
def test_evaluate_mle_sub_range(curves, label):
    """first != 0: tables inside a longer set, starting off every alignment the kernel has"""
    curve, q = curves(label), S.order(label)
    rng = random.Random(S.ALL.index(label) + 21)
    total = 3000
    vals, _ = S.build_vectors(label, total, 5)
    f = _upload(curve, vals)
    for v, first in ((0, total - 1), (2, 1), (3, 5), (5, 61), (8, 7), (11, 3), (11, total - 2048)):
        point = _point(q, v, rng)
        assert curve.Parallel.evaluateMle(f, point, first) == M.mle_eval(vals[first:first + (1 << v)], point, q), (v, first)
    f.free()


def test_evaluate_mle_largest(curves):
    """the size whose tile count makes the second level loop: == innerProduct(f, eqTable(r)) byte for byte"""
    curve, q = curves(BIG_LABEL), S.order(BIG_LABEL)
    v, _ = _big_vars()
    rng = random.Random(78)
    point = _random_point(q, v, rng)
    f = curve.Parallel.randomScalars(1 << v, 5)
    e = curve.Parallel.eqTable(point)
    got = curve.Parallel.evaluateMle(f, point)
    assert got == curve.Parallel.innerProduct(f, e) and got != 0
    assert curve.Parallel.evaluateMle(f, point) == got
    f.free(); e.free()


# ---------------------------------------------------------------------------------------------- binding
@pytest.mark.parametrize("label", S.ALL)
def test_bind_new_handle_and_ranges(curves, label):
    """both orders, count over {1, 3}, r over {0, 1, q - 1, random}: into a new handle, and into a range of an existing
    set apart from the source with every entry around it untouched"""
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    rng = random.Random(S.ALL.index(label) + 31)
    for v in (1, 2, 5, 9):
        n, h = 1 << v, 1 << (v - 1)
        for count in (1, 3):
            first = 3
            vals, _ = S.build_vectors(label, first + count * n + 2, 40 + v + count)
            f = _upload(curve, vals)
            for low in (False, True):
                for r in (0, 1, q - 1, rng.randrange(2, q)):
                    want = []
                    for k in range(count):
                        want += M.bind(vals[first + k * n:first + (k + 1) * n], r, q, low)
                    out = par.bindMle(f, r, v, count, low, first)
                    assert len(out) == count * h and curve.Scalar.toBigints(out) == want, (v, count, low, r)
                    out.free()
                # into an existing set, apart from the source
                dst_vals, _ = S.build_vectors(label, count * h + 11, 50 + v)
                dst = _upload(curve, dst_vals)
                assert par.bindMle(f, r, v, count, low, first, out=dst, firstOut=6) is dst
                assert curve.Scalar.toBigints(dst) == dst_vals[:6] + want + dst_vals[6 + count * h:], (v, count, low)
                dst.free()
            f.free()


@pytest.mark.parametrize("label", S.ALL)
def test_bind_in_place_and_against_combine(curves, label):
    """the high bind in place: the low half is overwritten, the high half and everything else untouched; the high bind ==
    combineScalars(1 - r, f, r, f, firstY = h) byte for byte; a disjoint range of the SAME handle as destination"""
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    rng = random.Random(S.ALL.index(label) + 41)
    for v in (1, 3, 6, 10):
        n, h = 1 << v, 1 << (v - 1)
        first = 5
        vals, _ = S.build_vectors(label, first + n + h + 9, 60 + v)
        r = rng.randrange(2, q)
        want = M.bind(vals[first:first + n], r, q)
        f = _upload(curve, vals)
        ref = par.combineScalars((1 - r) % q, f, r, f, h, first, first + h)
        new = par.bindMle(f, r, v, first=first)
        assert curve.Scalar.toBigints(new) == curve.Scalar.toBigints(ref) == want, v
        ref.free(); new.free()
        assert par.bindMle(f, r, v, first=first, out=f, firstOut=first + n + 2) is f          # apart, in the same handle
        vals[first + n + 2:first + n + 2 + h] = want
        assert curve.Scalar.toBigints(f) == vals, v
        assert par.bindMle(f, r, v, first=first, out=f, firstOut=first) is f                  # in place
        vals[first:first + h] = want
        assert curve.Scalar.toBigints(f) == vals, v
        f.free()


@pytest.mark.parametrize("label", S.ALL)
def test_bind_forbidden_overlaps(curves, label):
    """every overlap but the one allowed is MSMZ_ERR_ARG and leaves the set byte-identical"""
    curve, q = curves(label), S.order(label)
    v, first = 4, 16
    n, h = 1 << v, 1 << (v - 1)
    vals, _ = S.build_vectors(label, 100, 70)
    f = _upload(curve, vals)
    LOW = 1
    cases = [(1, 0, first + h),                                   # exactly the high half
             (1, 0, first + 1), (1, 0, first - 1), (1, 0, first - h + 1), (1, 0, first + h - 1), (1, 0, first + h + 1),
             (1, 0, first + n - 1),                               # partial overlaps with either half
             (1, LOW, first), (1, LOW, first + h), (1, LOW, first + 3), (1, LOW, first - h + 1),   # low binding, any overlap
             (2, 0, first), (2, 0, first + h), (2, 0, first + n), (2, 0, first + 2 * n - 1), (2, LOW, first),
             (2, 0, first - 2 * h + 1)]                           # several tables, any overlap
    for count, flags, first_out in cases:
        assert _c_bind(curve, f, first, v, 5, count, flags, first_out, f) == (MSMZ_ERR_ARG, f.handle), (count, flags, first_out)
    assert curve.Scalar.toBigints(f) == vals
    # the neighbours of the forbidden ranges are allowed: the destination ends where the source begins, or begins where it ends
    for count, flags, first_out in ((1, 0, first - h), (1, 0, first + n), (1, LOW, first - h), (2, LOW, first + 2 * n),
                                    (2, 0, first - 2 * h)):
        assert _c_bind(curve, f, first, v, 5, count, flags, first_out, f) == (0, f.handle), (count, flags, first_out)
    f.free()


# ---------------------------------------------------------------------------------------------- round polynomials
def _check_round(curve, q, tables_host, tables_dev, v, terms, low):
    want = M.round_poly(tables_host, terms, q, low)
    st, d, raw = _c_round(curve, tables_dev, v, terms, 1 if low else 0)
    assert st == 0 and d == len(want) - 1, (st, d)
    assert S.decode(raw[:32 * (d + 1)]) == want, (v, terms, low)
    assert raw[32 * (d + 1):] == b"\xaa" * (160 - 32 * (d + 1))    # bytes past d + 1 values are as they were
    return want


@pytest.mark.parametrize("label", S.ALL)
def test_sumcheck_round_forms(curves, label):
    """== the Python model for every table count 1 .. max at v over {1, 2, 7}, the four mask sets of the CPU test with
    coefficients over {NULL, 0, q - 1, random}, both orders; *degree is the largest popcount"""
    curve, q = curves(label), S.order(label)
    rng = random.Random(S.ALL.index(label) + 51)
    for v in (1, 2, 7):
        host = [_table(label, v, k) for k in range(MAX_TABLES)]
        dev = [_upload(curve, t) for t in host]
        for nt in range(1, MAX_TABLES + 1):
            for masks in mask_sets(nt, MAX_DEGREE):
                coeffs = [(None, None), (0, q - 1), (q - 1, rng.randrange(2, q)), (rng.randrange(2, q), None)][(nt + len(masks) + v) % 4]
                terms = list(zip(coeffs, masks))
                for low in (False, True):
                    _check_round(curve, q, host[:nt], [(a, 0) for a in dev[:nt]], v, terms, low)
        for coeffs in ((None, None), (0, q - 1), (q - 1, rng.randrange(2, q)), (rng.randrange(2, q), None)):
            _check_round(curve, q, host[:4], [(a, 0) for a in dev[:4]], v, list(zip(coeffs, (0b0011, 0b0100))), v % 2 == 0)
        for a in dev:
            a.free()


@pytest.mark.parametrize("label", S.ALL)
def test_sumcheck_round_table_placement_and_tiles(curves, label):
    """tables in separate handles, as ranges of ONE handle (off every alignment), and the same table twice (a square), at
    the tile edges of the kernel; the Python method returns the same values"""
    curve, q = curves(label), S.order(label)
    rng = random.Random(S.ALL.index(label) + 61)
    for v in (3, 6) + tuple(_round_vars()):
        n = 1 << v
        a, b = _table(label, v, 0), _table(label, v, 1)
        one = [7] * 3 + a + [9] * 2 + b + [1]
        da, db, d1 = _upload(curve, a), _upload(curve, b), _upload(curve, one)
        c = rng.randrange(2, q)
        for low in (False, True):
            want = _check_round(curve, q, [a, b], [(da, 0), (db, 0)], v, [(c, 0b11), (None, 0b01)], low)
            assert _check_round(curve, q, [a, b], [(d1, 3), (d1, 5 + n)], v, [(c, 0b11), (None, 0b01)], low) == want
            sq = _check_round(curve, q, [a, a], [(da, 0), (da, 0)], v, [(None, 0b11)], low)
            assert (sq[0] + sq[1]) % q == sum(x * x for x in a) % q
            assert curve.Parallel.sumcheckRound([da, (d1, 5 + n)], [(c, 0b11), (None, 0b01)], v, low) == want
            assert curve.Parallel.sumcheckRound([da, db], [(c, 3), (1, 1)], low=low) == want       # nVars from the table
        for arr in (da, db, d1):
            arr.free()


def test_sumcheck_round_largest(curves):
    """a two-table product at the size whose tile count makes the second level loop: g(0) + g(1) == the claimed sum from
    innerProduct, both orders; two calls return the same bytes"""
    curve, q = curves(BIG_LABEL), S.order(BIG_LABEL)
    _, v = _big_vars()
    f, g = curve.Parallel.randomScalars(1 << v, 8), curve.Parallel.randomScalars(1 << v, 9)
    claim = curve.Parallel.innerProduct(f, g)
    for low in (False, True):
        evals = curve.Parallel.sumcheckRound([f, g], [(None, 0b11)], low=low)
        assert len(evals) == 3 and (evals[0] + evals[1]) % q == claim
        assert curve.Parallel.sumcheckRound([f, g], [(None, 0b11)], v, low) == evals
    f.free(); g.free()


# ---------------------------------------------------------------------------------------------- a whole protocol
@pytest.mark.parametrize("low", [False, True])
@pytest.mark.parametrize("label", ["bls12-381", "pallas"])
def test_sumcheck_protocol(curves, label, low):
    """v = 10, tables eq, A, B, C, terms {+1: eq A B, q - 1: eq C}: per round g_k(0) + g_k(1) == g_(k-1)(r_(k-1)) by
    Lagrange interpolation on the host, then all four tables bound to the challenge; at the end g_v(r_v) ==
    eq(r) (A(r) B(r) - C(r)) with the four values from evaluateMle on the ORIGINAL tables.  Only 32-byte values cross."""
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    v = 10
    rng = random.Random(1000 + S.ALL.index(label))
    tau = _random_point(q, v, rng)
    orig = [par.eqTable(tau)] + [par.randomScalars(1 << v, 90 + k) for k in range(3)]
    terms = [(1, 0b0111), (q - 1, 0b1001)]
    ab = par.combineScalars(orig[1], orig[2])                                  # the Hadamard product A . B
    claim = (par.innerProduct(ab, orig[0]) - par.innerProduct(orig[3], orig[0])) % q
    ab.free()
    tabs = list(orig)                                                          # (round 0 reads the originals)
    challenges = []
    for k in range(v):
        evals = par.sumcheckRound(tabs, terms, v - k, low)
        assert len(evals) == 4, k
        assert (evals[0] + evals[1]) % q == claim, k
        r = rng.randrange(q)
        challenges.append(r)
        claim = M.interpolate(evals, r, q)
        nxt = [par.bindMle(t, r, v - k, low=low) for t in tabs]
        for t in tabs:
            if not any(t is o for o in orig):
                t.free()
        tabs = nxt
    assert all(len(t) == 1 for t in tabs)
    # the variables were bound high first (variable v-1, v-2, ..) or low first (variable 0, 1, ..)
    point = challenges if low else challenges[::-1]
    e, a, b, c = (par.evaluateMle(t, point) for t in orig)
    assert claim == e * (a * b - c) % q
    assert e == M.mle_eval(M.eq(tau, q), point, q)                             # eq(tau, r) from the model
    for t in tabs + orig:
        t.free()


# ---------------------------------------------------------------------------------------------- errors
def _good_calls_are_correct(curve, q):
    vals = [5, q - 1, 77, 0, 9, 1, 2, 3]
    f = _upload(curve, vals)
    assert curve.Parallel.evaluateMle(f, [3, 4, 5]) == M.mle_eval(vals, [3, 4, 5], q)
    out = curve.Parallel.bindMle(f, 6, low=True)
    assert curve.Scalar.toBigints(out) == M.bind(vals, 6, q, True)
    assert curve.Parallel.sumcheckRound([f, out], [(2, 3)], 2) == M.round_poly([vals[:4], M.bind(vals, 6, q, True)], [(2, 3)], q)
    f.free(); out.free()


@pytest.mark.parametrize("label", S.ALL)
def test_resident_entry_out_of_range(curves, label):
    """ONE record >= q at the first, a middle and the last index of the range: mle_eval, mle_bind (both orders, new handle
    and in place) and sumcheck_round (both orders, as either table) return MSMZ_ERR_RANGE, no handle appears, *out_handle,
    *degree and the output bytes are as they were, the next calls are correct; the same record OUTSIDE the range is not
    read"""
    curve, q = curves(label), S.order(label)
    v, first = 8, 4
    n = 1 << v
    rng = random.Random(12)
    vals = [rng.randrange(q) for _ in range(first + n + 4)]
    point = _random_point(q, v, rng)
    good = _upload(curve, vals)
    for index, bad_value in ((first, q), (first + 150, (1 << 256) - 1), (first + n - 1, q + 1)):
        bad = _upload(curve, vals)
        _plant(curve, bad, index, bad_value)
        assert _c_eval(curve, bad, first, point) == (MSMZ_ERR_RANGE, b"\xaa" * 32), index
        for flags in (0, 1):
            assert _c_bind(curve, bad, first, v, 5, 1, flags) == (MSMZ_ERR_RANGE, 0), index
            assert _c_bind(curve, bad, first, v - 1, 5, 2, flags) == (MSMZ_ERR_RANGE, 0), index
            for tables in ([(bad, first)], [(good, first), (bad, first)], [(bad, first), (good, 0)]):
                terms = [(None, (1 << len(tables)) - 1)]
                assert _c_round(curve, tables, v, terms, flags) == (MSMZ_ERR_RANGE, 99, b"\xaa" * 160), index
        scratch = _upload(curve, vals)
        _plant(curve, scratch, index, bad_value)
        assert _c_bind(curve, scratch, first, v, 5, 1, 0, first, scratch) == (MSMZ_ERR_RANGE, scratch.handle)   # in place
        scratch.free()
        _good_calls_are_correct(curve, q)
        # ranges clear of the bad record
        lo, vv = (index + 1, 6) if index < first + n - 1 else (first, 7)
        if index == first + 150:
            lo, vv = first, 7                      # [first, first + 128) ends before it
        sub = vals[lo:lo + (1 << vv)]
        assert not lo <= index < lo + (1 << vv)
        assert curve.Parallel.evaluateMle(bad, point[:vv], lo) == M.mle_eval(sub, point[:vv], q)
        out = curve.Parallel.bindMle(bad, 5, vv, first=lo)
        assert curve.Scalar.toBigints(out) == M.bind(sub, 5, q)
        out.free()
        assert curve.Parallel.sumcheckRound([(bad, lo), (good, lo)], [(None, 3)], vv, True) == M.round_poly([sub, sub], [(None, 3)], q, True)
        bad.free()
    good.free()


@pytest.mark.parametrize("label", S.ALL)
def test_argument_errors(curves, label):
    """MSMZ_ERR_ARG before any launch with the outputs untouched; host values >= q are MSMZ_ERR_RANGE with nothing launched"""
    curve, q = curves(label), S.order(label)
    n = 64
    sc = curve.Parallel.randomScalars(n, 2)
    pts = curve.Parallel.randomPointsFast(n, 2)
    before = curve.Scalar.toBigints(sc)
    lib = _lib()
    from msm_zprize_amd import _native as N
    big = (1 << 64) - 1
    p2 = [3, 4]
    # eq_table
    assert lib.msmz_scalars_eq_table(curve._ctx, _le(1), 1, None, None) == MSMZ_ERR_ARG
    assert _c_eq(curve, None, None, 0, 2) == (MSMZ_ERR_ARG, 0)                      # a null point with variables
    assert _c_eq(curve, [1] * 32) == (MSMZ_ERR_ARG, 0)                              # v > 31
    assert _c_eq(curve, [1] * 31 + [0], None, 0, 1 << 31) == (MSMZ_ERR_ARG, 0)
    # mle_eval
    assert lib.msmz_scalars_mle_eval(curve._ctx, sc.handle, 0, 2, _le(1) * 2, None) == MSMZ_ERR_ARG
    untouched = b"\xaa" * 32
    for f, first, point, nv in ((sc, 0, None, 2), (sc, 0, [1] * 32, None), (0xDEAD, 0, p2, None), (pts.handle, 0, p2, None),
                                (sc, n - 3, p2, None), (sc, n, [], None), (sc, big, p2, None), (sc, 0, [1] * 7, None)):
        assert _c_eval(curve, f, first, point, nv) == (MSMZ_ERR_ARG, untouched), (first, nv)
    # mle_bind
    b = N.MsmzMleBind(sc.handle, 0, 2, 1, 0, _le(5))
    h = C.c_uint64(0)
    assert lib.msmz_scalars_mle_bind(curve._ctx, None, 0, C.byref(h)) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_mle_bind(curve._ctx, C.byref(b), 0, None) == MSMZ_ERR_ARG
    for f, first, nv, r, count, flags, first_out, out in (
            (sc, 0, 2, None, 1, 0, 0, 0),                                             # a null challenge
            (sc, 0, 0, 5, 1, 0, 0, 0), (sc, 0, 32, 5, 1, 0, 0, 0),                    # n_vars 0, > 31
            (sc, 0, 2, 5, 0, 0, 0, 0), (sc, 0, 31, 5, 2, 0, 0, 0), (sc, 0, 1, 5, 1 << 31, 0, 0, 0),   # counts
            (sc, 0, 2, 5, 1, 2, 0, 0), (sc, 0, 2, 5, 1, 1 << 31, 0, 0),               # unknown flag bits
            (0xDEAD, 0, 2, 5, 1, 0, 0, 0), (pts.handle, 0, 2, 5, 1, 0, 0, 0),         # handles
            (sc, 0, 2, 5, 1, 0, 0, 0xDEAD), (sc, 0, 2, 5, 1, 0, 0, pts.handle),
            (sc, n - 3, 2, 5, 1, 0, 0, 0), (sc, big, 2, 5, 1, 0, 0, 0), (sc, 0, 7, 5, 1, 0, 0, 0), (sc, 0, 5, 5, 3, 0, 0, 0),   # ranges
            (sc, 0, 2, 5, 1, 0, n - 1, sc.handle), (sc, 0, 2, 5, 1, 0, big, sc.handle),
            (sc, 0, 2, 5, 1, 0, 1, 0)):                                               # first_out without a handle
        assert _c_bind(curve, f, first, nv, r, count, flags, first_out, out) == (MSMZ_ERR_ARG, out), (first, nv, count, flags)
    # sumcheck_round
    tabs = (N.MsmzSumcheckTable * 1)(N.MsmzSumcheckTable(sc.handle, 0))
    trms = (N.MsmzSumcheckTerm * 1)(N.MsmzSumcheckTerm(None, 1))
    d = C.c_uint32(0)
    ev = C.create_string_buffer(160)
    ok = N.MsmzSumcheck(tabs, 1, 2, trms, 1, 0)
    assert lib.msmz_scalars_sumcheck_round(curve._ctx, C.byref(ok), C.byref(d), ev) == 0
    assert lib.msmz_scalars_sumcheck_round(curve._ctx, None, C.byref(d), ev) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_sumcheck_round(curve._ctx, C.byref(ok), None, ev) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_sumcheck_round(curve._ctx, C.byref(ok), C.byref(d), None) == MSMZ_ERR_ARG
    for s in (N.MsmzSumcheck(None, 1, 2, trms, 1, 0), N.MsmzSumcheck(tabs, 1, 2, None, 1, 0)):
        assert lib.msmz_scalars_sumcheck_round(curve._ctx, C.byref(s), C.byref(d), ev) == MSMZ_ERR_ARG
    t1 = [(sc, 0)]
    for tables, nv, terms, flags in (
            ([], 2, [(None, 1)], 0), (t1 * 7, 2, [(None, 1)], 0),                    # table counts
            (t1, 2, [], 0), (t1, 2, [(None, 1)] * 9, 0),                             # term counts
            (t1, 0, [(None, 1)], 0), (t1, 32, [(None, 1)], 0),                       # n_vars
            (t1, 2, [(None, 1)], 2), (t1, 2, [(None, 1)], 1 << 31),                  # unknown flag bits
            (t1, 2, [(None, 0)], 0), (t1, 2, [(None, 2)], 0), (t1 * 2, 2, [(None, 3), (None, 4)], 0),   # masks
            (t1 * 5, 2, [(None, 0b11111)], 0), (t1 * 6, 2, [(None, 0b111110)], 0),   # more than four factors
            ([(0xDEAD, 0)], 2, [(None, 1)], 0), ([(pts.handle, 0)], 2, [(None, 1)], 0), (t1 + [(0xDEAD, 0)], 2, [(None, 1)], 0),
            ([(sc, n - 3)], 2, [(None, 1)], 0), ([(sc, big)], 2, [(None, 1)], 0), (t1, 7, [(None, 1)], 0),
            (t1 + [(sc, n - 1)], 2, [(None, 1)], 0)):
        assert _c_round(curve, tables, nv, terms, flags) == (MSMZ_ERR_ARG, 99, b"\xaa" * 160), (nv, terms, flags)
    # host values >= q: MSMZ_ERR_RANGE, nothing launched, nothing created
    for bad in (q, q + 1, (1 << 256) - 1):
        assert _c_eq(curve, [3, bad]) == (MSMZ_ERR_RANGE, 0)
        assert _c_eq(curve, [bad]) == (MSMZ_ERR_RANGE, 0)
        assert _c_eq(curve, [3, 4], bad) == (MSMZ_ERR_RANGE, 0)
        assert _c_eval(curve, sc, 0, [bad, 3]) == (MSMZ_ERR_RANGE, untouched)
        assert _c_bind(curve, sc, 0, 2, bad) == (MSMZ_ERR_RANGE, 0)
        assert _c_bind(curve, sc, 0, 2, bad, 1, 0, 0, sc) == (MSMZ_ERR_RANGE, sc.handle)
        assert _c_round(curve, t1, 2, [(None, 1), (bad, 1)]) == (MSMZ_ERR_RANGE, 99, b"\xaa" * 160)
    assert curve.Scalar.toBigints(sc) == before
    _good_calls_are_correct(curve, q)
    with pytest.raises(ValueError):
        curve.Parallel.eqTable([q])
    with pytest.raises(TypeError):
        curve.Parallel.evaluateMle(pts, [1])
    with pytest.raises(ValueError):
        curve.Parallel.bindMle(sc, 5, out=sc, firstOut=1)
    with pytest.raises(ValueError):
        curve.Parallel.sumcheckRound([sc], [(1, 2)])
    sc.free(); pts.free()


@pytest.mark.parametrize("label", S.ALL)
def test_multi_engine_context_is_unsupported(mod, label):
    """devices = [0, 0]: the two halves of every pair live in different blocks of 2^16 entries -- all four calls are
    MSMZ_ERR_UNSUPPORTED and leave their outputs as they were; the older calls on the same context still work"""
    mod.startThreads(devices=[0, 0])
    params = mod.curves.BY_LABEL[label]
    multi = (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)
    try:
        f = multi.Parallel.randomScalars(64, 3)
        assert _c_eq(multi, [3, 4]) == (MSMZ_ERR_UNSUPPORTED, 0)
        assert _c_eval(multi, f, 0, [3, 4]) == (MSMZ_ERR_UNSUPPORTED, b"\xaa" * 32)
        assert _c_bind(multi, f, 0, 2, 5) == (MSMZ_ERR_UNSUPPORTED, 0)
        assert _c_round(multi, [(f, 0)], 2, [(None, 1)]) == (MSMZ_ERR_UNSUPPORTED, 99, b"\xaa" * 160)
        assert multi.Parallel.innerProduct(f) == sum(multi.Scalar.toBigints(f)) % S.order(label)
        f.free()
    finally:
        multi.close()
        mod.startThreads()


# ---------------------------------------------------------------------------------------------- regression guard
@pytest.mark.parametrize("label", S.ALL)
def test_older_calls_return_the_bytes_they_did(curves, label):
    """innerProduct and combineScalars share fr_block_sum and the fold kernel (which now folds several sums in one
    launch) with the new calls: one size with several tiles == Python integers"""
    curve, q = curves(label), S.order(label)
    n = 3 * 2048 + 65
    xs, ys = S.build_vectors(label, n, 4242)
    x, y = _upload(curve, xs), _upload(curve, ys)
    assert curve.Parallel.innerProduct(x, y) == sum(a * b for a, b in zip(xs, ys)) % q
    assert curve.Parallel.innerProduct(x) == sum(xs) % q
    u = random.Random(5).randrange(2, q)
    out = curve.Parallel.combineScalars(u, x, q - 1, y)
    assert curve.Scalar.toBigints(out) == [(u * a - b) % q for a, b in zip(xs, ys)]
    for arr in (x, y, out):
        arr.free()

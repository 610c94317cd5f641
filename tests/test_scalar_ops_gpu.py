"""Arithmetic over resident scalar sets on the GPU (k_scalars_combine / k_scalars_dot / k_scalars_powers,
csrc/scalar_kernels.h): downloads and sums against Python integers mod the group order, bit-exact, at the sizes where
the kernels change shape (a partial wave, several blocks, the tile edges of the dot product and a looping second
level), ranges and in-place destinations, the errors, one IPA reduction that never downloads a vector, and a
multi-engine context."""
import ctypes as C
import random

import pytest

import check_points_util as U
import scalar_ops_util as S
from oracle import c_oracle
from oracle import params as P

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]


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
    t, p = C.c_uint32(0), C.c_uint32(0)
    _lib().msmz_test_scalar_dot_geometry(C.byref(t), C.byref(p))
    return t.value, p.value


def _term(v, first=0, coeff=None, coeff_first=0):
    """one msmz_scalar_term: v a resident array or a raw handle; coeff a resident array, an int (broadcast) or None (NULL)"""
    from msm_zprize_amd._native import MsmzScalarTerm
    vh = v if isinstance(v, int) else v.handle
    if hasattr(coeff, "handle"):
        return MsmzScalarTerm(vh, first, coeff.handle, coeff_first, None)
    return MsmzScalarTerm(vh, first, 0, coeff_first, None if coeff is None else int(coeff).to_bytes(32, "little"))


def _combine(curve, x, y, n, first_out=0, out=0):
    """msmz_scalars_combine through the C ABI -> (status, *out_handle afterwards)"""
    h = C.c_uint64(out if isinstance(out, int) else out.handle)
    st = _lib().msmz_scalars_combine(curve._ctx, C.byref(x), None if y is None else C.byref(y), n, first_out, C.byref(h))
    return st, h.value


def _dot(curve, x, y, n, first_x=0, first_y=0):
    buf = C.create_string_buffer(b"\xaa" * 32, 32)
    xh = x if isinstance(x, int) else x.handle
    yh = 0 if y is None else (y if isinstance(y, int) else y.handle)
    st = _lib().msmz_scalars_dot(curve._ctx, xh, first_x, yh, first_y, n, buf)
    return st, buf.raw


def _powers(curve, base, ratio, n):
    h = C.c_uint64(0)
    st = _lib().msmz_scalars_powers(curve._ctx, None if base is None else int(base).to_bytes(32, "little"),
                                    int(ratio).to_bytes(32, "little"), n, C.byref(h))
    return st, h.value


def _take(curve, handle, n):
    """download and free a result handle"""
    from msm_zprize_amd.parallel import DeviceArray
    arr = DeviceArray(curve, handle, n, "scalars")
    vals = curve.Scalar.toBigints(arr)
    arr.free()
    return vals


def _upload(curve, vals):
    return curve.Parallel.scalarsFromBytes(S.encode(vals), len(vals))


def _plant(curve, arr, index, value):
    """make `value` (>= q) entry `index` of a resident set.  Uploads and imports refuse such a value and leave no
    handle; msmz_import_scalars_into converts before it reports, so after its MSMZ_ERR_RANGE the refused value is what
    the existing handle holds (read back here)."""
    from msm_zprize_amd._native import MsmzSrc
    raw = S.encode([value])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, arr.handle, index, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert curve.Scalar.toBigints(arr, index, 1) == [value]


_vectors = {}


def _reference(label, n):
    """four vectors of one (curve, size), made once: x, y (the planted pairs) and two coefficient vectors"""
    if (label, n) not in _vectors:
        xs, ys = S.build_vectors(label, n, 1000 * S.ALL.index(label) + n)
        cs, ds = S.build_vectors(label, n, 77000 + 1000 * S.ALL.index(label) + n)
        _vectors[(label, n)] = (xs, ys, ds, cs)   # (c rotated against x: planted rows meet other planted rows)
    return _vectors[(label, n)]


# ---------------------------------------------------------------------------------------------- combine
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("label", S.ALL)
def test_combine_forms(curves, label, n):
    """every form of out_i = A_i x_i (+ B_i y_i) == Python integers, bit-exact: one term broadcast, Hadamard, two terms
    broadcast/broadcast, vector/broadcast, vector/vector, and NULL coefficients (x + y: the planted pairs sum to exactly
    q, q - 1 and 0; with explicit coefficients 1 the same sums go through the Montgomery product)"""
    curve, q = curves(label), S.order(label)
    xs, ys, cs, ds = _reference(label, n)
    rng = random.Random(n)
    a, b = rng.randrange(2, q), rng.randrange(2, q)
    x, y, c, d = (_upload(curve, v) for v in (xs, ys, cs, ds))
    forms = [
        ("a x", _term(x, 0, a), None, [a * v % q for v in xs]),
        ("0 x", _term(x, 0, 0), None, [0] * n),
        ("(q-1) x", _term(x, 0, q - 1), None, [(q - 1) * v % q for v in xs]),
        ("c . x", _term(x, 0, c), None, [u * v % q for u, v in zip(cs, xs)]),
        ("a x + b y", _term(x, 0, a), _term(y, 0, b), [(a * u + b * v) % q for u, v in zip(xs, ys)]),
        ("c . x + b y", _term(x, 0, c), _term(y, 0, b), [(w * u + b * v) % q for w, u, v in zip(cs, xs, ys)]),
        ("c . x + d . y", _term(x, 0, c), _term(y, 0, d), [(w * u + z * v) % q for w, u, z, v in zip(cs, xs, ds, ys)]),
        ("x", _term(x), None, xs),
        ("x + y", _term(x), _term(y), [(u + v) % q for u, v in zip(xs, ys)]),
        ("1 x + 1 y", _term(x, 0, 1), _term(y, 0, 1), [(u + v) % q for u, v in zip(xs, ys)]),
        ("x + (q-1) y", _term(x), _term(y, 0, q - 1), [(u - v) % q for u, v in zip(xs, ys)]),
    ]
    for name, tx, ty, want in forms:
        st, h = _combine(curve, tx, ty, n)
        assert st == 0 and h != 0, (name, st)
        got = _take(curve, h, n)
        bad = [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (name, bad[:3])
    assert 0 in forms[8][3][:64]   # (a planted pair did sum to q)
    for arr in (x, y, c, d):
        arr.free()


@pytest.mark.parametrize("label", S.ALL)
def test_combine_ranges_and_in_place(curves, label):
    """first* non-zero with x, y and the coefficients as ranges of ONE handle; then in place: destination == x range,
    == y range, and disjoint inside the same handle -- every entry outside [first_out, first_out + n) unchanged, the
    neighbours on both sides included; a partial overlap is MSMZ_ERR_ARG and leaves the handle as it was"""
    curve, q = curves(label), S.order(label)
    total, n = 700, 130   # (130: two full waves and a partial one; no range starts at a multiple of 64)
    vals, _ = S.build_vectors(label, total, 31)
    v = _upload(curve, vals)
    fx, fy, fc = 7, 301, 450
    u = random.Random(3).randrange(2, q)
    st, h = _combine(curve, _term(v, fx, v, fc), _term(v, fy, u), n)
    assert st == 0
    assert _take(curve, h, n) == [(vals[fc + i] * vals[fx + i] + u * vals[fy + i]) % q for i in range(n)]
    for first_out in (fx, fy, 150, 570, 0):   # == x range, == y range, disjoint between them, disjoint at the end / start
        if first_out == 0:
            n_, fx_ = 7, 7                      # [0, 7) ends where the x range [7, 14) begins
        else:
            n_, fx_ = n, fx
        want = list(vals)
        for i in range(n_):
            want[first_out + i] = (vals[fx_ + i] + u * vals[fy + i]) % q
        st, h = _combine(curve, _term(v, fx_), _term(v, fy, u), n_, first_out, v)
        assert (st, h) == (0, v.handle), first_out
        got = curve.Scalar.toBigints(v)
        assert got[first_out:first_out + n_] == want[first_out:first_out + n_], first_out
        assert got == want, first_out
        vals = want
    for first_out in (fx + 1, fx - 1, fy + n - 1, fy - n + 1, fx + 64):
        assert _combine(curve, _term(v, fx), _term(v, fy, u), n, first_out, v) == (MSMZ_ERR_ARG, v.handle), first_out
    assert _combine(curve, _term(v, fx, v, fc), None, n, fc + 1, v) == (MSMZ_ERR_ARG, v.handle)   # the coefficient range
    assert curve.Scalar.toBigints(v) == vals
    v.free()


@pytest.mark.parametrize("label", S.ALL)
def test_combined_handle_feeds_an_msm(curves, label):
    """the result is an ordinary scalar set: msmz_msm_resident over it == the oracle's MSM of the expected scalars"""
    curve, params, q = curves(label), P.CURVES[label], S.order(label)
    n = 257
    xs, ys, _, _ = _reference(label, n)
    a, b = 5, random.Random(8).randrange(q)
    x, y = _upload(curve, xs), _upload(curve, ys)
    pts = curve.Parallel.randomPointsFast(n, 17)
    out = curve.Parallel.combineScalars(a, x, b, y)
    assert len(out) == n and out.kind == "scalars"
    want = c_oracle.msm(params, [(a * u + b * v) % q for u, v in zip(xs, ys)], curve.Affine.toBigints(pts))
    assert curve.Parallel.msm(out, pts, n)["result"] == want
    for arr in (x, y, pts, out):
        arr.free()


# ---------------------------------------------------------------------------------------------- dot
def _dot_sizes():
    t, pp = _geometry()
    return [1, 63, 64, 65, 257, t - 1, t, t + 1, 3 * t + 65, t * pp + 1]


@pytest.mark.parametrize("label", S.ALL)
def test_dot(curves, label):
    """sum x_i y_i and sum x_i == Python integers at the wave, tile and pass edges (T * Pp + 1: the second level loops),
    the planted pairs in the first and last wave; two calls return the same bytes"""
    curve, q = curves(label), S.order(label)
    sizes = _dot_sizes()
    assert sizes[-1] == 2048 * 256 + 1 or sizes[-1] > sizes[-2]
    for n in sizes:
        xs, ys = S.build_vectors(label, n, 500 + n)
        x, y = _upload(curve, xs), _upload(curve, ys)
        st, got = _dot(curve, x, y, n)
        assert st == 0, n
        assert int.from_bytes(got, "little") == sum(u * v for u, v in zip(xs, ys)) % q, n
        assert _dot(curve, x, y, n) == (0, got)
        st, got = _dot(curve, x, None, n)
        assert st == 0 and int.from_bytes(got, "little") == sum(xs) % q, n
        st, got = _dot(curve, y, None, n)
        assert st == 0 and int.from_bytes(got, "little") == sum(ys) % q, n
        x.free(); y.free()


@pytest.mark.parametrize("label", S.ALL)
def test_dot_largest_accumulations_and_overlap(curves, label):
    """all-(q - 1) vectors: every product and every partial sum is as large as it gets; x and y as overlapping ranges of
    one handle; ranges that start off a wave boundary; the Python surface"""
    curve, q = curves(label), S.order(label)
    t, _ = _geometry()
    for n in (65, 257, 3 * t + 65):
        x = _upload(curve, [q - 1] * n)
        assert _dot(curve, x, x, n) == (0, (n % q).to_bytes(32, "little"))
        assert _dot(curve, x, None, n) == (0, (n * (q - 1) % q).to_bytes(32, "little"))
        x.free()
    total = 2 * t + 300
    vals, _ = S.build_vectors(label, total, 91)
    v = _upload(curve, vals)
    for n, fx, fy in ((t + 200, 0, 7), (t + 200, 93, 1), (total - 64, 64, 0), (total, 0, 0)):
        st, got = _dot(curve, v, v, n, fx, fy)
        assert st == 0 and int.from_bytes(got, "little") == sum(vals[fx + i] * vals[fy + i] for i in range(n)) % q, (n, fx, fy)
        st, got = _dot(curve, v, None, n, fx)
        assert st == 0 and int.from_bytes(got, "little") == sum(vals[fx:fx + n]) % q
    assert curve.Parallel.innerProduct(v, v, 100, 5, 50) == sum(vals[5 + i] * vals[50 + i] for i in range(100)) % q
    assert curve.Parallel.innerProduct(v) == sum(vals) % q
    v.free()


# ---------------------------------------------------------------------------------------------- powers
@pytest.mark.parametrize("label", S.ALL)
def test_powers(curves, label):
    """entry i = base ratio^i for n over {1, 2, 33, 257, 65537} (a partial run, several blocks, past the 2^16 block of a
    split), ratio over {0, 1, q - 1, random}, base over {NULL, 0, random}"""
    curve, q = curves(label), S.order(label)
    rng = random.Random(S.ALL.index(label) + 40)
    for ratio in (0, 1, q - 1, rng.randrange(2, q)):
        for base in (None, 0, rng.randrange(2, q)):
            for n in (1, 2, 33, 257, 65537):
                st, h = _powers(curve, base, ratio, n)
                assert st == 0 and h != 0, (ratio, base, n)
                got = _take(curve, h, n)
                want, acc = [], 1 if base is None else base
                for _ in range(n):
                    want.append(acc)
                    acc = acc * ratio % q
                bad = [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
                assert not bad, (hex(ratio), base, n, bad[:3])
    z = rng.randrange(2, q)
    arr = curve.Parallel.scalarPowers(z, 100, 3)
    assert curve.Scalar.toBigints(arr) == [3 * pow(z, i, q) % q for i in range(100)]
    arr.free()


# ---------------------------------------------------------------------------------------------- errors
def _good_calls_are_correct(curve, q):
    xs = [5, q - 1, 77] + [9] * 70
    x = _upload(curve, xs)
    st, h = _combine(curve, _term(x, 0, 3), _term(x), len(xs))
    assert st == 0 and _take(curve, h, len(xs)) == [4 * v % q for v in xs]
    assert _dot(curve, x, x, len(xs)) == (0, (sum(v * v for v in xs) % q).to_bytes(32, "little"))
    x.free()


@pytest.mark.parametrize("label", S.ALL)
def test_resident_entry_out_of_range(curves, label):
    """ONE entry >= q at the first, a middle and the last index, in x, in y and in a coefficient vector: combine and dot
    return MSMZ_ERR_RANGE, *out_handle stays 0, a following good call is correct, and the same entry OUTSIDE the
    addressed range is no error"""
    curve, q = curves(label), S.order(label)
    n = 300
    rng = random.Random(12)
    vals = [rng.randrange(q) for _ in range(n)]
    good = _upload(curve, vals)
    for index, bad_value in ((0, q), (150, (1 << 256) - 1), (n - 1, q + 1)):
        bad = _upload(curve, vals)
        _plant(curve, bad, index, bad_value)
        for x, y, c in ((bad, good, good), (good, bad, good), (good, good, bad)):
            assert _combine(curve, _term(x, 0, c), _term(y, 0, 5), n) == (MSMZ_ERR_RANGE, 0), index
            assert _combine(curve, _term(y, 0, 5), _term(x, 0, c), n) == (MSMZ_ERR_RANGE, 0), index
        assert _combine(curve, _term(bad), None, n) == (MSMZ_ERR_RANGE, 0)
        for x, y in ((bad, good), (good, bad), (bad, None)):
            st, raw = _dot(curve, x, y, n)
            assert st == MSMZ_ERR_RANGE, index
        _good_calls_are_correct(curve, q)
        # ranges clear of the bad entry
        lo, cnt = (1, n - 1) if index == 0 else (0, index)
        st, h = _combine(curve, _term(bad, lo, good, lo), _term(good, lo, bad, lo), cnt)
        assert st == 0
        assert _take(curve, h, cnt) == [2 * vals[lo + i] * vals[lo + i] % q for i in range(cnt)]
        assert _dot(curve, bad, bad, cnt, lo, lo) == (0, (sum(v * v for v in vals[lo:lo + cnt]) % q).to_bytes(32, "little"))
        bad.free()
    good.free()


@pytest.mark.parametrize("label", S.ALL)
def test_argument_errors(curves, label):
    """MSMZ_ERR_ARG before any launch, outputs untouched; broadcast values >= q are MSMZ_ERR_RANGE with nothing launched"""
    curve, q = curves(label), S.order(label)
    n = 100
    sc = curve.Parallel.randomScalars(n, 2)
    pts = curve.Parallel.randomPointsFast(n, 2)
    before = curve.Scalar.toBigints(sc)
    lib = _lib()
    h = C.c_uint64(0)
    one = (1).to_bytes(32, "little")
    assert lib.msmz_scalars_combine(curve._ctx, None, None, n, 0, C.byref(h)) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_combine(curve._ctx, C.byref(_term(sc)), None, n, 0, None) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_dot(curve._ctx, sc.handle, 0, 0, 0, n, None) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_powers(curve._ctx, one, None, n, C.byref(h)) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_powers(curve._ctx, one, one, n, None) == MSMZ_ERR_ARG
    big = (1 << 64) - 1
    for tx, ty, cnt, first_out, out in [
            (_term(sc), None, 0, 0, 0), (_term(sc), None, 1 << 32, 0, 0),               # n == 0, n >= 2^32
            (_term(0xDEAD), None, n, 0, 0), (_term(sc), _term(0xDEAD), n, 0, 0),        # unknown handles
            (_term(sc, 0, None), None, n, 0, 0xDEAD),
            (_term(pts), None, n, 0, 0), (_term(sc), _term(pts), n, 0, 0), (_term(sc), None, n, 0, pts.handle),   # not scalar sets
            (_term(sc, 1), None, n, 0, 0), (_term(sc, n), None, 1, 0, 0), (_term(sc, big), None, 2, 0, 0),   # beyond / wraps
            (_term(sc), _term(sc, 51), 50, 0, 0), (_term(sc), _term(sc, big), 2, 0, 0),
            (_term(sc), None, n + 1, 0, 0),
            (_term(sc), None, 10, 91, sc.handle), (_term(sc), None, 2, big, sc.handle),   # the destination range
            (_term(sc), None, 10, 1, 0)]:                                                # first_out without a handle
        st, hh = _combine(curve, tx, ty, cnt, first_out, out)
        assert (st, hh) == (MSMZ_ERR_ARG, out), (cnt, first_out)
    from msm_zprize_amd._native import MsmzScalarTerm
    for tx in (MsmzScalarTerm(sc.handle, 0, 0xDEAD, 0, None), MsmzScalarTerm(sc.handle, 0, pts.handle, 0, None),
               MsmzScalarTerm(sc.handle, 0, sc.handle, 1, None), MsmzScalarTerm(sc.handle, 0, sc.handle, big, None)):
        assert _combine(curve, tx, None, n) == (MSMZ_ERR_ARG, 0)
    untouched = b"\xaa" * 32
    for x, y, cnt, fx, fy in [(sc, None, 0, 0, 0), (sc, None, 1 << 32, 0, 0), (0xDEAD, None, n, 0, 0), (sc, 0xDEAD, n, 0, 0),
                              (pts.handle, None, n, 0, 0), (sc, pts.handle, n, 0, 0), (sc, None, n, 1, 0), (sc, sc, n, 0, 1),
                              (sc, None, 2, big, 0), (sc, sc, 2, 0, big), (sc, None, n, 0, 1)]:
        assert _dot(curve, x, y, cnt, fx, fy) == (MSMZ_ERR_ARG, untouched), (cnt, fx, fy)
    assert _powers(curve, 1, 2, 0) == (MSMZ_ERR_ARG, 0) and _powers(curve, 1, 2, 1 << 32) == (MSMZ_ERR_ARG, 0)
    for bad in (q, q + 1, (1 << 256) - 1):   # broadcast values: the host refuses
        assert _combine(curve, _term(sc, 0, bad), None, n) == (MSMZ_ERR_RANGE, 0)
        assert _combine(curve, _term(sc), _term(sc, 0, bad), n) == (MSMZ_ERR_RANGE, 0)
        assert _combine(curve, _term(sc, 0, bad), None, n, 0, sc) == (MSMZ_ERR_RANGE, sc.handle)
        assert _powers(curve, bad, 2, n) == (MSMZ_ERR_RANGE, 0)
        assert _powers(curve, 2, bad, n) == (MSMZ_ERR_RANGE, 0)
        assert _powers(curve, None, bad, n) == (MSMZ_ERR_RANGE, 0)
    assert curve.Scalar.toBigints(sc) == before   # (a refused in-place call launched nothing)
    _good_calls_are_correct(curve, q)
    with pytest.raises(ValueError):
        curve.Parallel.combineScalars(q, sc)
    with pytest.raises(ValueError):
        curve.Parallel.combineScalars(1, sc, 2, sc, 50, 0, 50, sc, 1)
    with pytest.raises(TypeError):
        curve.Parallel.innerProduct(pts)
    with pytest.raises(ValueError):
        curve.Parallel.scalarPowers(q, 4)
    sc.free(); pts.free()


# ---------------------------------------------------------------------------------------------- one IPA reduction
@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_ipa_reduction_on_the_device(curves, label):
    """n = 64 down to 1 in six rounds over a, b (scalars) and G (points): L and R from msmSegments, the cross terms
    from innerProduct, the folds a' = a_lo + u^-1 a_hi and b' = b_lo + u b_hi in place on the halves of one handle,
    G' = G_lo + [u] G_hi by mulPoints.  Per round <a', G'> == <a, G> + [u] L + [u^-1] R (host: the oracle's scalar
    multiplication, msmz_point_add) and <a', b'> == <a, b> + u <a_lo, b_hi> + u^-1 <a_hi, b_lo>.  No vector is downloaded
    inside the loop."""
    curve, params, q = curves(label), P.CURVES[label], S.order(label)
    n = 64
    par = curve.Parallel
    a, b, G = par.randomScalars(n, 61), par.randomScalars(n, 62), par.randomPointsFast(n, 63)
    rng = random.Random(64)
    commit = par.msm(a, G, n)["result"]
    inner = par.innerProduct(a, b, n)
    rounds = 0
    while n > 1:
        h = n // 2
        u = rng.randrange(2, q)
        uinv = pow(u, -1, q)
        L, R = par.msmSegments(a, G, [(h, 0, h), (0, h, h)])        # <a_lo, G_hi>, <a_hi, G_lo>
        cl = par.innerProduct(a, b, h, 0, h)                         # <a_lo, b_hi>
        cr = par.innerProduct(a, b, h, h, 0)                         # <a_hi, b_lo>
        assert par.combineScalars(1, a, uinv, a, h, 0, h, out=a) is a
        assert par.combineScalars(1, b, u, b, h, 0, h, out=b) is b
        folded = par.mulPoints(u, G, h, addend=G, firstPoint=h)
        G.free()
        G = folded
        n = h
        want = curve.pointAdd(curve.pointAdd(commit, U.scale(params, u, L)), U.scale(params, uinv, R))
        commit = par.msm(a, G, n)["result"]
        assert (commit["x"], commit["y"], bool(commit["isZero"])) == (want["x"], want["y"], bool(want["isZero"])), rounds
        want_inner = (inner + u * cl + uinv * cr) % q
        inner = par.innerProduct(a, b, n)
        assert inner == want_inner, rounds
        rounds += 1
    assert rounds == 6 and len(a) == 64 and len(G) == 1
    a0, b0 = curve.Scalar.toBigints(a, 0, 1)[0], curve.Scalar.toBigints(b, 0, 1)[0]
    assert a0 * b0 % q == inner
    for arr in (a, b, G):
        arr.free()


# ---------------------------------------------------------------------------------------------- multi-engine contexts
@pytest.mark.parametrize("label", S.ALL)
def test_multi_engine_context(mod, curves, label):
    """devices = [0, 0], n = 2^16 + 257 (block 0 on one engine, 257 entries of block 1 on the other): combine with all
    firsts 0 (new and over a whole existing set), dot and powers equal the single-engine results; a non-zero first is
    MSMZ_ERR_UNSUPPORTED"""
    params, q = P.CURVES[label], S.order(label)
    n = (1 << 16) + 257
    rng = random.Random(21)
    u, z, base = rng.randrange(2, q), rng.randrange(2, q), rng.randrange(2, q)

    def run(curve):
        x, y, c = (curve.Parallel.randomScalars(n, seed) for seed in (71, 72, 73))
        outs = []
        st, h = _combine(curve, _term(x, 0, c), _term(y, 0, u), n)
        assert st == 0
        outs.append(_take(curve, h, n))
        outs.append(_dot(curve, x, y, n))
        outs.append(_dot(curve, x, None, n))
        st, h = _powers(curve, base, z, n)
        assert st == 0
        outs.append(_take(curve, h, n))
        assert _combine(curve, _term(x, 0, u), _term(y), n, 0, x) == (0, x.handle)   # in place over the whole set
        outs.append(curve.Scalar.toBigints(x))
        calls = [_combine(curve, _term(x, 1), None, 10), _combine(curve, _term(x), _term(y, 1 << 16), 10),
                 _combine(curve, _term(x, 0, c, 1), None, 10), _combine(curve, _term(x), None, 10, 5, y),
                 _combine(curve, _term(x), None, 10, 0, y),   # a destination that is not written whole
                 (_dot(curve, x, y, 10, 1, 0)[0], 0), (_dot(curve, x, y, 10, 0, 1 << 16)[0], 0)]
        for st, h in calls[:3]:
            if st == 0:
                assert _lib().msmz_free(curve._ctx, h) == 0   # (a single engine takes these ranges)
        refused = [st for st, _ in calls]
        for arr in (x, y, c):
            arr.free()
        return outs, refused

    want, ok = run(curves(label))
    assert ok == [0] * 7
    assert want[3][:3] == [base, base * z % q, base * z * z % q] and want[3][-1] == base * pow(z, n - 1, q) % q
    mod.startThreads(devices=[0, 0])
    mparams = mod.curves.BY_LABEL[label]
    multi = (mod.Weierstrass if mparams["kind"] == "weierstrass" else mod.TwistedEdwards).create(mparams)
    try:
        got, refused = run(multi)
        assert got == want
        assert refused == [MSMZ_ERR_UNSUPPORTED] * 7
    finally:
        multi.close()
        mod.startThreads()

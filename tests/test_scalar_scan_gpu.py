"""Recurrences and inversion over resident scalar sets on the GPU (k_scalars_rec_tile / _carry / _apply and
k_scalars_inverse, csrc/scan_kernels.h): downloads and final values against Python integers mod the group order,
bit-exact, at the sizes where the kernels change shape (a partial wave, the tile edges, more tile aggregates than one
pass of the carry kernel, the chunk edges of the inversion), values that stress the arithmetic, ranges and in-place
destinations, the errors, a KZG opening and a grand product that never download an intermediate vector, and a
two-engine context.  Sizes come from msmz_test_scalar_scan_geometry."""
import ctypes as C
import random

import pytest

import check_points_util as CP
import scalar_ops_util as S
import scalar_scan_util as U
from oracle import params as P

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
REVERSE, EXCLUSIVE = 1, 2
UNTOUCHED = b"\xaa" * 32


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
    t, p, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    _lib().msmz_test_scalar_scan_geometry(C.byref(t), C.byref(p), C.byref(c))
    assert t.value >= 256 and p.value >= 64 and c.value >= 64
    return t.value, p.value, c.value


def _handle(v):
    return 0 if v is None else (v if isinstance(v, int) else v.handle)


class Raw(int):
    """a raw handle value in the place of `a` (a plain int there is a broadcast multiplier)"""
    @property
    def handle(self):
        return int(self)


def _rec(curve, a, b, n, flags=0, init=None, first_a=0, first_b=0, first_out=0, out=0):
    """msmz_scalars_recurrence through the C ABI.  a: a resident array / Raw handle, an int (broadcast) or None; b: a
    resident array / raw handle or None -> (status, *out_handle afterwards, the bytes of `last`)"""
    from msm_zprize_amd._native import MsmzScalarRec
    resident = hasattr(a, "handle")
    rec = MsmzScalarRec(a.handle if resident else 0, first_a,
                        None if resident or a is None else int(a).to_bytes(32, "little"), _handle(b), first_b,
                        None if init is None else int(init).to_bytes(32, "little"), flags)
    h = C.c_uint64(_handle(out))
    last = C.create_string_buffer(UNTOUCHED, 32)
    st = _lib().msmz_scalars_recurrence(curve._ctx, C.byref(rec), n, first_out, C.byref(h), last)
    return st, h.value, last.raw


def _inv(curve, x, n, first=0, first_out=0, out=0):
    """msmz_scalars_inverse -> (status, *out_handle afterwards, *n_zero afterwards)"""
    h = C.c_uint64(_handle(out))
    zeros = C.c_uint64(1 << 40)
    st = _lib().msmz_scalars_inverse(curve._ctx, _handle(x), first, n, first_out, C.byref(h), C.byref(zeros))
    return st, h.value, zeros.value


def _take(curve, handle, n):
    """download and free a result handle"""
    from msm_zprize_amd.parallel import DeviceArray
    arr = DeviceArray(curve, handle, n, "scalars")
    vals = curve.Scalar.toBigints(arr)
    arr.free()
    return vals


def _raw(curve, arr, first, n):
    buf = C.create_string_buffer(32 * n)
    assert _lib().msmz_download_scalars(curve._ctx, _handle(arr), first, n, buf) == 0
    return buf.raw


def _upload(curve, vals):
    return curve.Parallel.scalarsFromBytes(S.encode(vals), len(vals))


def _plant(curve, arr, index, value):
    """make `value` (>= q) entry `index` of a resident set, as tests/test_scalar_ops_gpu.py does: msmz_import_scalars_into
    converts before it reports, so after its MSMZ_ERR_RANGE the refused value is what the handle holds"""
    from msm_zprize_amd._native import MsmzSrc
    raw = S.encode([value])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, arr.handle, index, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert curve.Scalar.toBigints(arr, index, 1) == [value]


def _check(curve, q, n, a_vals, b_vals, a, b, flags, init=None, what=""):
    """one recurrence into a new handle == the plain loop, entries and last"""
    st, h, last = _rec(curve, a, b, n, flags, init)
    assert st == 0 and h != 0, (what, n, flags, st)
    want, want_last = U.recurrence(q, n, a_vals, b_vals, init, bool(flags & REVERSE), bool(flags & EXCLUSIVE))
    got = _take(curve, h, n)
    bad = [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (what, n, flags, bad[:3])
    assert int.from_bytes(last, "little") == want_last, (what, n, flags)


# ---------------------------------------------------------------------------------------------- sizes
def _edge_sizes():
    t = _geometry()[0]
    return [1, 2, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 2 * t + 1]


@pytest.mark.parametrize("label", S.ALL)
def test_edge_sizes_every_mode(curves, label):
    """{1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 T + 1} x the five modes x forward / reverse x inclusive /
    exclusive: every downloaded entry and `last`, bit-exact"""
    curve, q = curves(label), S.order(label)
    for n in _edge_sizes():
        xs, ys = S.build_vectors(label, n, 1000 * S.ALL.index(label) + n)
        k = random.Random(n).randrange(2, q)
        x, y = _upload(curve, xs), _upload(curve, ys)
        for mode, mult, addend in U.MODES:
            a_vals = None if mult is None else (k if mult == "broadcast" else xs)
            a = None if mult is None else (k if mult == "broadcast" else x)
            for flags in range(4):
                _check(curve, q, n, a_vals, ys if addend else None, a, y if addend else None, flags, None, mode)
        x.free(); y.free()


@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_more_aggregates_than_one_carry_pass(curves, label):
    """T P - 1, T P and T P + 1 entries: the one workgroup of the carry launch loops and hands its running value from
    pass to pass.  Two modes: resident multiplier with resident addend (forward, over the prefixes of one device-made
    set) and a broadcast multiplier in reverse (over the suffixes, so that one Python loop serves the three sizes)."""
    curve, q = curves(label), S.order(label)
    t, p, _ = _geometry()
    top = t * p + 1
    a = curve.Parallel.randomScalars(top, 101)
    b = curve.Parallel.randomScalars(top, 102)
    av, bv = S.decode(_raw(curve, a, 0, top)), S.decode(_raw(curve, b, 0, top))
    z = random.Random(5).randrange(2, q)
    init = random.Random(6).randrange(q)
    fwd, y = [], init
    for i in range(top):
        y = (av[i] * y + bv[i]) % q
        fwd.append(y)
    rev, y = [0] * top, init
    for i in range(top - 1, -1, -1):
        y = (z * y + bv[i]) % q
        rev[i] = y
    fwd_raw, rev_raw = S.encode(fwd), S.encode(rev)
    for n in (top - 2, top - 1, top):
        st, h, last = _rec(curve, a, b, n, 0, init)
        assert st == 0, n
        assert int.from_bytes(last, "little") == fwd[n - 1], n
        assert _raw(curve, h, 0, n) == fwd_raw[:32 * n], n
        assert _lib().msmz_free(curve._ctx, h) == 0
        first = top - n
        st, h, last = _rec(curve, z, b, n, REVERSE, init, 0, first)
        assert st == 0, n
        assert int.from_bytes(last, "little") == rev[first], n
        assert _raw(curve, h, 0, n) == rev_raw[32 * first:], n
        assert _lib().msmz_free(curve._ctx, h) == 0
    a.free(); b.free()


@pytest.mark.parametrize("label", S.ALL)
def test_values_that_stress_the_arithmetic(curves, label):
    """multipliers all q - 1; multipliers with a 0 (what came before is forgotten); init = q - 1; addends all q - 1 over
    more than T entries (every addition wraps)"""
    curve, q = curves(label), S.order(label)
    t = _geometry()[0]
    n = t + 70
    rng = random.Random(9)
    ones = [q - 1] * n
    mixed = [rng.randrange(1, q) for _ in range(n)]
    holed = list(mixed)
    for i in (0, 63, t - 1, t, n - 1):
        holed[i] = 0
    m1, mx, hz = _upload(curve, ones), _upload(curve, mixed), _upload(curve, holed)
    for flags in range(4):
        _check(curve, q, n, ones, None, m1, None, flags, None, "products of q - 1")
        _check(curve, q, n, ones, ones, m1, m1, flags, q - 1, "a = b = init = q - 1")
        _check(curve, q, n, None, ones, None, m1, flags, q - 1, "sums of q - 1")
        _check(curve, q, n, q - 1, ones, q - 1, m1, flags, q - 1, "broadcast q - 1")
        _check(curve, q, n, holed, mixed, hz, mx, flags, q - 1, "multipliers with zeros")
        _check(curve, q, n, holed, None, hz, None, flags, None, "products through zeros")
        _check(curve, q, n, 0, mixed, 0, mx, flags, 5, "broadcast 0")
        _check(curve, q, n, 1, mixed, 1, mx, flags, 0, "broadcast 1")
    for arr in (m1, mx, hz):
        arr.free()


# ---------------------------------------------------------------------------------------------- ranges
@pytest.mark.parametrize("label", S.ALL)
def test_ranges_and_in_place(curves, label):
    """a, b and the destination as ranges of ONE handle with non-zero firsts; a destination inside a larger handle with
    its neighbours unchanged on both sides; the destination exactly the a range and exactly the b range; a partial
    overlap is MSMZ_ERR_ARG and leaves the handle as it was"""
    curve, q = curves(label), S.order(label)
    t = _geometry()[0]
    n = t + 130
    total = 3 * n + 300
    vals, _ = S.build_vectors(label, total, 41)
    v = _upload(curve, vals)
    fa, fb = 7, n + 93
    st, h, last = _rec(curve, v, v, n, 0, 3, fa, fb)
    assert st == 0
    want, want_last = U.recurrence(q, n, vals[fa:fa + n], vals[fb:fb + n], 3)
    assert _take(curve, h, n) == want and int.from_bytes(last, "little") == want_last
    for first_out, flags in ((2 * n + 150, 0), (fa, REVERSE), (fb, EXCLUSIVE), (fa, EXCLUSIVE | REVERSE), (fb, 0)):
        out, want_last = U.recurrence(q, n, vals[fa:fa + n], vals[fb:fb + n], 3, bool(flags & REVERSE), bool(flags & EXCLUSIVE))
        want = vals[:first_out] + out + vals[first_out + n:]
        st, h, last = _rec(curve, v, v, n, flags, 3, fa, fb, first_out, v)
        assert (st, h) == (0, v.handle), first_out
        assert int.from_bytes(last, "little") == want_last, first_out
        got = curve.Scalar.toBigints(v)
        assert got[first_out:first_out + n] == out, (first_out, flags)
        assert got == want, (first_out, flags)
        vals = want
    # one operand in place: prefix products over the a range, prefix sums over the b range, a broadcast multiplier
    for a, b, first_a, first_b, first_out in ((v, None, fa, 0, fa), (None, v, 0, fb, fb), (5, v, 0, fb, fb)):
        out, want_last = U.recurrence(q, n, None if a is None else (5 if a == 5 else vals[first_a:first_a + n]),
                                      None if b is None else vals[first_b:first_b + n])
        st, h, last = _rec(curve, a, b, n, 0, None, first_a, first_b, first_out, v)
        assert (st, h) == (0, v.handle)
        vals = vals[:first_out] + out + vals[first_out + n:]
        assert curve.Scalar.toBigints(v) == vals and int.from_bytes(last, "little") == want_last
    for first_out in (fa + 1, fa - 1, fb + n - 1, fb - n + 1, fa + 64):
        assert _rec(curve, v, v, n, 0, None, fa, fb, first_out, v) == (MSMZ_ERR_ARG, v.handle, UNTOUCHED), first_out
    assert _rec(curve, 5, v, n, 0, None, 0, fb, fb + 1, v) == (MSMZ_ERR_ARG, v.handle, UNTOUCHED)
    assert _inv(curve, v, n, fa, fa + 1, v)[:2] == (MSMZ_ERR_ARG, v.handle)
    assert curve.Scalar.toBigints(v) == vals
    v.free()


# ---------------------------------------------------------------------------------------------- inverse
@pytest.mark.parametrize("label", S.ALL)
def test_inverse(curves, label):
    """sizes {1, 63, 64, 65, C - 1, C, C + 1, 3 C + 7}; zeros nowhere, at the first entry, at the last, on both sides of
    a chunk edge, over a whole chunk, everywhere: out, n_zero, and x_i out_i == 1 or both 0; then in place; q - 1 -> q - 1
    and 1 -> 1"""
    curve, q = curves(label), S.order(label)
    c = _geometry()[2]
    rng = random.Random(31 + S.ALL.index(label))
    for n in (1, 63, 64, 65, c - 1, c, c + 1, 3 * c + 7):
        base = [rng.randrange(2, q) for _ in range(n)]
        for i, v in zip((0, n // 2, n - 1), (q - 1, 1, q - 1)):
            base[i] = v
        inv_base = [pow(v, -1, q) for v in base]
        assert inv_base[0] == q - 1 and inv_base[n // 2] in (1, q - 1)
        placements = [[], [0], [n - 1], [i for i in (c - 1, c) if i < n], list(range(c, min(2 * c, n))), list(range(n))]
        for k, zeros in enumerate(placements):
            if k and not zeros:
                continue
            zs = set(zeros)
            xs = [0 if i in zs else v for i, v in enumerate(base)]
            want = [0 if i in zs else v for i, v in enumerate(inv_base)]
            x = _upload(curve, xs)
            st, h, nz = _inv(curve, x, n)
            assert (st, nz) == (0, len(zs)) and h != 0, (n, k)
            got = _take(curve, h, n)
            assert got == want, (n, k)
            assert all((u * w % q == 1) or (u == 0 and w == 0) for u, w in zip(xs, got))
            assert _inv(curve, x, n, 0, 0, x) == (0, x.handle, len(zs))      # in place
            assert curve.Scalar.toBigints(x) == want, (n, k)
            x.free()
    # a range of a larger set into a range of another; the Python surface
    vals = [rng.randrange(q) for _ in range(c + 200)]
    vals[150] = 0
    x, y = _upload(curve, vals), _upload(curve, vals)
    out, zeros = curve.Parallel.invertScalars(x, c + 50, 100, y, 30)
    assert out is y and zeros == 1
    assert curve.Scalar.toBigints(y) == vals[:30] + U.inverse(q, vals[100:c + 150])[0] + vals[c + 80:]
    assert curve.Scalar.toBigints(x) == vals
    x.free(); y.free()


# ---------------------------------------------------------------------------------------------- errors
def _good_calls_are_correct(curve, q):
    xs = [5, q - 1, 77, 0] + [9] * 70
    x = _upload(curve, xs)
    _check(curve, q, len(xs), xs, xs, x, x, 0, 2, "after an error")
    st, h, nz = _inv(curve, x, len(xs))
    assert (st, nz) == (0, 1) and _take(curve, h, len(xs)) == U.inverse(q, xs)[0]
    x.free()


@pytest.mark.parametrize("label", S.ALL)
def test_resident_entry_out_of_range(curves, label):
    """ONE entry >= q at the first, a middle and the last index of a, of b and of the inverse's operand: MSMZ_ERR_RANGE,
    *out_handle stays 0, `last` and `n_zero` stay as they were, a following good call is correct; the same entry OUTSIDE
    the addressed range is not read"""
    curve, q = curves(label), S.order(label)
    t = _geometry()[0]
    n = t + 300
    rng = random.Random(12)
    vals = [rng.randrange(1, q) for _ in range(n)]
    good = _upload(curve, vals)
    for index, bad_value in ((0, q), (t + 1, (1 << 256) - 1), (n - 1, q + 1)):
        bad = _upload(curve, vals)
        _plant(curve, bad, index, bad_value)
        for a, b in ((bad, good), (good, bad), (bad, None), (None, bad), (7, bad)):
            for flags in (0, REVERSE | EXCLUSIVE):
                assert _rec(curve, a, b, n, flags) == (MSMZ_ERR_RANGE, 0, UNTOUCHED), (index, flags)
        assert _inv(curve, bad, n) == (MSMZ_ERR_RANGE, 0, 1 << 40)
        _good_calls_are_correct(curve, q)
        lo, cnt = (1, n - 1) if index == 0 else (0, index)   # ranges clear of the bad entry
        st, h, last = _rec(curve, bad, bad, cnt, 0, None, lo, lo)
        want, want_last = U.recurrence(q, cnt, vals[lo:lo + cnt], vals[lo:lo + cnt])
        assert st == 0 and _take(curve, h, cnt) == want and int.from_bytes(last, "little") == want_last
        st, h, nz = _inv(curve, bad, cnt, lo)
        assert (st, nz) == (0, 0) and _take(curve, h, cnt) == U.inverse(q, vals[lo:lo + cnt])[0]
        bad.free()
    good.free()


@pytest.mark.parametrize("label", S.ALL)
def test_argument_errors(curves, label):
    """MSMZ_ERR_ARG before any launch, outputs untouched; broadcast values >= q are MSMZ_ERR_RANGE with nothing launched"""
    from msm_zprize_amd._native import MsmzScalarRec
    curve, q = curves(label), S.order(label)
    n = 100
    sc = curve.Parallel.randomScalars(n, 2)
    pts = curve.Parallel.randomPointsFast(n, 2)
    before = curve.Scalar.toBigints(sc)
    lib = _lib()
    h = C.c_uint64(0)
    rec = MsmzScalarRec(sc.handle, 0, None, 0, 0, None, 0)
    assert lib.msmz_scalars_recurrence(curve._ctx, None, n, 0, C.byref(h), None) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_recurrence(curve._ctx, C.byref(rec), n, 0, None, None) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_inverse(curve._ctx, sc.handle, 0, n, 0, None, None) == MSMZ_ERR_ARG
    big = (1 << 64) - 1
    for a, b, cnt, flags, fa, fb, first_out, out in [
            (sc, None, 0, 0, 0, 0, 0, 0), (sc, sc, 1 << 32, 0, 0, 0, 0, 0),                    # n == 0, n >= 2^32
            (sc, sc, n, 4, 0, 0, 0, 0), (sc, None, n, 1 << 31, 0, 0, 0, 0),                    # unknown flag bits
            (None, None, n, 0, 0, 0, 0, 0),                                                    # nothing to do
            (Raw(0xDEAD), None, n, 0, 0, 0, 0, 0), (sc, 0xDEAD, n, 0, 0, 0, 0, 0), (sc, None, n, 0, 0, 0, 0, 0xDEAD),
            (Raw(pts.handle), None, n, 0, 0, 0, 0, 0), (5, pts.handle, n, 0, 0, 0, 0, 0), (sc, None, n, 0, 0, 0, 0, pts.handle),
            (sc, None, n, 0, 1, 0, 0, 0), (sc, None, 1, 0, n, 0, 0, 0), (sc, None, 2, 0, big, 0, 0, 0),   # beyond / wraps
            (None, sc, n, 0, 0, 1, 0, 0), (5, sc, 2, 0, 0, big, 0, 0), (sc, sc, n + 1, 0, 0, 0, 0, 0),
            (sc, None, 10, 0, 0, 0, 91, sc.handle), (sc, None, 2, 0, 0, 0, big, sc.handle),   # the destination range
            (sc, None, 10, 0, 0, 0, 1, 0)]:                                                    # first_out without a handle
        assert _rec(curve, a, b, cnt, flags, None, fa, fb, first_out, out) == (MSMZ_ERR_ARG, _handle(out), UNTOUCHED), \
            (cnt, flags, fa, fb, first_out)
    for x, cnt, first, first_out, out in [(sc, 0, 0, 0, 0), (sc, 1 << 32, 0, 0, 0), (0xDEAD, n, 0, 0, 0), (pts.handle, n, 0, 0, 0),
                                          (sc, n, 1, 0, 0), (sc, 2, big, 0, 0), (sc, n + 1, 0, 0, 0), (sc, 10, 0, 1, 0),
                                          (sc, 10, 0, 91, sc.handle), (sc, 10, 0, 0, pts.handle), (sc, 10, 0, 0, 0xDEAD),
                                          (sc, 10, 0, 5, sc.handle)]:
        assert _inv(curve, x, cnt, first, first_out, out) == (MSMZ_ERR_ARG, _handle(out), 1 << 40), (cnt, first, first_out)
    for bad in (q, q + 1, (1 << 256) - 1):   # broadcast values: the host refuses
        assert _rec(curve, bad, sc, n) == (MSMZ_ERR_RANGE, 0, UNTOUCHED)
        assert _rec(curve, bad, None, n) == (MSMZ_ERR_RANGE, 0, UNTOUCHED)
        assert _rec(curve, sc, None, n, 0, bad) == (MSMZ_ERR_RANGE, 0, UNTOUCHED)
        assert _rec(curve, 5, sc, n, 0, bad, 0, 0, 0, sc) == (MSMZ_ERR_RANGE, sc.handle, UNTOUCHED)
    assert curve.Scalar.toBigints(sc) == before   # (a refused in-place call launched nothing)
    _good_calls_are_correct(curve, q)
    with pytest.raises(ValueError):
        curve.Parallel.scalarRecurrence(q, sc)
    with pytest.raises(TypeError):
        curve.Parallel.prefixProducts(pts)
    with pytest.raises(TypeError):
        curve.Parallel.divideByLinear(sc, sc)
    with pytest.raises(ValueError):
        curve.Parallel.invertScalars(sc, 50, 0, sc, 10)
    sc.free(); pts.free()


# ---------------------------------------------------------------------------------------------- a KZG opening
@pytest.mark.parametrize("label", ["bls12-377", "bls12-381"])
def test_kzg_opening_on_the_device(curves, label):
    """SRS [tau^i] G from scalarPowers and mulPoints; (w, v) = divideByLinear(p, z); v == p(z) == <p, powers of z>; w ==
    synthetic division; C_p = msm(p, SRS), C_w = msm(w, SRS) over all n entries (the top entry of w is 0); with the
    oracle's group law on the host C_p - [v] G == [tau - z] C_w"""
    curve, params, q = curves(label), P.CURVES[label], S.order(label)
    par = curve.Parallel
    n = 2 * _geometry()[0] + 5
    rng = random.Random(50 + S.ALL.index(label))
    tau, z = rng.randrange(2, q), rng.randrange(2, q)
    G = CP.generator(params)
    taus = par.scalarPowers(tau, n)
    gens = par.pointsFromBigints([G] * n)
    srs = par.mulPoints(taus, gens, n)
    p = par.randomScalars(n, 77)
    pv = curve.Scalar.toBigints(p)
    w, v = par.divideByLinear(p, z)
    assert len(w) == n and w.kind == "scalars"
    assert v == sum(c * pow(z, i, q) for i, c in enumerate(pv)) % q
    zs = par.scalarPowers(z, n)
    assert v == par.innerProduct(p, zs)
    wv, value = U.synthetic_division(q, pv, z)
    assert value == v and wv[n - 1] == 0
    assert curve.Scalar.toBigints(w) == wv
    c_p = par.msm(p, srs, n)["result"]
    c_w = par.msm(w, srs, n)["result"]
    lhs = CP.add(params, c_p, CP.scale(params, (q - v) % q, G))
    rhs = CP.scale(params, (tau - z) % q, c_w)
    assert (lhs["x"], lhs["y"], bool(lhs["isZero"])) == (rhs["x"], rhs["y"], bool(rhs["isZero"]))
    assert not lhs["isZero"]
    for arr in (taus, gens, srs, p, w, zs):
        arr.free()


# ---------------------------------------------------------------------------------------------- a grand product
@pytest.mark.parametrize("label", ["pallas", "bls12-377"])
def test_grand_product_on_the_device(curves, label):
    """f random and non-zero, g a permutation of f: invertScalars(g), combineScalars with the resident coefficient
    (f . g^-1), exclusive prefixProducts.  Entry 0 is 1, every entry is the Python running product, last == 1; only the
    final column and `last` come down"""
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    n = _geometry()[0] + 3
    rng = random.Random(60 + S.ALL.index(label))
    fv = [rng.randrange(1, q) for _ in range(n)]
    gv = list(fv)
    rng.shuffle(gv)
    f, g = _upload(curve, fv), _upload(curve, gv)
    ginv, zeros = par.invertScalars(g)
    assert zeros == 0
    ratio = par.combineScalars(ginv, f)
    column, last = par.prefixProducts(ratio, exclusive=True)
    want, acc = [], 1
    for u, w in zip(fv, gv):
        want.append(acc)
        acc = acc * u * pow(w, -1, q) % q
    got = curve.Scalar.toBigints(column)
    assert got[0] == 1 and got == want
    assert last == 1 and acc == 1
    for arr in (f, g, ginv, ratio, column):
        arr.free()


# ---------------------------------------------------------------------------------------------- two engines
@pytest.mark.parametrize("label", S.ALL)
def test_two_engine_context(mod, curves, label):
    """devices = [0, 0], n = 2^16 + 257 (longer than one block): the inverse, into a new set and in place over the whole
    set, equals the single-engine result; the inverse with a non-zero first and every recurrence are
    MSMZ_ERR_UNSUPPORTED"""
    n = (1 << 16) + 257

    def run(curve):
        x = curve.Parallel.randomScalars(n, 81)
        st, h, nz = _inv(curve, x, n)
        assert st == 0
        outs = [_raw(curve, h, 0, n), nz]
        assert _lib().msmz_free(curve._ctx, h) == 0
        y = curve.Parallel.randomScalars(n, 82)
        calls = [_inv(curve, x, 10, 1), _inv(curve, x, 10, 0, 500, y), _inv(curve, y, 10, 0, 0, y)]
        calls += [_rec(curve, a, b, n, flags) for a, b in ((x, None), (None, x), (x, x), (5, x), (5, None)) for flags in (0, 3)]
        y.free()
        for st, h, _ in calls[:1] + calls[3:]:
            if st == 0:
                assert _lib().msmz_free(curve._ctx, h) == 0   # (a single engine takes these calls)
        assert _inv(curve, x, n, 0, 0, x)[:2] == (0, x.handle)
        outs.append(_raw(curve, x, 0, n))
        x.free()
        return outs, [c[0] for c in calls]

    want, ok = run(curves(label))
    assert ok == [0] * 13 and want[0] == want[2] and want[1] == 0
    mod.startThreads(devices=[0, 0])
    mparams = mod.curves.BY_LABEL[label]
    multi = (mod.Weierstrass if mparams["kind"] == "weierstrass" else mod.TwistedEdwards).create(mparams)
    try:
        got, refused = run(multi)
        assert got == want
        assert refused == [MSMZ_ERR_UNSUPPORTED] * 13
    finally:
        multi.close()
        mod.startThreads()

"""msmz_points_fixed_base on the GPU (k_fixed_table, k_fixed_mul; csrc/fixed_kernels.h): downloads against the oracle's
[s]B (tests/fixed_base_util.py) at the wave and block edges of the shared inversion, over every kind of base and forced
window widths; byte for byte against msmz_points_mul over n copies of B; the bit bound and its errors; the table cache,
filled, overfilled and reordered by a hit; an SRS end to end; multi-engine contexts; the argument errors."""
import ctypes as C
import random

import pytest

import check_points_util as U
import fixed_base_util as FB
import points_mul_util as M
from oracle import params as P

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
SIZES = [1, 63, 64, 65, 257, 4097]   # a partial wave, a full one, a wave plus a lane, blocks with a ragged tail


@pytest.fixture(scope="module")
def mod():
    import msm_zprize_amd as m
    m.startThreads()
    return m


def _create(mod, label):
    params = mod.curves.BY_LABEL[label]
    return (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)


@pytest.fixture(scope="module")
def curves(mod):
    cache = {}

    def get(label):
        if label not in cache:
            cache[label] = _create(mod, label)
        return cache[label]

    yield get
    for c in cache.values():
        c.close()


def _lib():
    from msm_zprize_amd._native import lib
    return lib()


def _xy(params, point):
    fb = params["fe_bytes"]
    if point["isZero"] and params["kind"] == "weierstrass":
        return bytes(2 * fb)
    return point["x"].to_bytes(fb, "little") + point["y"].to_bytes(fb, "little")


def _fixed(curve, scalars, n, base=0, index=0, xy=None, fs=0, bits=0, flags=0, h0=0):
    """msmz_points_fixed_base through the C ABI -> (status, *out_handle)"""
    from msm_zprize_amd._native import MsmzFixedBase
    f = MsmzFixedBase(base if isinstance(base, int) else base.handle, index, xy,
                      scalars if isinstance(scalars, int) else scalars.handle, fs, bits, flags)
    h = C.c_uint64(h0)
    st = _lib().msmz_points_fixed_base(curve._ctx, C.byref(f), n, C.byref(h))
    return st, h.value


def _window(curve, c):
    assert _lib().msmz_test_set_fixed_base_window(curve._ctx, c) == 0


def _built(curve):
    b = C.c_uint64()
    assert _lib().msmz_test_fixed_base_tables(curve._ctx, C.byref(b)) == 0
    return b.value


def _raw(curve, handle, first, count):
    """the bytes and flags msmz_download_points gives for records [first, first + count)"""
    fb = curve.fe_bytes
    data, inf = C.create_string_buffer(2 * fb * count), C.create_string_buffer(count)
    assert _lib().msmz_download_points(curve._ctx, handle, first, count, data, inf) == 0
    return data.raw, inf.raw


def _points(curve, handle, n):
    fb = curve.fe_bytes
    data, inf = _raw(curve, handle, 0, n)
    return [U.pt(int.from_bytes(data[2 * fb * i:2 * fb * i + fb], "little"),
                 int.from_bytes(data[2 * fb * i + fb:2 * fb * (i + 1)], "little"), inf[i] != 0) for i in range(n)]


def _free(curve, *handles):
    for h in handles:
        assert _lib().msmz_free(curve._ctx, h) == 0


def _assert_equal(params, got, want, what):
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad and len(got) == len(want), (what, bad[:3])


# ---------------------------------------------------------------------------------------------- parity with the oracle
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("label", FB.ALL)
def test_generator_multiples_equal_the_oracle(curves, label, n):
    """[s_i]G by the NULL route and the planner's width, records and infinity flags bit-exact: 0, 1, 2, q - 1, both sides
    of every window boundary and the carry chains in the first positions, then seeded random scalars"""
    curve, params = curves(label), P.CURVES[label]
    scalars = FB.gpu_scalars(params, n, 1000 * FB.ALL.index(label) + n)
    g = U.generator(params)
    sa = curve.Parallel.scalarsFromBigints(scalars)
    st, h = _fixed(curve, sa, n)
    assert st == 0 and h != 0
    _assert_equal(params, _points(curve, h, n), [FB.expected(label, s, g) for s in scalars], n)
    _free(curve, h)
    sa.free()


@pytest.mark.parametrize("c", [0, 4, 13, 16])
@pytest.mark.parametrize("label", FB.ALL)
def test_every_base_at_forced_widths(curves, label, c):
    """n = 257 under the planner's width (0) and forced 4, 13, 16; B = the generator as bytes, a random [k]G as host
    bytes and as a resident record at base_index > 0, every on-curve named point (small orders on the cofactor curves),
    a record flagged infinite, the twisted Edwards identity: all bit-exact, is_inf included"""
    curve, params = curves(label), P.CURVES[label]
    n = 257
    rng = random.Random(7 * FB.ALL.index(label) + c)
    scalars = FB.gpu_scalars(params, n, 31 + c)
    sa = curve.Parallel.scalarsFromBigints(scalars)
    named = FB.bases(label, rng)
    resident = curve.Parallel.pointsFromBigints([U.generator(params)] + [b for _, b in named])
    _window(curve, c)
    try:
        for k, (name, b) in enumerate(named):
            want = [FB.expected(label, s, b) for s in scalars]
            routes = [("resident", dict(base=resident, index=k + 1))]
            if not (b["isZero"] and params["kind"] != "weierstrass"):
                routes.append(("bytes", dict(xy=_xy(params, b))))
            for route, args in routes:
                st, h = _fixed(curve, sa, n, **args)
                assert st == 0, (name, route, st)
                _assert_equal(params, _points(curve, h, n), want, (name, route))
                _free(curve, h)
    finally:
        _window(curve, 0)
    resident.free(); sa.free()


# ---------------------------------------------------------------------------------------------- against points_mul
@pytest.mark.parametrize("label", FB.ALL)
def test_bytes_equal_points_mul_over_copies(curves, label):
    """msmz_points_mul over n copies of B and the same scalars leaves the same set: the base points and (Weierstrass) the
    endomorphism images behind them download to the same bytes, and one MSM over each against random scalars agrees, GLV
    on and off -- for a random B, a small-order B where the curve has one, and B at infinity"""
    from msm_zprize_amd._native import MsmzMul
    curve, params = curves(label), P.CURVES[label]
    n = 257
    weier = params["kind"] == "weierstrass"
    rng = random.Random(FB.ALL.index(label))
    scalars = FB.gpu_scalars(params, n, 77)
    sa = curve.Parallel.scalarsFromBigints(scalars)
    t = curve.Parallel.randomScalars(n, 78)
    named = FB.bases(label, rng)[1:]
    for name, b in named:
        copies = curve.Parallel.pointsFromBigints([b] * n)
        m = MsmzMul(copies.handle, 0, sa.handle, 0, None, 0, 0)
        hm = C.c_uint64(0)
        assert _lib().msmz_points_mul(curve._ctx, C.byref(m), n, C.byref(hm)) == 0
        st, hf = _fixed(curve, sa, n, base=copies, index=n - 1)
        assert st == 0
        total = 2 * n if weier else n
        assert _raw(curve, hf, 0, total) == _raw(curve, hm.value, 0, total), name
        from msm_zprize_amd.parallel import DeviceArray
        a, bb = DeviceArray(curve, hf, n, "points"), DeviceArray(curve, hm.value, n, "points")
        for glv in ((0, 1) if weier else (0,)):
            ra = curve.Parallel.msm(t, a, n, False, {"glv": glv})["result"]
            rb = curve.Parallel.msm(t, bb, n, False, {"glv": glv})["result"]
            assert (ra["x"], ra["y"], bool(ra["isZero"])) == (rb["x"], rb["y"], bool(rb["isZero"])), (name, glv)
        a.free(); bb.free(); copies.free()
    sa.free(); t.free()


# ---------------------------------------------------------------------------------------------- scalar_bits
@pytest.mark.parametrize("label", FB.ALL)
def test_scalar_bits(curves, label):
    """bounds 1, 64, 128 and >= the bit length of q give the bytes of the call without a bound; one scalar at 2^b inside
    the range is MSMZ_ERR_RANGE with *out_handle untouched and the next call fine; outside the range it is not read; a
    resident scalar >= q (planted as tests/test_points_mul_gpu.py plants it) is MSMZ_ERR_RANGE too"""
    from msm_zprize_amd._native import MsmzSrc
    from msm_zprize_amd.parallel import DeviceArray
    curve, params = curves(label), P.CURVES[label]
    q, n = params["order"], 257
    rng = random.Random(11)
    for b in (1, 64, 128):
        vals = [0, 1, (1 << b) - 1] + [rng.randrange(1 << b) for _ in range(n - 3)]
        sa = curve.Parallel.scalarsFromBigints(vals)
        st, h0 = _fixed(curve, sa, n)
        assert st == 0
        want = _raw(curve, h0, 0, n)
        for bits in (b, 256, FB.order_bits(params), FB.order_bits(params) + 1):
            st, h = _fixed(curve, sa, n, bits=bits)
            assert st == 0, bits
            assert _raw(curve, h, 0, n) == want, (b, bits)
            _free(curve, h)
        _free(curve, h0)
        sa.free()
        # the scalar 2^b at index 200: inside [0, 257) it breaks the bound, the ranges clear of it do not read it
        vals[200] = 1 << b
        sa = curve.Parallel.scalarsFromBigints(vals)
        assert _fixed(curve, sa, n, bits=b, h0=99) == (MSMZ_ERR_RANGE, 99)
        for cnt, fs in ((200, 0), (56, 201)):
            st, h = _fixed(curve, sa, cnt, fs=fs, bits=b)
            assert st == 0 and h != 0
            fb = curve.fe_bytes
            assert _raw(curve, h, 0, cnt)[0] == want[0][2 * fb * fs:2 * fb * (fs + cnt)]
            _free(curve, h)
        st, h = _fixed(curve, sa, n)   # without the bound the same set is fine
        assert st == 0
        _free(curve, h)
        sa.free()
    # a resident value >= q: msmz_import_scalars_into converts before it reports, so the refused value stays resident
    h = C.c_uint64()
    assert _lib().msmz_alloc_scalars(curve._ctx, n, C.byref(h)) == 0
    sc = DeviceArray(curve, h.value, n, "scalars")
    good = M.encode_scalars([rng.randrange(q) for _ in range(n)])
    src = MsmzSrc(C.cast(C.c_char_p(good), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, sc.handle, 0, C.byref(src), n) == 0
    raw = M.encode_scalars([q])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, sc.handle, 200, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert curve.Scalar.toBigints(sc, 200, 1) == [q]
    assert _fixed(curve, sc, n, h0=5) == (MSMZ_ERR_RANGE, 5)
    for cnt, fs in ((50, 201), (200, 0)):
        st, hh = _fixed(curve, sc, cnt, fs=fs)
        assert st == 0 and hh != 0
        _free(curve, hh)
    sc.free()


# ---------------------------------------------------------------------------------------------- the table cache
@pytest.mark.parametrize("label", ["pallas", "ed-on-bls12-377"])
def test_tables_are_cached(mod, label):
    """two calls on one base build one table, another base a second one, the generator by either route one more; freeing
    the handle a resident base came from changes nothing"""
    curve, params = _create(mod, label), P.CURVES[label]
    try:
        n = 65
        rng = random.Random(3)
        scalars = [rng.randrange(params["order"]) for _ in range(n)]
        sa = curve.Parallel.scalarsFromBigints(scalars)
        g = U.generator(params)
        b1, b2 = (U.scale(params, rng.randrange(1, params["order"]), g) for _ in range(2))
        src = curve.Parallel.pointsFromBigints([g, b1])
        assert _built(curve) == 0
        st, h1 = _fixed(curve, sa, n, base=src, index=1)
        assert st == 0 and _built(curve) == 1
        st, h2 = _fixed(curve, sa, n, base=src, index=1)
        assert st == 0 and _built(curve) == 1
        src.free()
        st, h3 = _fixed(curve, sa, n, xy=_xy(params, b1))   # the same base by its bytes: the same table
        assert st == 0 and _built(curve) == 1
        want = [FB.expected(label, s, b1) for s in scalars]
        for h in (h1, h2, h3):
            _assert_equal(params, _points(curve, h, n), want, "b1")
        st, h4 = _fixed(curve, sa, n, xy=_xy(params, b2))
        assert st == 0 and _built(curve) == 2
        _assert_equal(params, _points(curve, h4, n), [FB.expected(label, s, b2) for s in scalars], "b2")
        st, h5 = _fixed(curve, sa, n)
        assert st == 0 and _built(curve) == 3
        st, h6 = _fixed(curve, sa, n, xy=_xy(params, g))
        assert st == 0 and _built(curve) == 3
        assert _raw(curve, h5, 0, n) == _raw(curve, h6, 0, n)
        _free(curve, h1, h2, h3, h4, h5, h6)
        sa.free()
    finally:
        curve.close()


def _cache_tables():
    """the tables an engine keeps, from msmz_test_cache_geometry"""
    t = C.c_uint32(0)
    _lib().msmz_test_cache_geometry(None, C.byref(t), None)
    return t.value


@pytest.mark.parametrize("label", ["pallas", "ed-on-bls12-377"])
def test_table_cache_evicts_the_one_unused_longest(mod, label):
    """fixed_tables + 1 bases at n = 65 on a context of its own.  With four tables: build A, B, C, D; hit A; build E.  Then
    A is still cached (built unchanged) and B is not (built + 1, which makes C the table that leaves): D is served from
    the cache and C is built again.  Every result against the oracle's [s]B, so a table freed under a call, or the table
    of another base handed out, shows as wrong points.  Then the same sequence under a forced window width: an equal
    base under another width is another key, so every first use builds although the planner's tables are cached"""
    T = _cache_tables()
    assert T >= 3
    curve, params = _create(mod, label), P.CURVES[label]
    try:
        n = 65
        rng = random.Random(17 + FB.ALL.index(label))
        scalars = FB.gpu_scalars(params, n, 5)
        sa = curve.Parallel.scalarsFromBigints(scalars)
        g = U.generator(params)
        bases = [U.scale(params, rng.randrange(2, params["order"]), g) for _ in range(T + 1)]
        assert len({(b["x"], b["y"]) for b in bases}) == T + 1
        want = [[FB.expected(label, s, b) for s in scalars] for b in bases]

        def use(k, builds, what):
            before = _built(curve)
            st, h = _fixed(curve, sa, n, xy=_xy(params, bases[k]))
            assert st == 0 and h != 0, (what, k)
            assert _built(curve) - before == builds, (what, k, "built")
            _assert_equal(params, _points(curve, h, n), want[k], (what, k))
            _free(curve, h)

        cc, K, entries = C.c_int32(), C.c_int32(), C.c_uint64()
        assert _lib().msmz_test_fixed_base_plan(params["curve_id"], n, 0, C.byref(cc), C.byref(K), C.byref(entries)) == 0
        forced = 4 if cc.value != 4 else 5
        assert _built(curve) == 0
        for width in (0, forced):
            _window(curve, width)
            for k in range(T):
                use(k, 1, (width, "fill"))
            use(0, 0, (width, "hit the oldest"))
            use(T, 1, (width, "overflow"))          # the oldest not hit, bases[1], leaves
            use(0, 0, (width, "hit before the overflow: kept"))
            use(1, 1, (width, "the oldest not hit: gone"))   # bases[2] leaves
            use(3, 0, (width, "still cached"))
            use(2, 1, (width, "left with the rebuild"))
        assert _built(curve) == 2 * (T + 3)
        _window(curve, 0)
        sa.free()
    finally:
        curve.close()


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("label", FB.ALL)
def test_srs_end_to_end(curves, label):
    """scalarPowers(tau, 300) -> fixedBaseMul -> msm(p, SRS) == [p(tau)]G with p(tau) from Python integers; checkPoints
    finds every point of the SRS on the curve and in the subgroup"""
    curve, params = curves(label), P.CURVES[label]
    q, n = params["order"], 300
    rng = random.Random(41 + FB.ALL.index(label))
    tau = rng.randrange(2, q)
    powers = curve.Parallel.scalarPowers(tau, n)
    srs = curve.Parallel.fixedBaseMul(powers)
    assert len(srs) == n and srs.kind == "points"
    coeffs = [rng.randrange(q) for _ in range(n)]
    p_tau = sum(c * pow(tau, i, q) for i, c in enumerate(coeffs)) % q
    pa = curve.Parallel.scalarsFromBigints(coeffs)
    got = curve.Parallel.msm(pa, srs, n)["result"]
    want = FB.expected(label, p_tau, U.generator(params))
    assert M.canon(params, U.pt(got["x"], got["y"], bool(got["isZero"]))) == want
    res = curve.Parallel.checkPoints(srs)
    assert res.ok and res.offCurve == 0 and res.offSubgroup == 0
    # the Python surface: an affine base, a resident base, a range and a bound
    g = U.generator(params)
    b = U.scale(params, 12345, g)
    src = curve.Parallel.pointsFromBigints([g, b])
    small = curve.Parallel.scalarsFromBigints([5, 0, (1 << 64) - 1, 7])
    for base in (b, (src, 1)):
        out = curve.Parallel.fixedBaseMul(small, base, 2, firstScalar=1, scalarBits=64)
        _assert_equal(params, _points(curve, out.handle, 2), [FB.expected(label, s, b) for s in (0, (1 << 64) - 1)], "surface")
        out.free()
    with pytest.raises(Exception):
        curve.Parallel.fixedBaseMul(small, b, scalarBits=8)   # 2^64 - 1 breaks an 8-bit bound
    for a in (powers, srs, pa, src, small):
        a.free()


# ---------------------------------------------------------------------------------------------- multi-engine contexts
@pytest.mark.parametrize("engines", [1, 2, 8])
def test_multi_engine_context(mod, curves, engines):
    """1, 2 and 8 engines on one GPU, n = 2^16 + 5 (two blocks of the deal): the downloaded bytes equal the single-engine
    handle's for the generator, host bytes and a resident base in the second block; first_s != 0 is refused"""
    label = "pallas"
    params = P.CURVES[label]
    n = (1 << 16) + 5
    b = U.scale(params, 987654321, U.generator(params))

    def run(curve):
        sc = curve.Parallel.randomScalars(n, 61)
        pts = curve.Parallel.randomPointsFast(n, 62)
        outs = []
        for args in (dict(), dict(xy=_xy(params, b)), dict(base=pts, index=n - 2)):
            st, h = _fixed(curve, sc, n, **args)
            assert st == 0, (args.keys(), st)
            outs.append(_raw(curve, h, 0, n))
            _free(curve, h)
        refused = _fixed(curve, sc, 10, fs=1)
        sc.free(); pts.free()
        return outs, refused

    want, ok = run(curves(label))
    assert ok[0] == 0
    _free(curves(label), ok[1])
    assert want[0] != want[1] and want[1] != want[2] and any(want[0][0])
    mod.startThreads(devices=[0] * engines)
    multi = _create(mod, label)
    try:
        got, refused = run(multi)
        assert got == want
        if engines > 1:
            assert refused == (MSMZ_ERR_UNSUPPORTED, 0)
        else:
            assert refused[0] == 0
    finally:
        multi.close()
        mod.startThreads()


# ---------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("label", FB.ALL)
def test_argument_errors(curves, label):
    from msm_zprize_amd._native import MsmzFixedBase
    curve, params = curves(label), P.CURVES[label]
    n = 300
    pts = curve.Parallel.randomPointsFast(n, 2)
    sc = curve.Parallel.randomScalars(n, 2)
    f = _lib().msmz_points_fixed_base
    h = C.c_uint64(0)
    ok = MsmzFixedBase(0, 0, None, sc.handle, 0, 0, 0)
    assert f(None, C.byref(ok), n, C.byref(h)) == MSMZ_ERR_ARG
    assert f(curve._ctx, None, n, C.byref(h)) == MSMZ_ERR_ARG
    assert f(curve._ctx, C.byref(ok), n, None) == MSMZ_ERR_ARG
    g = _xy(params, U.generator(params))
    p = params["modulus"]
    fb = params["fe_bytes"]
    cases = [
        dict(n=0), dict(n=1 << 30),                                  # n == 0, n beyond the record-index limit
        dict(scalars=0xDEAD), dict(scalars=pts.handle),              # unknown scalar handle, one of the wrong kind
        dict(base=0xDEAD), dict(base=sc.handle),                     # the same for the base
        dict(fs=1), dict(n=2, fs=(1 << 64) - 1), dict(n=1, fs=n),    # scalar ranges beyond the set
        dict(base=pts, index=n), dict(base=pts, index=(1 << 64) - 1),  # base_index beyond the base points
        dict(index=1),                                               # an index without a handle
        dict(base=pts, xy=g),                                        # both routes
        dict(flags=1), dict(bits=-1), dict(bits=257),
    ]
    for kw in cases:
        args = dict(scalars=sc, n=n)
        args.update(kw)
        scalars, cnt = args.pop("scalars"), args.pop("n")
        assert _fixed(curve, scalars, cnt, h0=3, **args) == (MSMZ_ERR_ARG, 3), kw
    for bad in (p.to_bytes(fb, "little") + g[fb:], g[:fb] + ((1 << (8 * fb)) - 1).to_bytes(fb, "little")):
        assert _fixed(curve, sc, n, xy=bad, h0=3) == (MSMZ_ERR_RANGE, 3)
    if params["kind"] == "weierstrass":
        pre = curve.Parallel.precomputePoints(pts, n, {"c": 8}, 2)
        assert _fixed(curve, sc, n, base=pre.handle, h0=3) == (MSMZ_ERR_UNSUPPORTED, 3)
        pre.free()
        assert _fixed(curve, sc, n, base=pts, index=n, h0=3) == (MSMZ_ERR_ARG, 3)   # an endomorphism image is no base point
    assert _lib().msmz_test_set_fixed_base_window(curve._ctx, 3) == MSMZ_ERR_ARG
    assert _lib().msmz_test_set_fixed_base_window(curve._ctx, 17) == MSMZ_ERR_ARG
    st, hh = _fixed(curve, sc, n)   # the context is as usable as before
    assert st == 0
    s = curve.Scalar.toBigints(sc, 0, 2)
    _assert_equal(params, _points(curve, hh, 2), [FB.expected(label, v, U.generator(params)) for v in s], "after errors")
    _free(curve, hh)
    pts.free(); sc.free()

"""The scalar bit bound (msmz_opts.reserved[1], `scalarBits`): "every scalar of this call is below 2^bits".  Every result
is compared bit-exactly against the C oracle and against the same call without the bound; the log's window count is the
bounded one (the assertion that needs the feature); a scalar at 2^bits fails the call with MSMZ_ERR_RANGE, in normal
time, and leaves the context usable."""
import ctypes as C
import random

import pytest

from oracle import c_oracle
from oracle import params as P

pytestmark = pytest.mark.gpu

ALL = ["bls12-377", "pallas", "bls12-381", "ed-on-bls12-377"]
WEIER = ALL[:3]
MSMZ_ERR_ARG, MSMZ_ERR_RANGE = 1, 6
GLV_HALF = 127   # the half length the windows of a GLV MSM are sized for (constants_gen.h GLV_BITS - 1)
TILE = 2048      # scalars per sort tile (1024 with GLV)


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


def _strip(p):
    return {"x": p["x"], "y": p["y"], "isZero": bool(p.get("isZero", False))}


def _enc(scalars):
    return b"".join(int(s).to_bytes(32, "little") for s in scalars)


def _bits(label):
    return P.CURVES[label]["order"].bit_length()


def _scalars(label, bound, n, seed):
    """random below min(q, 2^bound); 0, 1, the largest admissible scalar (all windows all-ones: the carry reaches the top)
    and 2^(bound-1) on the first and last lanes of the sort tiles"""
    q = P.CURVES[label]["order"]
    top = min(q, 1 << bound)
    rng = random.Random(seed)
    s = [rng.randrange(top) for _ in range(n)]
    special = [top - 1, min(top - 1, 1 << (bound - 1)), 0, 1]
    lanes = [0, 1, 1023, 1024, TILE - 1, TILE, 2 * TILE - 1, n - 2, n - 1]
    for j, i in enumerate(i for i in lanes if 0 <= i < n):
        s[i] = special[j % 4]
    if n >= 4:
        s[n - 1], s[0] = top - 1, top - 1
    return s


def _windows(label, bound, stats, retried=False):
    """the window count the planner gives the bound for the c and the GLV choice that ran"""
    b = min(bound, _bits(label)) if bound else _bits(label)
    if stats.glv:
        b = min(b, GLV_HALF)
        if retried:
            return None
    return -(-(b + 1) // stats.c)


def _run(curve, fn, scalars, pts, n, opts):
    if fn == "msmProjective":
        r = curve.Parallel.msmProjective(scalars, pts, n, {k: v for k, v in opts.items() if k != "glv"})
    else:
        r = getattr(curve.Parallel, fn)(scalars, pts, n, False, dict(opts))
    return _strip(r["result"]), r["stats"]


def _functions(label):
    return ["msmUnsafe", "msm", "msmProjective"]   # (twisted Edwards: all three take the extended-coordinate path)


@pytest.mark.parametrize("n", [1, 3, 257, 4096, 1 << 16])
@pytest.mark.parametrize("label", ALL)
def test_bounded_matches_oracle_and_unbounded(curves, mod, label, n):
    """4 curves x 8 bounds x 5 sizes x {msmUnsafe, msm, msmProjective} x GLV {0, 1, -1}: result == oracle == bound 0, and
    log.K is the bounded window count"""
    from msm_zprize_amd._native import lib
    curve = curves(label)
    weier = label in WEIER
    pts = curve.Parallel.randomPointsFast(n, 77 + n)
    pb = curve.Affine.toBigints(pts)
    for bound in (1, 8, 32, 33, 64, 128, 200, _bits(label)):
        s = _scalars(label, bound, n, 1000 * bound + n)
        want = _strip(c_oracle.msm(P.CURVES[label], s, pb))
        host = _enc(s)
        res = curve.Parallel.scalarsFromBytes(host, n)
        for fn in _functions(label):
            for glv in ((0, 1, -1) if weier and fn != "msmProjective" else (0,)):
                for sc in (host, res):
                    before = lib().msmz_test_retries(curve._ctx)
                    got, st = _run(curve, fn, sc, pts, n, {"glv": glv, "scalarBits": bound})
                    retried = lib().msmz_test_retries(curve._ctx) != before
                    assert got == want, (bound, fn, glv)
                    k = _windows(label, bound, st, retried)
                    assert k is None or st.K == k, (bound, fn, glv, st.K, st.c, st.glv)
                    if glv == -1 and bound <= GLV_HALF:
                        assert st.glv == 0, (bound, fn)   # the split would only double the point set
                plain, st0 = _run(curve, fn, res, pts, n, {"glv": glv})
                assert plain == want, (bound, fn, glv)
                assert st0.K == _windows(label, 0, st0), (fn, glv)
        res.free()
    pts.free()


# (bound, c, what the planner makes of it: tests/native/scalar_bits_test.cpp prints the two BLS12-377 shapes)
USER_C = [(8, 9, "K = 1"), (8, 17, "K = 1"), (1, 2, "K = 1"), (16, 17, "K = 1"), (64, 7, "top window folds"),
          (64, 17, "top window spreads over 4 sub-windows"), (128, 16, "1-bit top window"), (33, 17, "K = 2, exact"),
          (64, 22, "fallback sort"), (200, 24, "fallback sort"), (32, 3, "many windows"), (100, 13, "")]


@pytest.mark.parametrize("bound,c,what", USER_C)
@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_bounded_user_window(curves, label, bound, c, what):
    from msm_zprize_amd._native import lib
    curve = curves(label)
    for n in (5, 4096 + 37):
        pts = curve.Parallel.randomPointsFast(n, 5)
        pb = curve.Affine.toBigints(pts)
        s = _scalars(label, bound, n, bound * 31 + c)
        want = _strip(c_oracle.msm(P.CURVES[label], s, pb))
        for fn in ("msmUnsafe", "msm", "msmProjective"):
            for glv in ((0, 1) if fn != "msmProjective" else (0,)):
                before = lib().msmz_test_retries(curve._ctx)
                got, st = _run(curve, fn, _enc(s), pts, n, {"glv": glv, "c": c, "scalarBits": bound})
                assert got == want, (fn, glv, n, what)
                if lib().msmz_test_retries(curve._ctx) == before:   # (a redo runs the windows of the proven half length)
                    assert st.c == c and st.K == -(-(min(bound, GLV_HALF if st.glv else 256) + 1) // c), (fn, glv, n, st.K)
                assert _run(curve, fn, _enc(s), pts, n, {"glv": glv, "c": c})[0] == want
        got, st = _run(curve, "msmUnsafe", _enc(s), pts, n, {"glv": 0, "c": c, "scalarBits": bound, "reduceAffine": 1})
        assert got == want and st.K == -(-(bound + 1) // c), what
        pts.free()


@pytest.mark.parametrize("c", [7, 17])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_scalar_at_the_bound_is_a_range_error(curves, mod, c, where):
    """BLS12-377, bound 64: c = 7 folds the top window, c = 17 spreads it.  One scalar equal to 2^64 among valid ones:
    MSMZ_ERR_RANGE on the host and the resident route, single and batched, and the next valid MSM is correct"""
    curve = curves("bls12-377")
    bound, n, B = 64, 5000, 3
    rng = random.Random(c)
    pts = curve.Parallel.randomPointsFast(n, 21)
    pb = curve.Affine.toBigints(pts)
    vecs = [[rng.randrange(1 << bound) for _ in range(n)] for _ in range(B)]
    want = [_strip(c_oracle.msm(P.BLS12_377, v, pb)) for v in vecs]
    at = {"first": 0, "middle": 2048 + 517, "last": n - 1}[where]
    opts = {"glv": 0, "c": c, "scalarBits": bound}
    for k in (0, B - 1):
        bad = [list(v) for v in vecs]
        bad[k][at] = 1 << bound
        host = [_enc(v) for v in bad]
        res = curve.Parallel.scalarsFromBytes(host[k], n)
        res_all = curve.Parallel.scalarsFromBytes(b"".join(host), B * n)
        for call in (lambda: curve.Parallel.msm(host[k], pts, n, False, opts),
                     lambda: curve.Parallel.msmUnsafe(res, pts, n, False, opts),
                     lambda: curve.Parallel.msmBatch(host, pts, n, opts),
                     lambda: curve.Parallel.msmBatchUnsafe(res_all, pts, n, opts)):
            with pytest.raises(mod._native.MsmzError) as e:
                call()
            assert e.value.status == MSMZ_ERR_RANGE
            # the context stays usable, and the same scalars pass without the bound (2^64 is below q)
            assert _run(curve, "msm", _enc(vecs[0]), pts, n, opts)[0] == want[0]
        assert [_strip(r) for r in curve.Parallel.msmBatch([_enc(v) for v in vecs], pts, n, opts)] == want
        res.free()
        res_all.free()
    pts.free()


def test_bad_bounds_are_argument_errors(curves):
    from msm_zprize_amd._native import MsmzLog, MsmzOpts, lib
    curve = curves("pallas")
    pts = curve.Parallel.randomPointsFast(8, 1)
    sc = curve.Parallel.randomScalars(16, 1)
    out = C.create_string_buffer(64 * 2)
    inf = (C.c_int * 2)()
    s = b"\x01" + b"\x00" * 31
    L = lib()
    for bad in (-1, 257, 1 << 30):
        o = MsmzOpts()
        o.reserved[1] = bad
        assert L.msmz_msm(curve._ctx, pts.handle, s * 8, 8, C.byref(o), out, inf, None) == MSMZ_ERR_ARG
        assert L.msmz_msm_resident(curve._ctx, pts.handle, sc.handle, 8, C.byref(o), out, inf, None) == MSMZ_ERR_ARG
        assert L.msmz_msm_batch(curve._ctx, pts.handle, s * 16, 8, 2, C.byref(o), out, inf, None) == MSMZ_ERR_ARG
        assert L.msmz_msm_batch_resident(curve._ctx, pts.handle, sc.handle, 8, 2, C.byref(o), out, inf, None) == MSMZ_ERR_ARG
        h = C.c_uint64()
        assert L.msmz_precompute_points(curve._ctx, pts.handle, 8, C.byref(o), 0, C.byref(h)) == MSMZ_ERR_ARG
    for ok in (0, 255, 256):
        o = MsmzOpts()
        o.reserved[1] = ok
        log = MsmzLog()
        assert L.msmz_msm(curve._ctx, pts.handle, s * 8, 8, C.byref(o), out, inf, C.byref(log)) == 0
        assert log.K == -(-(255 + 1) // log.c) if not log.glv else True


@pytest.mark.parametrize("B", [1, 4, 16])
@pytest.mark.parametrize("label", WEIER)
def test_bounded_batch_equals_single_calls(curves, label, B):
    curve = curves(label)
    n = 3000
    pts = curve.Parallel.randomPointsFast(n, 3)
    pb = curve.Affine.toBigints(pts)
    for bound in (33, 64, 128):
        vecs = [_scalars(label, bound, n, 100 * B + k) for k in range(B)]
        want = [_strip(c_oracle.msm(P.CURVES[label], v, pb)) for v in vecs]
        host = [_enc(v) for v in vecs]
        res = curve.Parallel.scalarsFromBytes(b"".join(host), B * n)
        for glv in (0, 1, -1):
            o = {"glv": glv, "scalarBits": bound}
            single = [_run(curve, "msm", h, pts, n, o)[0] for h in host]
            assert single == want
            assert [_strip(r) for r in curve.Parallel.msmBatch(host, pts, n, o)] == single, (bound, glv)
            log = curve.Parallel.lastBatchLog
            if not log.glv:
                assert log.K == -(-(bound + 1) // log.c), (bound, glv)
            assert [_strip(r) for r in curve.Parallel.msmBatchUnsafe(res, pts, n, o)] == single, (bound, glv)
            assert [_strip(r) for r in curve.Parallel.msmBatch(host, pts, n, {"glv": glv})] == single
        res.free()
    pts.free()


@pytest.mark.parametrize("factor", [0, 2])
@pytest.mark.parametrize("label", WEIER)
def test_bounded_precomputed_set(curves, mod, label, factor):
    """copies for the bounded window count: fewer records, the handle reports the bound, results equal the plain handle's,
    a different bound is refused"""
    from msm_zprize_amd._native import lib
    curve = curves(label)
    n, bound = 3000, 64
    pts = curve.Parallel.randomPointsFast(n, 17)
    pb = curve.Affine.toBigints(pts)
    vecs = [_scalars(label, bound, n, 9 + k) for k in range(3)]
    want = [_strip(c_oracle.msm(P.CURVES[label], v, pb)) for v in vecs]
    for glv in (0, 1):
        full = curve.Parallel.precomputePoints(pts, n, {"glv": glv}, factor)
        pre = curve.Parallel.precomputePoints(pts, n, {"glv": glv, "scalarBits": bound, "c": full.info["c"]}, factor)
        info = pre.info
        assert full.info["scalarBits"] == 0 and info["scalarBits"] == bound
        b = min(bound, GLV_HALF) if glv else bound
        assert info["K"] == -(-(b + 1) // info["c"]) and info["K"] < full.info["K"]
        bits = C.c_int32(-1)
        assert lib().msmz_precomputed_scalar_bits(curve._ctx, pre.handle, C.byref(bits)) == 0 and bits.value == bound
        assert lib().msmz_precomputed_scalar_bits(curve._ctx, pts.handle, C.byref(bits)) == MSMZ_ERR_ARG
        if factor == 0 and not glv:
            assert info["factor"] == info["K"] and info["records"] == info["K"] * n < full.info["records"]
        for o in ({}, {"scalarBits": bound}):
            for v, w in zip(vecs, want):
                got, st = _run(curve, "msm", _enc(v), pre, n, o)
                assert got == w and (st.K == info["K"] or st.glv), (glv, o)
            assert [_strip(r) for r in curve.Parallel.msmBatchUnsafe([_enc(v) for v in vecs], pre, n, o)] == want
        assert _run(curve, "msm", _enc(vecs[0]), pts, n, {"glv": glv, "scalarBits": bound})[0] == want[0]
        for o in ({"scalarBits": bound + 1}, {"scalarBits": 8}):
            with pytest.raises(mod._native.MsmzError) as e:
                curve.Parallel.msm(_enc(vecs[0]), pre, n, False, o)
            assert e.value.status == MSMZ_ERR_ARG
        with pytest.raises(mod._native.MsmzError) as e:   # the plain handle has no bound: none but 0 fits it
            curve.Parallel.msm(_enc(vecs[0]), full, n, False, {"scalarBits": bound})
        assert e.value.status == MSMZ_ERR_ARG
        # a scalar above the handle's bound, with the bound left to the handle
        bad = list(vecs[0])
        bad[n // 2] = 1 << bound
        with pytest.raises(mod._native.MsmzError) as e:
            curve.Parallel.msm(_enc(bad), pre, n)
        assert e.value.status == MSMZ_ERR_RANGE
        assert _run(curve, "msm", _enc(vecs[1]), pre, n, {})[0] == want[1]
        pre.free()
        full.free()
    pts.free()


@pytest.mark.parametrize("label", WEIER)
def test_bounded_glv_redo(curves, label):
    """the assumed GLV half length lowered below the bound: the first attempt's windows do not hold the halves, k_hist
    flags it, and the redo with the proven length equals the oracle"""
    from msm_zprize_amd._native import lib
    curve = curves(label)
    n, bound = 2500, 64
    pts = curve.Parallel.randomPointsFast(n, 4)
    pb = curve.Affine.toBigints(pts)
    s = _scalars(label, bound, n, 3)
    want = _strip(c_oracle.msm(P.CURVES[label], s, pb))
    L = lib()
    before = L.msmz_test_retries(curve._ctx)
    assert L.msmz_test_set_glv_bits(curve._ctx, 40) == 0
    try:
        for c in (0, 7, 13):
            assert _run(curve, "msm", _enc(s), pts, n, {"glv": 1, "c": c, "scalarBits": bound})[0] == want, c
        assert [_strip(r) for r in curve.Parallel.msmBatch([_enc(s)] * 2, pts, n, {"glv": 1, "scalarBits": bound})] == [want] * 2
    finally:
        assert L.msmz_test_set_glv_bits(curve._ctx, 0) == 0
    assert L.msmz_test_retries(curve._ctx) >= before + 4
    pts.free()


def test_bounded_two_engines_on_one_gpu(mod):
    n, bound = (1 << 17) + 999, 64
    mod.startThreads(devices=[0, 0])
    multi = mod.Weierstrass.create(mod.curves.bls12377Params)
    try:
        pts = multi.Parallel.randomPointsFast(n, 4)
        pb = multi.Affine.toBigints(pts)
        vecs = [_scalars("bls12-377", bound, n, k) for k in range(2)]
        want = [_strip(c_oracle.msm(P.BLS12_377, v, pb)) for v in vecs]
        for glv in (0, 1, -1):
            o = {"glv": glv, "scalarBits": bound}
            got, st = _run(multi, "msmUnsafe", _enc(vecs[0]), pts, n, o)
            assert got == want[0] and (st.glv or st.K == -(-(bound + 1) // st.c))
            res = multi.Parallel.scalarsFromBytes(_enc(vecs[0]), n)
            assert _run(multi, "msm", res, pts, n, o)[0] == want[0]
            res.free()
            assert [_strip(r) for r in multi.Parallel.msmBatch([_enc(v) for v in vecs], pts, n, o)] == want
        bad = list(vecs[0])
        bad[(1 << 16) + 5] = 1 << bound   # on the second engine's share
        with pytest.raises(mod._native.MsmzError) as e:
            multi.Parallel.msm(_enc(bad), pts, n, False, {"glv": 0, "scalarBits": bound})
        assert e.value.status == MSMZ_ERR_RANGE
        assert _run(multi, "msm", _enc(vecs[1]), pts, n, {"glv": 0, "scalarBits": bound})[0] == want[1]
    finally:
        multi.close()
        mod.startThreads()

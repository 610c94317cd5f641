"""Precomputed point sets (msmz_precompute_points): shifted copies 2^(c j) P_i of a resident set, so that F windows share
one bucket set.  Every MSM result is compared bit-exactly against the C oracle and against the same MSM over the plain
handle; the copies themselves are checked record by record against c_oracle.scale."""
import ctypes as C
import random

import pytest

from oracle import c_oracle
from oracle import params as P
from oracle import prng

pytestmark = pytest.mark.gpu

WEIER = ["bls12-377", "pallas", "bls12-381"]
MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6


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


def _msm(curve, scalars, pts, n, opts, safe):
    f = curve.Parallel.msm if safe else curve.Parallel.msmUnsafe
    return _strip(f(scalars, pts, n, False, dict(opts))["result"])


@pytest.mark.parametrize("n", [1, 5, 257, 4096, 1 << 16])
@pytest.mark.parametrize("factor", [0, 2, 3])
@pytest.mark.parametrize("label", WEIER)
def test_precomputed_matches_oracle_and_plain(curves, label, factor, n):
    """3 curves x F x n, GLV on and off, safe and unsafe, host and resident scalars"""
    curve = curves(label)
    q = P.CURVES[label]["order"]
    rng = random.Random(100 * factor + n)
    pts = curve.Parallel.randomPointsFast(n, 31 + n)
    pb = curve.Affine.toBigints(pts)
    s = [rng.randrange(q) for _ in range(n)]
    want = _strip(c_oracle.msm(P.CURVES[label], s, pb))
    host = _enc(s)
    res = curve.Parallel.scalarsFromBytes(host, n)
    for glv in (0, 1):
        pre = curve.Parallel.precomputePoints(pts, n, {"glv": glv}, factor)
        assert pre.info["glv"] == glv and pre.info["factor"] >= 2
        if factor:
            assert pre.info["factor"] == factor
        for safe in (0, 1):
            for sc in (host, res):
                assert _msm(curve, sc, pre, n, {}, safe) == want, (glv, safe)
        assert _msm(curve, res, pts, n, {"glv": glv, "c": pre.info["c"]}, 0) == want
        pre.free()
    res.free()
    pts.free()


@pytest.mark.parametrize("label", WEIER)
def test_precomputed_prefix_and_defaults(curves, label):
    """an MSM over a prefix of the precomputed set; the engine's default c / GLV; opts that name the handle's own"""
    curve = curves(label)
    q = P.CURVES[label]["order"]
    n = 3000
    rng = random.Random(7)
    pts = curve.Parallel.randomPointsFast(n, 12)
    pb = curve.Affine.toBigints(pts)
    pre = curve.Parallel.precomputePoints(pts, n)
    info = pre.info
    assert info["records"] == info["factor"] * n * (2 if info["glv"] else 1)
    for m in (1, 999, n):
        s = [rng.randrange(q) for _ in range(m)]
        want = _strip(c_oracle.msm(P.CURVES[label], s, pb[:m]))
        assert _msm(curve, _enc(s), pre, m, {}, 1) == want, m
        assert _msm(curve, _enc(s), pre, m, {"c": info["c"], "glv": info["glv"]}, 0) == want, m
    pre.free()
    pts.free()


@pytest.mark.parametrize("c", [3, 5, 11, 16, 17])
@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_precomputed_user_window(curves, label, c):
    """user window sizes, among them ones with a thin top window (BLS12-377, c = 16: 1 bit; c = 5: 3 bits)"""
    curve = curves(label)
    q = P.CURVES[label]["order"]
    n = 2000
    rng = random.Random(c)
    pts = curve.Parallel.randomPointsFast(n, 9)
    pb = curve.Affine.toBigints(pts)
    s = [rng.randrange(q) for _ in range(n)]
    want = _strip(c_oracle.msm(P.CURVES[label], s, pb))
    for glv in (0, 1):
        for factor in (0, 2):
            pre = curve.Parallel.precomputePoints(pts, n, {"glv": glv, "c": c}, factor)
            assert pre.info["c"] == c
            assert _msm(curve, _enc(s), pre, n, {}, 0) == want, (glv, factor)
            pre.free()


@pytest.mark.parametrize("label", WEIER)
def test_precomputed_special_scalars_and_retry(curves, mod, label):
    """scalars 0, 1, q - 1, all equal; the GLV retry (windows for the proven bound) forced with msmz_test_set_glv_bits"""
    from msm_zprize_amd._native import lib
    curve = curves(label)
    c = P.CURVES[label]
    q = c["order"]
    n = 700
    rng = random.Random(5)
    pts = curve.Parallel.randomPointsFast(n, 3)
    pb = curve.Affine.toBigints(pts)
    vecs = [[0] * n, [1] * n, [q - 1] * n, [rng.randrange(q)] * n, [rng.randrange(q) for _ in range(n)]]
    want = [_strip(c_oracle.msm(c, v, pb)) for v in vecs]
    for glv in (0, 1):
        pre = curve.Parallel.precomputePoints(pts, n, {"glv": glv}, 0)
        for v, w in zip(vecs, want):
            assert _msm(curve, _enc(v), pre, n, {}, 1) == w, glv
        assert [_strip(r) for r in curve.Parallel.msmBatch([_enc(v) for v in vecs], pre, n)] == want
        if glv:
            L = lib()
            before = L.msmz_test_retries(curve._ctx)
            assert L.msmz_test_set_glv_bits(curve._ctx, 100) == 0
            try:
                assert _msm(curve, _enc(vecs[4]), pre, n, {}, 1) == want[4]
                assert [_strip(r) for r in curve.Parallel.msmBatch([_enc(v) for v in vecs[3:]], pre, n)] == want[3:]
            finally:
                assert L.msmz_test_set_glv_bits(curve._ctx, 0) == 0
            assert L.msmz_test_retries(curve._ctx) >= before + 2
        pre.free()


@pytest.mark.parametrize("label", WEIER)
def test_precomputed_degenerate_points_safe(curves, label):
    """a point set holding P, 2^c P, -P and points at infinity (the copies put P and 2^c P into one bucket), safe MSM"""
    curve = curves(label)
    c = P.CURVES[label]
    q, p = c["order"], c["modulus"]
    n, cc = 400, 6
    base = curve.Affine.toBigints(curve.Parallel.randomPointsFast(n, 15))
    for i in range(0, 60, 3):
        base[i + 100] = _strip(c_oracle.scale(c, 1 << cc, base[i]))
        base[i + 101] = {"x": base[i]["x"], "y": (p - base[i]["y"]) % p, "isZero": False}
        base[i + 102] = dict(base[i])
    for i in range(300, 320):
        base[i] = {"x": 0, "y": 0, "isZero": True}
    pts = curve.Parallel.pointsFromBigints(base)
    rng = random.Random(2)
    vecs = [[rng.randrange(q) for _ in range(n)], [rng.randrange(1 << cc)] * n, [1] * n]
    for glv in (0, 1):
        pre = curve.Parallel.precomputePoints(pts, n, {"glv": glv, "c": cc}, 0)
        for v in vecs:
            want = _strip(c_oracle.msm(c, v, base))
            assert _msm(curve, _enc(v), pre, n, {}, 1) == want, glv
        pre.free()


@pytest.mark.parametrize("label", WEIER)
def test_precomputed_records(curves, label):
    """stage check: downloaded record j R + i equals 2^(c j) P_i (and record j R + n + i its endomorphism image's
    partner: same y); points at infinity stay at infinity in every copy"""
    curve = curves(label)
    c = P.CURVES[label]
    n = 37
    base = curve.Affine.toBigints(curve.Parallel.randomPointsFast(n, 8))
    base[5] = {"x": 0, "y": 0, "isZero": True}
    pts = curve.Parallel.pointsFromBigints(base)
    # the cube root of unity the engine's images use (the plain set's record n holds P_0's image): one of params' two
    p = c["modulus"]
    beta = curve.Affine.toBigints(pts, n, 1)[0]["x"] * pow(base[0]["x"], -1, p) % p
    assert beta in (c["endomorphism"]["beta"], c["endomorphism"]["beta"] ** 2 % p)
    for glv, cc, factor in ((0, 7, 0), (1, 9, 3)):
        pre = curve.Parallel.precomputePoints(pts, n, {"glv": glv, "c": cc}, factor)
        info = pre.info
        R = n * (2 if glv else 1)
        assert info["records"] == info["factor"] * R
        recs = curve.Affine.toBigints(pre, 0, info["records"])
        for j in range(info["factor"]):
            for i in range(n):
                got = _strip(recs[j * R + i])
                want = _strip(c_oracle.scale(c, 1 << (cc * j), base[i]))
                if want["isZero"]:
                    assert got["isZero"], (j, i)
                    continue
                assert got == want, (glv, j, i)
                if glv:
                    img = _strip(recs[j * R + n + i])
                    assert img == {"x": beta * want["x"] % p, "y": want["y"], "isZero": False}, (j, i)
            if glv:
                assert recs[j * R + n + 5]["isZero"]
        pre.free()
    pts.free()


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("label", WEIER)
def test_precomputed_batch(curves, label, B):
    """batched MSMs over a precomputed handle, host and resident scalars"""
    curve = curves(label)
    q = P.CURVES[label]["order"]
    n = 1500
    rng = random.Random(B)
    pts = curve.Parallel.randomPointsFast(n, 44)
    pb = curve.Affine.toBigints(pts)
    vecs = [[rng.randrange(q) for _ in range(n)] for _ in range(B)]
    want = [_strip(c_oracle.msm(P.CURVES[label], v, pb)) for v in vecs]
    host = [_enc(v) for v in vecs]
    res = curve.Parallel.scalarsFromBytes(b"".join(host), B * n)
    for glv, factor in ((0, 0), (1, 0), (0, 3)):
        pre = curve.Parallel.precomputePoints(pts, n, {"glv": glv}, factor)
        for safe in (0, 1):
            f = curve.Parallel.msmBatch if safe else curve.Parallel.msmBatchUnsafe
            assert [_strip(r) for r in f(host, pre, n)] == want, (glv, factor, safe)
            assert [_strip(r) for r in f(res, pre, n)] == want, (glv, factor, safe, "resident")
        pre.free()
    res.free()
    pts.free()


def test_precomputed_batch_split(curves):
    """B = 69 vectors of 2^16 scalars over a precomputed set: more entries than one batched pass takes (sub-batches of
    35 and 34 vectors); closed form.  (The set is built with c = 17, K = 15 windows, so up to 68 vectors are
    68 x 15 x 2^16 <= 2^26 entries and run as ONE pipeline: the 64 vectors this test used to run never split, which
    the sub-batch counter showed.)"""
    curve = curves("bls12-377")
    c = P.CURVES["bls12-377"]
    q = c["order"]
    n, B = 1 << 16, 69
    pts = curve.Parallel.randomPointsFast(n, 21)
    sc = curve.Parallel.randomScalars(B * n, 22)
    a = prng.multipliers_np(21, n)
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    want = [_strip(c_oracle.scale(c, prng.sum_of_products_mod(prng.scalars_np(22, n, q, first=k * n), a, q), gen))
            for k in range(B)]
    pre = curve.Parallel.precomputePoints(pts, n, {"glv": 0}, 0)
    from msm_zprize_amd._native import lib
    L = lib()
    sb0, sb1 = C.c_uint64(), C.c_uint64()
    assert L.msmz_test_passes(curve._ctx, None, C.byref(sb0)) == 0
    assert [_strip(r) for r in curve.Parallel.msmBatchUnsafe(sc, pre, n)] == want
    assert L.msmz_test_passes(curve._ctx, None, C.byref(sb1)) == 0
    assert sb1.value >= sb0.value + 2   # (sub-batches: the split path was taken)
    pre.free()
    sc.free()
    pts.free()


def test_precomputed_2e20_closed_form(curves):
    """2^20 device-generated points and scalars at the default c, closed form (sum_i s_i a_i) G"""
    curve = curves("bls12-377")
    c = P.CURVES["bls12-377"]
    q = c["order"]
    n = 1 << 20
    pts = curve.Parallel.randomPointsFast(n, 101)
    sc = curve.Parallel.randomScalars(n, 102)
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    t = prng.sum_of_products_mod(prng.scalars_np(102, n, q), prng.multipliers_np(101, n), q)
    want = _strip(c_oracle.scale(c, t, gen))
    pre = curve.Parallel.precomputePoints(pts, n)
    pts.free()   # the precomputed handle owns its memory
    assert _msm(curve, sc, pre, n, {}, 0) == want
    pre.free()
    sc.free()


def test_precomputed_longest_bucket(curves):
    """2^20 + 2^18 points, c = 16, all 16 windows in one set, every scalar sum_k 2^(16 k): each window's digit is 1, so
    one bucket collects 16 n > 2^24 entries (a plain set's bucket never exceeds 2^24).  The precomputed set accepts the
    shape and the MSM matches the closed form and the plain set"""
    curve = curves("bls12-377")
    c = P.CURVES["bls12-377"]
    q = c["order"]
    n, cc = (1 << 20) + (1 << 18), 16
    pts = curve.Parallel.randomPointsFast(n, 55)
    s = sum(1 << (cc * k) for k in range(16))
    assert s < q
    host = s.to_bytes(32, "little") * n
    a = prng.multipliers_np(55, n)
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    want = _strip(c_oracle.scale(c, s * (int(a.astype(object).sum()) % q) % q, gen))
    pre = curve.Parallel.precomputePoints(pts, n, {"glv": 0, "c": cc}, 0)
    assert pre.info["factor"] == pre.info["K"] == 16
    got = curve.Parallel.msm(host, pre, n, True)
    assert got["stats"].max_bucket == 16 * n > 1 << 24
    assert _strip(got["result"]) == want
    assert _msm(curve, host, pts, n, {"glv": 0, "c": cc}, 1) == want
    pre.free()
    pts.free()


def test_precomputed_errors_then_usable(curves, mod):
    """TE / projective: UNSUPPORTED; c or GLV mismatch, N above n, factor 1, the size limit: ARG; a scalar >= q: RANGE,
    and the context stays usable; freeing the source leaves the precomputed handle working"""
    from msm_zprize_amd._native import MsmzOpts, lib
    L = lib()
    ed = curves("ed-on-bls12-377")
    tp = ed.Parallel.randomPointsFast(16, 1)
    o = MsmzOpts()
    o.glv = -1
    h = C.c_uint64()
    assert L.msmz_precompute_points(ed._ctx, tp.handle, 16, C.byref(o), 0, C.byref(h)) == MSMZ_ERR_UNSUPPORTED

    curve = curves("bls12-381")
    c = P.CURVES["bls12-381"]
    q = c["order"]
    n = 300
    pts = curve.Parallel.randomPointsFast(n, 2)
    pb = curve.Affine.toBigints(pts)
    o = MsmzOpts()
    o.glv = -1
    o.buckets = 1
    assert L.msmz_precompute_points(curve._ctx, pts.handle, n, C.byref(o), 0, C.byref(h)) == MSMZ_ERR_UNSUPPORTED
    o.buckets = 0
    o.reserved[0] = 1
    assert L.msmz_precompute_points(curve._ctx, pts.handle, n, C.byref(o), 0, C.byref(h)) == MSMZ_ERR_UNSUPPORTED
    o.reserved[0] = 0
    assert L.msmz_precompute_points(curve._ctx, pts.handle, n, C.byref(o), 1, C.byref(h)) == MSMZ_ERR_ARG
    assert L.msmz_precompute_points(curve._ctx, pts.handle, n + 1, C.byref(o), 0, C.byref(h)) == MSMZ_ERR_ARG
    assert L.msmz_precompute_points(curve._ctx, 987654, n, C.byref(o), 0, C.byref(h)) == MSMZ_ERR_ARG
    # size limit: 2^20 points, c = 18, all windows in one set -- the packed index leaves too few fine bits, a window
    # would need more coarse bins than one sort pass holds
    big = curve.Parallel.randomPointsFast(1 << 20, 3)
    o.c, o.glv = 18, 0
    assert L.msmz_precompute_points(curve._ctx, big.handle, 1 << 20, C.byref(o), 0, C.byref(h)) == MSMZ_ERR_ARG
    big.free()

    pre = curve.Parallel.precomputePoints(pts, n, {"glv": 0, "c": 7}, 0)
    assert L.msmz_precompute_points(curve._ctx, pre.handle, n, None, 0, C.byref(h)) == MSMZ_ERR_ARG   # not twice
    pts.free()
    rng = random.Random(4)
    s = [rng.randrange(q) for _ in range(n)]
    want = _strip(c_oracle.msm(c, s, pb))
    for bad in ({"c": 8}, {"glv": 1}, {"buckets": 1}):
        with pytest.raises(mod._native.MsmzError) as e:
            if "buckets" in bad:
                curve.Parallel._msm(_enc(s), pre, n, False, {}, 1, 1)
            else:
                _msm(curve, _enc(s), pre, n, bad, 1)
        assert e.value.status == (MSMZ_ERR_UNSUPPORTED if "buckets" in bad else MSMZ_ERR_ARG), bad
    out = C.create_string_buffer(96)
    inf = C.c_int()
    assert L.msmz_msm(curve._ctx, pre.handle, _enc(s) + _enc([0]), n + 1, None, out, C.byref(inf), None) == MSMZ_ERR_ARG
    bad = list(s)
    bad[77] = q
    with pytest.raises(mod._native.MsmzError) as e:
        _msm(curve, _enc(bad), pre, n, {}, 1)
    assert e.value.status == MSMZ_ERR_RANGE
    assert _msm(curve, _enc(s), pre, n, {}, 1) == want
    assert L.msmz_msm(curve._ctx, pre.handle, _enc(s), n, None, out, C.byref(inf), None) == 0   # null opts: defaults
    got = {"x": int.from_bytes(out.raw[:48], "little"), "y": int.from_bytes(out.raw[48:], "little"), "isZero": False}
    assert got == want
    ci, gi, fi, ki, ri = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    assert L.msmz_precomputed_info(curve._ctx, pre.handle, C.byref(ci), C.byref(gi), C.byref(fi), C.byref(ki),
                                   C.byref(ri)) == 0
    assert (ci.value, gi.value, fi.value, ki.value, ri.value) == (7, 0, ki.value, ki.value, ki.value * n)
    assert L.msmz_precomputed_info(curve._ctx, pre.handle, None, None, None, None, None) == 0
    pre.free()
    assert L.msmz_precomputed_info(curve._ctx, ri.value + 12345, None, None, None, None, None) == MSMZ_ERR_ARG


@pytest.mark.parametrize("engines", [2, 3])
def test_precomputed_multi_engine(mod, engines):
    """2- and 3-engine contexts on device 0: every engine precomputes its share; single and batched MSMs agree with the
    single-engine context's plain handle"""
    n, B = (1 << 17) + 1234, 3
    mod.startThreads(devices=[0])
    one = mod.Weierstrass.create(mod.curves.bls12377Params)
    mod.startThreads(devices=[0] * engines)
    multi = mod.Weierstrass.create(mod.curves.bls12377Params)
    try:
        rng = random.Random(engines)
        q = P.CURVES["bls12-377"]["order"]
        host = [_enc([rng.randrange(q) for _ in range(n)]) for _ in range(B)]
        p1 = one.Parallel.randomPointsFast(n, 4)
        pm = multi.Parallel.randomPointsFast(n, 4)
        for glv in (0, 1):
            want = one.Parallel.msmBatchUnsafe(host, p1, n, {"glv": glv})
            pre = multi.Parallel.precomputePoints(pm, n, {"glv": glv}, 0)
            assert pre.info["records"] == pre.info["factor"] * n * (2 if glv else 1)
            assert multi.Parallel.msmBatchUnsafe(host, pre, n) == want
            assert multi.Parallel.msmUnsafe(host[1], pre, n)["result"] == want[1]
            sm = multi.Parallel.scalarsFromBytes(b"".join(host), B * n)
            assert multi.Parallel.msmBatch(sm, pre, n) == want
            sm.free()
            pre.free()
    finally:
        one.close()
        multi.close()
        mod.startThreads()

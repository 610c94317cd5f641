"""Batched MSM (msmz_msm_batch / msmz_msm_batch_resident): B scalar vectors against one resident point set.  Every
result is compared bit-exactly, per problem, against the C oracle and against msmz_msm_resident run once per vector."""
import ctypes as C
import random

import pytest

from oracle import c_oracle
from oracle import params as P
from oracle import prng

pytestmark = pytest.mark.gpu

WEIER = ["bls12-377", "pallas", "bls12-381"]
MSMZ_ERR_ARG, MSMZ_ERR_RANGE = 1, 6


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


def _sub_batches(curve):
    """batched pipelines the context ran to a result so far (msmz_test_passes)"""
    from msm_zprize_amd._native import lib
    sb = C.c_uint64()
    assert lib().msmz_test_passes(curve._ctx, None, C.byref(sb)) == 0
    return sb.value


def _loop_resident(curve, vecs, pts, n, opts, safe):
    """msmz_msm_resident once per vector"""
    out = []
    for v in vecs:
        sc = curve.Parallel.scalarsFromBytes(_enc(v), n)
        f = curve.Parallel.msm if safe else curve.Parallel.msmUnsafe
        out.append(_strip(f(sc, pts, n, False, dict(opts))["result"]))
        sc.free()
    return out


@pytest.mark.parametrize("n", [1, 5, 257, 4096])
@pytest.mark.parametrize("B", [1, 2, 3, 17])
@pytest.mark.parametrize("label", WEIER)
def test_batch_matches_oracle_and_loop(curves, label, B, n):
    """3 curves x GLV on / off x safe / unsafe, host-buffer and resident scalars"""
    curve = curves(label)
    q = P.CURVES[label]["order"]
    rng = random.Random(1000 * B + n)
    pts = curve.Parallel.randomPointsFast(n, 77 + n)
    pb = curve.Affine.toBigints(pts)
    vecs = [[rng.randrange(q) for _ in range(n)] for _ in range(B)]
    want = [_strip(c_oracle.msm(P.CURVES[label], v, pb)) for v in vecs]
    host = [_enc(v) for v in vecs]
    res = curve.Parallel.scalarsFromBytes(b"".join(host), B * n)
    for glv in (0, 1):
        for safe in (0, 1):
            f = curve.Parallel.msmBatch if safe else curve.Parallel.msmBatchUnsafe
            got = [_strip(r) for r in f(host, pts, n, {"glv": glv})]
            assert got == want, (glv, safe)
            got = [_strip(r) for r in f(res, pts, n, {"glv": glv})]
            assert got == want, (glv, safe, "resident")
    assert _loop_resident(curve, vecs, pts, n, {"glv": 1}, 0) == want
    res.free()
    pts.free()


@pytest.mark.parametrize("label", WEIER)
def test_batch_mixed_vectors_safe(curves, label):
    """vectors of different kinds in one batch (all zero, all equal, q - 1, random) over a point set with equal and
    opposite points, safe additions"""
    curve = curves(label)
    c = P.CURVES[label]
    q, p = c["order"], c["modulus"]
    n = 300
    base = curve.Affine.toBigints(curve.Parallel.randomPointsFast(n, 5))
    for i in range(0, 100, 2):   # equal and opposite points
        base[i + 100] = dict(base[i])
        base[i + 101] = {"x": base[i]["x"], "y": (p - base[i]["y"]) % p, "isZero": False}
    pts = curve.Parallel.pointsFromBigints(base)
    rng = random.Random(3)
    vecs = [[0] * n, [rng.randrange(q)] * n, [q - 1] * n, [rng.randrange(q) for _ in range(n)], [1] * n]
    want = [_strip(c_oracle.msm(c, v, base)) for v in vecs]
    for glv in (0, 1):
        got = [_strip(r) for r in curve.Parallel.msmBatch([_enc(v) for v in vecs], pts, n, {"glv": glv})]
        assert got == want, glv
    assert _loop_resident(curve, vecs, pts, n, {"glv": 0}, 1) == want


@pytest.mark.parametrize("c", [5, 11, 16, 17])
@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_batch_user_window(curves, label, c):
    """user-chosen window sizes: generic kernels and the ones specialised for c = 16 / 17"""
    curve = curves(label)
    q = P.CURVES[label]["order"]
    n, B = 3000, 4
    rng = random.Random(c)
    pts = curve.Parallel.randomPointsFast(n, 9)
    pb = curve.Affine.toBigints(pts)
    vecs = [[rng.randrange(q) for _ in range(n)] for _ in range(B)]
    want = [_strip(c_oracle.msm(P.CURVES[label], v, pb)) for v in vecs]
    for glv in (0, 1):
        got = [_strip(r) for r in curve.Parallel.msmBatchUnsafe([_enc(v) for v in vecs], pts, n, {"glv": glv, "c": c})]
        assert got == want, glv


def test_batch_large_split(curves):
    """B = 64 vectors of 2^16 device-generated scalars: more entries than one batched pass takes (host sub-batches);
    closed-form expectations"""
    curve = curves("bls12-377")
    c = P.CURVES["bls12-377"]
    q = c["order"]
    n, B = 1 << 16, 64
    pts = curve.Parallel.randomPointsFast(n, 21)
    sc = curve.Parallel.randomScalars(B * n, 22)
    a = prng.multipliers_np(21, n)
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    want = []
    for k in range(B):
        t = prng.sum_of_products_mod(prng.scalars_np(22, n, q, first=k * n), a, q)
        want.append(_strip(c_oracle.scale(c, t, gen)))
    for glv in (0, 1):
        before = _sub_batches(curve)
        got = [_strip(r) for r in curve.Parallel.msmBatchUnsafe(sc, pts, n, {"glv": glv})]
        assert got == want, glv
        assert _sub_batches(curve) >= before + 2, glv   # (the split path was taken)
    log = curve.Parallel.lastBatchLog
    assert log.n_entries > B * n   # totals over the batch
    sc.free()
    pts.free()


def test_batch_range_error_then_usable(curves, mod):
    curve = curves("bls12-381")
    q = P.CURVES["bls12-381"]["order"]
    n, B = 100, 3
    rng = random.Random(8)
    pts = curve.Parallel.randomPointsFast(n, 2)
    pb = curve.Affine.toBigints(pts)
    vecs = [[rng.randrange(q) for _ in range(n)] for _ in range(B)]
    bad = [list(v) for v in vecs]
    bad[1][37] = q
    with pytest.raises(mod._native.MsmzError) as e:
        curve.Parallel.msmBatch([_enc(v) for v in bad], pts, n)
    assert e.value.status == MSMZ_ERR_RANGE
    want = [_strip(c_oracle.msm(P.CURVES["bls12-381"], v, pb)) for v in vecs]
    assert [_strip(r) for r in curve.Parallel.msmBatch([_enc(v) for v in vecs], pts, n)] == want


def test_batch_abi_arguments(curves, mod):
    """batch == 0, n == 0, null buffers, a resident set shorter than batch * n"""
    from msm_zprize_amd._native import MsmzOpts, lib
    curve = curves("pallas")
    pts = curve.Parallel.randomPointsFast(8, 1)
    sc = curve.Parallel.randomScalars(15, 1)
    out = C.create_string_buffer(64 * 4)
    inf = (C.c_int * 4)()
    o = MsmzOpts()
    L = lib()
    s = b"\x01" + b"\x00" * 31
    assert L.msmz_msm_batch(curve._ctx, pts.handle, s * 8, 8, 0, C.byref(o), out, inf, None) == MSMZ_ERR_ARG
    assert L.msmz_msm_batch(curve._ctx, pts.handle, s * 8, 0, 1, C.byref(o), out, inf, None) == MSMZ_ERR_ARG
    assert L.msmz_msm_batch(curve._ctx, pts.handle, None, 8, 1, C.byref(o), out, inf, None) == MSMZ_ERR_ARG
    assert L.msmz_msm_batch(curve._ctx, pts.handle, s * 8, 8, 1, C.byref(o), None, inf, None) == MSMZ_ERR_ARG
    assert L.msmz_msm_batch_resident(curve._ctx, pts.handle, sc.handle, 8, 2, C.byref(o), out, inf, None) == MSMZ_ERR_ARG
    assert L.msmz_msm_batch_resident(curve._ctx, pts.handle, sc.handle, 7, 2, C.byref(o), out, inf, None) == 0


@pytest.mark.parametrize("engines", [2, 3])
def test_batch_multi_engine(mod, engines):
    """2- and 3-engine contexts on device 0 (blocks of 2^16 dealt round-robin) agree with the single-engine batch"""
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
            assert multi.Parallel.msmBatchUnsafe(host, pm, n, {"glv": glv}) == want
            sm = multi.Parallel.scalarsFromBytes(b"".join(host), B * n)
            assert multi.Parallel.msmBatch(sm, pm, n, {"glv": glv}) == want
            sm.free()
    finally:
        one.close()
        multi.close()
        mod.startThreads()


def test_batch_twisted_edwards_and_projective(curves):
    """ed-on-bls12-377 and projective buckets run the problems one by one: same per-problem results"""
    n, B = 500, 3
    for label in ("ed-on-bls12-377", "bls12-377"):
        curve = curves(label)
        c = P.CURVES[label]
        rng = random.Random(11)
        pts = curve.Parallel.randomPointsFast(n, 6)
        pb = curve.Affine.toBigints(pts)
        vecs = [[rng.randrange(c["order"]) for _ in range(n)] for _ in range(B)]
        want = [_strip(c_oracle.msm(c, v, pb)) for v in vecs]
        opts = {"glv": 0, "buckets": 1} if label == "bls12-377" else {}
        got = [_strip(r) for r in curve.Parallel.msmBatch([_enc(v) for v in vecs], pts, n, opts)]
        if label == "ed-on-bls12-377":   # twisted Edwards results carry no infinity flag
            got = [{"x": g["x"], "y": g["y"]} for g in got]
            want = [{"x": w["x"], "y": w["y"]} for w in want]
        assert got == want, label

"""Full-size checks at BASELINE.json's configurations, where the oracle itself is too slow: the
reference has no check beyond 2^12 either, so these use size-independent
properties of structured inputs:

  * points are P_i = a_i * G with known a_i, hence  MSM = (sum_i s_i a_i mod q) * G   (closed form,
    the expected point computed by the oracle with ONE scalar multiplication);
  * shard additivity  MSM(A u B) = MSM(A) + MSM(B)  (the multi-GPU combine step, msmz_point_add);
  * every algorithm variant (GLV on/off, affine / projective buckets, different c) and a repeated run
    give byte-identical canonical results (determinism despite atomically ordered buckets).
"""
import pytest

from oracle import c_oracle
from oracle import params as P
from oracle import prng

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    import msm_zprize_amd as m
    m.startThreads()
    return m


def test_first_msm_of_a_context_at_2e24(mod):
    """A fresh context whose FIRST MSM runs the sort at its largest LDS footprints: 2^24 points leave 7 fine bits, so
    k_coarse stages 8192 bins (96 KB of dynamic LDS on top of 32.8 KB static) and k_fine its full 156 KB.  The LDS
    limits are raised once in Engine::init(); nothing is retried (round 2 hid an `invalid argument` behind a second
    attempt).  Closed form as below."""
    curve = mod.Weierstrass.create(mod.curves.bls12377Params)
    try:
        n = 1 << 24
        pts = curve.Parallel.randomPointsFast(n, 41)
        sc = curve.Parallel.randomScalars(n, 42)
        out = curve.Parallel.msmUnsafe(sc, pts, n, True, {"glv": 0})
        assert _strip(out["result"]) == _expected("bls12-377", 41, 42, n)
        assert out["stats"].c == 17 and out["stats"].K == 15
    finally:
        curve.close()


def _expected(label, pseed, sseed, n):
    c = P.CURVES[label]
    q = c["order"]
    t = prng.sum_of_products_mod(prng.scalars_np(sseed, n, q), prng.multipliers_np(pseed, n), q)
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    r = c_oracle.scale(c, t, gen)
    return {"x": r["x"], "y": r["y"], "isZero": bool(r.get("isZero", False))}


def _strip(p):
    return {"x": p["x"], "y": p["y"], "isZero": bool(p.get("isZero", False))}


def _range_passes(curve):
    """index-range passes the context ran so far (msmz_test_passes)"""
    import ctypes as C
    from msm_zprize_amd._native import lib
    rp = C.c_uint64()
    assert lib().msmz_test_passes(curve._ctx, C.byref(rp), None) == 0
    return rp.value


def test_config2_bls12_377_2e20_no_glv_affine(mod):
    """BASELINE configs[1]: BLS12-377 G1, 2^20, no GLV, affine buckets -- plus the variants"""
    curve = mod.Weierstrass.create(mod.curves.bls12377Params)
    n = 1 << 20
    pts = curve.Parallel.randomPointsFast(n, 11)
    sc = curve.Parallel.randomScalars(n, 12)
    want = _expected("bls12-377", 11, 12, n)
    r1 = curve.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 0})["result"]
    assert r1 == want
    assert curve.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 0})["result"] == r1          # determinism
    assert curve.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 1})["result"] == want        # reference default (GLV)
    assert curve.Parallel.msm(sc, pts, n, False, {"glv": 0, "c": 13})["result"] == want     # safe adds, other window
    assert curve.Parallel.msmProjective(sc, pts, n)["result"] == want
    # shard additivity on the first 2^18 points: MSM(A u B) = MSM(A) + MSM(B) with B uploaded separately
    h = 1 << 17
    pa = curve.Affine.toBigints(pts, 0, 2 * h)
    sa = curve.Scalar.toBigints(sc, 0, 2 * h)
    whole = curve.Parallel.msmUnsafe(curve.Parallel.scalarsFromBigints(sa), curve.Parallel.pointsFromBigints(pa), 2 * h,
                                     False, {"glv": 0})["result"]
    a = curve.Parallel.msmUnsafe(curve.Parallel.scalarsFromBigints(sa[:h]), curve.Parallel.pointsFromBigints(pa[:h]), h,
                                 False, {"glv": 0})["result"]
    b = curve.Parallel.msmUnsafe(curve.Parallel.scalarsFromBigints(sa[h:]), curve.Parallel.pointsFromBigints(pa[h:]), h,
                                 False, {"glv": 0})["result"]
    assert curve.pointAdd(a, b) == whole
    curve.close()


def test_default_glv_choice_follows_the_input_size(mod):
    """options without `glv`: the engine splits with GLV below 2^21 points and not from there on (include/msmz.h);
    either way the result is the closed form"""
    curve = mod.Weierstrass.create(mod.curves.bls12377Params)
    for log2n, glv in ((12, 1), (21, 0)):
        n = 1 << log2n
        pts = curve.Parallel.randomPointsFast(n, 21)
        sc = curve.Parallel.randomScalars(n, 22)
        out = curve.Parallel.msmUnsafe(sc, pts, n, True)
        assert out["result"] == _expected("bls12-377", 21, 22, n)
        assert out["stats"].glv == glv
        pts.free(); sc.free()
    curve.close()


def test_config3_pallas_2e22_projective(mod):
    """BASELINE configs[2]: Pallas 2^22, projective buckets (msmProjective, parallel.ts:69-87)"""
    curve = mod.Weierstrass.create(mod.curves.pallasParams)
    n = 1 << 22
    pts = curve.Parallel.randomPointsFast(n, 21)
    sc = curve.Parallel.randomScalars(n, 22)
    want = _expected("pallas", 21, 22, n)
    assert curve.Parallel.msmProjective(sc, pts, n)["result"] == want
    assert curve.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 1})["result"] == want
    curve.close()


def test_config4_ed_on_bls12_377_2e24(mod):
    """BASELINE configs[3]: twisted Edwards 2^24 (ed-on-bls12-377; the reference's TE path has no GLV)"""
    curve = mod.TwistedEdwards.create(mod.curves.edOnBls12377Params)
    n = 1 << 24
    pts = curve.Parallel.randomPointsFast(n, 31)
    sc = curve.Parallel.randomScalars(n, 32)
    want = _expected("ed-on-bls12-377", 31, 32, n)
    assert _strip(curve.Parallel.msm(sc, pts, n)["result"]) == want
    curve.close()


def test_bls12_381_2e18(mod):
    curve = mod.Weierstrass.create(mod.curves.bls12381Params)
    n = 1 << 18
    pts = curve.Parallel.randomPointsFast(n, 41)
    sc = curve.Parallel.randomScalars(n, 42)
    want = _expected("bls12-381", 41, 42, n)
    assert curve.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 1})["result"] == want
    assert curve.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 0})["result"] == want
    curve.close()


def test_config5_shard_2e23_per_gpu(mod):
    """BASELINE configs[4] runs 2^23 points per GPU on 8 GPUs: one shard of that size, closed-form check"""
    curve = mod.Weierstrass.create(mod.curves.bls12377Params)
    n = 1 << 23
    pts = curve.Parallel.randomPointsFast(n, 51)
    sc = curve.Parallel.randomScalars(n, 52)
    assert curve.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 0})["result"] == _expected("bls12-377", 51, 52, n)
    curve.close()


def test_inputs_beyond_one_sorting_pass(mod):
    """sizes whose (half-)scalar count exceeds one sorting pass (2^24 entries) run as index ranges
    inside the engine: BLS12-377 2^25 without GLV (two passes of 2^24) and 2^24 with GLV (two passes of 2^23 points,
    each addressing its endomorphism images behind the WHOLE set) -- closed form as above"""
    curve = mod.Weierstrass.create(mod.curves.bls12377Params)
    n = 1 << 25
    pts = curve.Parallel.randomPointsFast(n, 61)
    sc = curve.Parallel.randomScalars(n, 62)
    before = _range_passes(curve)
    assert curve.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 0})["result"] == _expected("bls12-377", 61, 62, n)
    assert _range_passes(curve) == before + 2
    h = 1 << 24
    assert curve.Parallel.msmUnsafe(sc, pts, h, False, {"glv": 1})["result"] == _expected("bls12-377", 61, 62, h)
    assert _range_passes(curve) == before + 4   # (each call ran exactly two index-range passes)
    pts.free(); sc.free()
    curve.close()


def test_two_engine_context_at_full_size(mod):
    """msmz_create with n_devices = 2 (two engines on GPU 0): 2^20 points split in blocks over the engines, every
    variant equal to the closed form"""
    mod.startThreads(devices=[0, 0])
    curve = mod.Weierstrass.create(mod.curves.bls12377Params)
    mod.startThreads()
    n = 1 << 20
    pts = curve.Parallel.randomPointsFast(n, 11)
    sc = curve.Parallel.randomScalars(n, 12)
    want = _expected("bls12-377", 11, 12, n)
    assert curve.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 0})["result"] == want
    assert curve.Parallel.msmUnsafe(sc, pts, n, True, {"glv": 1})["result"] == want
    curve.close()


@pytest.mark.parametrize("label", ["bls12-377", "pallas", "ed-on-bls12-377"])
def test_equal_scalars_one_long_bucket_per_window(mod, label):
    """Adversarial input: all 2^16 scalars equal, so every window has ONE bucket holding every point (the
    same-scalar case of src/bigint/msm.test.ts:47-56 at a size where it stresses the long-bucket handling: many tree
    rounds on the affine path, sqrt-sized chunks on the projective / twisted-Edwards path).
    Expected: (s * sum a_i mod q) * G."""
    import numpy as np
    c = P.CURVES[label]
    q = c["order"]
    n = 1 << 16
    params = mod.curves.BY_LABEL[label]
    curve = (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)
    pts = curve.Parallel.randomPointsFast(n, 31)
    a_sum = int(sum(int(v) for v in prng.multipliers_np(31, n)))
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    for s in (q - 2, 0x1234567890ABCDEF1234567890ABCDEF1234567 % q):
        r = c_oracle.scale(c, s * a_sum % q, gen)
        want = {"x": r["x"], "y": r["y"], "isZero": bool(r.get("isZero", False))}
        sc = curve.Parallel.scalarsFromBytes(int(s).to_bytes(32, "little") * n, n)
        if params["kind"] == "weierstrass":
            assert _strip(curve.Parallel.msmUnsafe(sc, pts, n, False, {"glv": 0})["result"]) == want
            assert _strip(curve.Parallel.msm(sc, pts, n, False, {"glv": 1})["result"]) == want
            assert _strip(curve.Parallel.msmProjective(sc, pts, n)["result"]) == want
        else:
            assert _strip(curve.Parallel.msm(sc, pts, n)["result"]) == want
        sc.free()
    curve.close()

"""msmz_points_mul on the GPU (k_points_mul over either group policy, csrc/mul_kernels.h): downloaded records against the
oracle's [s]P (+ Q) (tests/points_mul_util.py over oracle/bigint_ref.py) at the sizes that exercise the whole-wave
normalisation, the IPA fold, the result used as an ordinary point set, the closed form over generated inputs, the
errors and a multi-engine context."""
import ctypes as C
import random

import pytest

import check_points_util as U
import points_mul_util as M
from oracle import params as P
from oracle import prng

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
SIZES = [1, 63, 64, 65, 257]   # a partial wave, a full wave, a wave plus one lane, several blocks with a ragged tail


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


def _mul(curve, points, n, scalars, addend=None, fp=0, fs=0, fq=0):
    """msmz_points_mul through the C ABI -> (status, handle).  scalars: a resident array, an int (broadcast) or None
    (scalars_handle == 0 with a null scalar)"""
    from msm_zprize_amd._native import MsmzMul
    raw = None if scalars is None or hasattr(scalars, "handle") else int(scalars).to_bytes(32, "little")
    m = MsmzMul(points if isinstance(points, int) else points.handle, fp,
                scalars.handle if hasattr(scalars, "handle") else 0, fs, raw,
                0 if addend is None else (addend if isinstance(addend, int) else addend.handle), fq)
    h = C.c_uint64(0)
    st = _lib().msmz_points_mul(curve._ctx, C.byref(m), n, C.byref(h))
    return st, h.value


def _strip(p):
    return {"x": p["x"], "y": p["y"], "isZero": bool(p.get("isZero", False))}


def _download(curve, handle, n):
    from msm_zprize_amd.parallel import DeviceArray
    arr = DeviceArray(curve, handle, n, "points")
    pts = [_strip(p) for p in curve.Affine.toBigints(arr)]
    return arr, pts


_sets = {}


def _reference(label, n):
    """the rows of one set and the oracle's answers for the three modes, computed once per (curve, size)"""
    if (label, n) not in _sets:
        params = P.CURVES[label]
        rows = M.build_set(label, n, 1000 * M.ALL.index(label) + n)
        u = random.Random(n).randrange(1, params["order"])
        plain = [U.scale(params, s, p) for s, p, _ in rows]
        _sets[(label, n)] = dict(
            rows=rows, u=u, plain=[M.canon(params, r) for r in plain],
            added=[M.canon(params, U.add(params, r, q)) for r, (_, _, q) in zip(plain, rows)],
            bcast=[M.expected(params, u, p, q) for _, p, q in rows])
    return _sets[(label, n)]


# ---------------------------------------------------------------------------------------------- bit-exact downloads
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("label", M.ALL)
def test_downloads_equal_the_oracle(curves, label, n):
    """records and infinity flags of [s_i]P_i, [s_i]P_i + Q_i and [u]P_i + Q_i == the oracle's affine points; the sets
    hold s = 0, 1, q - 1, P and Q at infinity, Q = +-[s]P and (cofactor curves) a small-order point, in the first wave
    and in the last one"""
    curve, params, ref = curves(label), P.CURVES[label], _reference(label, n)
    rows = ref["rows"]
    pa = curve.Parallel.pointsFromBigints([p for _, p, _ in rows])
    qa = curve.Parallel.pointsFromBigints([q for _, _, q in rows])
    sa = curve.Parallel.scalarsFromBigints([s for s, _, _ in rows])
    for mode, args, want in [("plain", (sa, None), ref["plain"]), ("addend", (sa, qa), ref["added"]),
                             ("broadcast", (ref["u"], qa), ref["bcast"])]:
        st, h = _mul(curve, pa, n, *args)
        assert st == 0, (mode, st)
        out, got = _download(curve, h, n)
        bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if M.canon(params, g) != w]
        assert not bad, (mode, bad[:3])
        if params["kind"] == "weierstrass":
            assert [g["isZero"] for g in got] == [w["isZero"] for w in want]
        out.free()
    st, h = _mul(curve, pa, n, 0)   # [0]P: the neutral element everywhere
    assert st == 0
    out, got = _download(curve, h, n)
    assert all(M.canon(params, g) == M.neutral(params) for g in got)
    out.free()
    pa.free(); qa.free(); sa.free()


# ---------------------------------------------------------------------------------------------- the IPA fold
@pytest.mark.parametrize("label", ["pallas", "bls12-377"])
def test_ipa_fold(curves, label):
    """G'_i = G_lo,i + [u] G_hi,i over the halves of ONE handle: P = Q, first_p = 64, first_q = 0, the broadcast u"""
    curve, params = curves(label), P.CURVES[label]
    n = 128
    gens = curve.Parallel.randomPointsFast(n, 31)
    g = [_strip(p) for p in curve.Affine.toBigints(gens)]
    u = random.Random(5).randrange(1, params["order"])
    st, h = _mul(curve, gens, n // 2, u, gens, fp=n // 2, fq=0)
    assert st == 0
    out, got = _download(curve, h, n // 2)
    assert got == [M.expected(params, u, g[n // 2 + i], g[i]) for i in range(n // 2)]
    out.free(); gens.free()


# ---------------------------------------------------------------------------------------------- the result as a set
@pytest.mark.parametrize("label", M.ALL)
def test_result_is_an_ordinary_point_set(curves, label):
    """msm(t, mulPoints(s, P)) == msm(s t mod q, P), safe and unsafe, GLV on and off (the endomorphism images of the
    new set are read); checkPoints finds nothing; a precomputed copy of it gives the same MSM"""
    curve, params = curves(label), P.CURVES[label]
    n, q = 1 << 12, params["order"]
    weier = params["kind"] == "weierstrass"
    pts = curve.Parallel.randomPointsFast(n, 11)
    s = curve.Parallel.randomScalars(n, 12)
    t = curve.Parallel.randomScalars(n, 13)
    st_ = curve.Parallel.scalarsFromBigints([a * b % q for a, b in zip(curve.Scalar.toBigints(s), curve.Scalar.toBigints(t))])
    out = curve.Parallel.mulPoints(s, pts)
    assert len(out) == n and out.kind == "points"
    want = None
    for glv in ((0, 1) if weier else (0,)):
        for f in (curve.Parallel.msm, curve.Parallel.msmUnsafe):
            a = _strip(f(t, out, n, False, {"glv": glv})["result"])
            b = _strip(f(st_, pts, n, False, {"glv": glv})["result"])
            assert a == b, (glv, f.__name__)
            assert want is None or a == want
            want = a
    assert not want["isZero"]
    res = curve.Parallel.checkPoints(out)
    assert res.ok and res.offCurve == 0 and res.offSubgroup == 0
    if weier:
        for glv in (0, 1):   # (glv = 1: the copies are made from the new set's endomorphism images too)
            pre = curve.Parallel.precomputePoints(out, n, {"glv": glv}, 2)
            assert _strip(curve.Parallel.msm(t, pre, n)["result"]) == want, glv
            pre.free()
    for a in (pts, s, t, st_, out):
        a.free()


@pytest.mark.parametrize("label", M.ALL)
def test_closed_form(curves, label):
    """randomPointsFast has known a_i (P_i = [a_i]G) and randomScalars known s_i: the sum of mulPoints(s, P) ==
    [sum s_i a_i mod q] G"""
    curve, params = curves(label), P.CURVES[label]
    n, q = 1 << 12, params["order"]
    pts = curve.Parallel.randomPointsFast(n, 41)
    s = curve.Parallel.randomScalars(n, 42)
    ones = curve.Parallel.scalarsFromBigints([1] * n)
    out = curve.Parallel.mulPoints(s, pts)
    k = sum(prng.scalar(42, i, q) * prng.point_multiplier(41, i) for i in range(n)) % q
    want = M.canon(params, U.scale(params, k, U.generator(params)))
    got = _strip(curve.Parallel.msm(ones, out, n)["result"])
    assert M.canon(params, got) == want
    for a in (pts, s, ones, out):
        a.free()


# ---------------------------------------------------------------------------------------------- errors
def _small_mul_is_correct(curve, params):
    n = 65
    pts = curve.Parallel.randomPointsFast(n, 5)
    u = 0x1234567 % params["order"]
    st, h = _mul(curve, pts, n, u)
    assert st == 0
    out, got = _download(curve, h, n)
    p = [_strip(x) for x in curve.Affine.toBigints(pts)]
    assert got[0] == M.expected(params, u, p[0]) and got[64] == M.expected(params, u, p[64])
    out.free(); pts.free()


@pytest.mark.parametrize("label", M.ALL)
def test_scalar_out_of_range(curves, label):
    """MSMZ_ERR_RANGE and no handle: the broadcast scalar >= q (host check), and a RESIDENT scalar >= q, which only the
    kernel can find.  Uploads and imports refuse such a value, but msmz_import_scalars_into converts before it reports:
    after its MSMZ_ERR_RANGE the refused value is what the existing handle holds (read back below), so that is the
    route by which a value >= q becomes resident.  The context stays usable."""
    from msm_zprize_amd._native import MsmzSrc
    curve, params = curves(label), P.CURVES[label]
    q, n = params["order"], 257
    pts = curve.Parallel.randomPointsFast(n, 6)
    for bad in (q, q + 1, (1 << 256) - 1):
        assert _mul(curve, pts, n, bad) == (MSMZ_ERR_RANGE, 0)
    h = C.c_uint64()
    assert _lib().msmz_alloc_scalars(curve._ctx, n, C.byref(h)) == 0
    from msm_zprize_amd.parallel import DeviceArray
    sc = DeviceArray(curve, h.value, n, "scalars")
    rng = random.Random(9)
    good = M.encode_scalars([rng.randrange(q) for _ in range(n)])
    src = MsmzSrc(C.cast(C.c_char_p(good), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, sc.handle, 0, C.byref(src), n) == 0
    st, hh = _mul(curve, pts, n, sc)
    assert st == 0
    _lib().msmz_free(curve._ctx, hh)
    raw = M.encode_scalars([q])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, sc.handle, 200, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert curve.Scalar.toBigints(sc, 200, 1) == [q]   # resident all the same
    assert _mul(curve, pts, n, sc) == (MSMZ_ERR_RANGE, 0)
    for cnt, fs in ((50, 201), (200, 0)):   # ranges clear of it work: the context stays usable
        st, hh = _mul(curve, pts, cnt, sc, fs=fs)
        assert st == 0 and hh != 0
        assert _lib().msmz_free(curve._ctx, hh) == 0
    _small_mul_is_correct(curve, params)
    sc.free(); pts.free()


@pytest.mark.parametrize("label", M.ALL)
def test_argument_errors(curves, label):
    from msm_zprize_amd._native import MsmzMul
    curve, params = curves(label), P.CURVES[label]
    n = 300
    pts = curve.Parallel.randomPointsFast(n, 2)
    sc = curve.Parallel.randomScalars(n, 2)
    f = _lib().msmz_points_mul
    h = C.c_uint64(0)
    one = (1).to_bytes(32, "little")
    assert f(None, C.byref(MsmzMul(pts.handle, 0, 0, 0, one, 0, 0)), n, C.byref(h)) == MSMZ_ERR_ARG     # null context
    assert f(curve._ctx, None, n, C.byref(h)) == MSMZ_ERR_ARG                                          # null descriptor
    assert f(curve._ctx, C.byref(MsmzMul(pts.handle, 0, 0, 0, one, 0, 0)), n, None) == MSMZ_ERR_ARG     # null out_handle
    cases = [
        (pts, 0, 1, None, 0, 0, 0),              # n == 0
        (0xDEAD, n, 1, None, 0, 0, 0),           # unknown handles
        (pts, n, 1, 0xDEAD, 0, 0, 0),
        (sc.handle, n, 1, None, 0, 0, 0),        # handles of the wrong kind
        (pts, n, 1, sc.handle, 0, 0, 0),
        (pts, n, None, None, 0, 0, 0),           # scalars_handle == 0 with a null scalar
        (pts, n, 1, None, 1, 0, 0),              # ranges beyond their sets
        (pts, 1, 1, None, n, 0, 0),
        (pts, 2, 1, None, (1 << 64) - 1, 0, 0),  # first + n wraps
        (pts, n, sc, None, 0, 1, 0),
        (pts, 2, sc, None, 0, (1 << 64) - 1, 0),
        (pts, n, 1, pts, 0, 0, 1),
        (pts, 2, 1, pts, 0, 0, (1 << 64) - 1),
        (pts, n + 1, sc, pts, 0, 0, 0),
        (pts, 1 << 30, 1, None, 0, 0, 0),        # n beyond the record-index limit
    ]
    for p, cnt, s, a, fp, fs, fq in cases:
        assert _mul(curve, p, cnt, s, a, fp, fs, fq) == (MSMZ_ERR_ARG, 0), (cnt, fp, fs, fq)
    from msm_zprize_amd.parallel import DeviceArray
    scalars_as_points = DeviceArray(curve, pts.handle, n, "scalars")
    assert _mul(curve, pts, n, scalars_as_points)[0] == MSMZ_ERR_ARG   # a point handle where scalars belong
    _small_mul_is_correct(curve, params)
    if params["kind"] == "weierstrass":
        pre = curve.Parallel.precomputePoints(pts, n, {"c": 8}, 2)
        assert _mul(curve, pre, n, 1) == (MSMZ_ERR_UNSUPPORTED, 0)
        assert _mul(curve, pts, n, sc, pre) == (MSMZ_ERR_UNSUPPORTED, 0)
        pre.free()
        _small_mul_is_correct(curve, params)
    # the Python surface refuses before the library is asked
    with pytest.raises(ValueError):
        curve.Parallel.mulPoints(params["order"], pts)
    with pytest.raises(ValueError):
        curve.Parallel.mulPoints(sc, pts, n, None, 1)
    out = curve.Parallel.mulPoints(sc, pts, 10, pts, firstPoint=5, firstScalar=7, firstAddend=9)
    p = [_strip(x) for x in curve.Affine.toBigints(pts, 0, 32)]
    s = curve.Scalar.toBigints(sc, 0, 32)
    assert [_strip(x) for x in curve.Affine.toBigints(out)] == [M.expected(params, s[7 + i], p[5 + i], p[9 + i]) for i in range(10)]
    out.free(); pts.free(); sc.free()


# ---------------------------------------------------------------------------------------------- multi-engine contexts
@pytest.mark.parametrize("label", M.ALL)
def test_multi_engine_context(mod, curves, label):
    """devices = [0, 0]: every engine multiplies its share (blocks 0 and 2 / block 1 of 2^17 + 5 points); the downloaded
    bytes equal the single-engine ones; a non-zero first is refused"""
    params = P.CURVES[label]
    single = curves(label)
    fb = params["fe_bytes"]
    n = (1 << 17) + 5
    u = random.Random(3).randrange(1, params["order"])

    def run(curve):
        pts = curve.Parallel.randomPointsFast(n, 51)
        add = curve.Parallel.randomPointsFast(n, 52)
        sc = curve.Parallel.randomScalars(n, 53)
        outs = []
        for args in ((sc, add), (u, None)):
            st, h = _mul(curve, pts, n, *args)
            assert st == 0
            data, inf = C.create_string_buffer(2 * fb * n), C.create_string_buffer(n)
            assert _lib().msmz_download_points(curve._ctx, h, 0, n, data, inf) == 0
            outs.append((data.raw, inf.raw))
            assert _lib().msmz_free(curve._ctx, h) == 0
        refused = [_mul(curve, pts, 10, sc, add, fp=1), _mul(curve, pts, 10, sc, add, fs=1), _mul(curve, pts, 10, sc, add, fq=1),
                   _mul(curve, pts, 10, u, None, fp=1 << 16)]
        for a in (pts, add, sc):
            a.free()
        return outs, refused

    want, ok = run(single)
    assert all(st == 0 for st, _ in ok)
    for _, h in ok:
        _lib().msmz_free(single._ctx, h)
    assert want[0] != want[1] and any(want[0][0])
    mod.startThreads(devices=[0, 0])
    mparams = mod.curves.BY_LABEL[label]
    multi = (mod.Weierstrass if mparams["kind"] == "weierstrass" else mod.TwistedEdwards).create(mparams)
    try:
        got, refused = run(multi)
        assert got == want
        assert refused == [(MSMZ_ERR_UNSUPPORTED, 0)] * 4
    finally:
        multi.close()
        mod.startThreads()

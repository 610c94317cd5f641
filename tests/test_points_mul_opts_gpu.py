"""msmz_points_mul_opts on the GPU (k_points_mul with a bit bound, k_points_mul_glv; csrc/mul_kernels.h): downloads
against the oracle's [s]P (+ Q) and, byte for byte, against the plain msmz_points_mul, at the sizes that exercise both
whole-wave inversions; the bound's errors; points outside the subgroup under the vouch; the IPA fold; the result as an
ordinary point set; the curve without an endomorphism; argument errors; a two-engine context."""
import ctypes as C
import random

import pytest

import check_points_util as U
import points_mul_opts_util as O
import points_mul_util as M
from oracle import bigint_ref as B
from oracle import params as P

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_RANGE = 1, 6
SIZES = [1, 63, 64, 65, 257]   # a partial wave, a full wave, a wave plus one lane, several blocks with a ragged tail
SUB = O.MSMZ_MUL_SUBGROUP


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


def _mul(curve, points, n, scalars, addend=None, fp=0, fs=0, fq=0, flags=0, bits=0, reserved=(0, 0), opts=True):
    """msmz_points_mul_opts (opts=False: msmz_points_mul) through the C ABI -> (status, handle).  scalars: a resident
    array or an int (broadcast)"""
    from msm_zprize_amd._native import MsmzMul, MsmzMulOpts
    raw = None if hasattr(scalars, "handle") else int(scalars).to_bytes(32, "little")
    m = MsmzMul(points.handle, fp, scalars.handle if hasattr(scalars, "handle") else 0, fs, raw,
                0 if addend is None else addend.handle, fq)
    h = C.c_uint64(0)
    if not opts:
        return _lib().msmz_points_mul(curve._ctx, C.byref(m), n, C.byref(h)), h.value
    o = MsmzMulOpts(flags, bits, (C.c_int32 * 2)(*reserved))
    return _lib().msmz_points_mul_opts(curve._ctx, C.byref(m), n, C.byref(o), C.byref(h)), h.value


def _raw(curve, params, handle, n):
    """(x | y bytes, infinity flags) of a result, which is then freed"""
    fb = params["fe_bytes"]
    data, inf = C.create_string_buffer(2 * fb * n), C.create_string_buffer(n)
    assert _lib().msmz_download_points(curve._ctx, handle, 0, n, data, inf) == 0
    assert _lib().msmz_free(curve._ctx, handle) == 0
    return data.raw, inf.raw


def _encode(params, pts):
    """oracle points as msmz_download_points gives them: canonical bytes, the all-zero record and flag for infinity"""
    fb = params["fe_bytes"]
    weier = params["kind"] == "weierstrass"
    data = b"".join(bytes(2 * fb) if weier and q["isZero"] else q["x"].to_bytes(fb, "little") + q["y"].to_bytes(fb, "little")
                    for q in pts)
    return data, bytes(1 if weier and q["isZero"] else 0 for q in pts)


def _decode(params, raw):
    fb = params["fe_bytes"]
    data, inf = raw
    return [U.pt(int.from_bytes(data[2 * fb * i:2 * fb * i + fb], "little"),
                 int.from_bytes(data[2 * fb * i + fb:2 * fb * (i + 1)], "little"), bool(inf[i])) for i in range(len(inf))]


_scaled = {}


def _scale(label, s, p):
    """[s]P by the oracle, once per (s, P): the sets draw their points from a small pool"""
    key = (label, s, p["x"], p["y"], p["isZero"])
    if key not in _scaled:
        _scaled[key] = U.scale(P.CURVES[label], s, p)
    return _scaled[key]


def _expected(label, s, p, q=None):
    params = P.CURVES[label]
    r = _scale(label, s, p)
    return M.canon(params, r if q is None else U.add(params, r, q))


def _broadcast_scalars(label):
    q = P.CURVES[label]["order"]
    rng = random.Random(O.ALL.index(label) + 5)
    special = [1, O.lam(label), q - 1, q - O.lam(label)] if label in O.WEIER else [1, 2, q - 1, q - 2]
    return special + [rng.randrange(q) for _ in range(4)]


_sets = {}


def _reference(label, n):
    """the rows of one set of subgroup points and the oracle's answers, computed once per (curve, size)"""
    if (label, n) not in _sets:
        rows = O.subgroup_set(label, n, 2000 * O.ALL.index(label) + n)
        _sets[(label, n)] = dict(
            rows=rows, plain=_encode(P.CURVES[label], [_expected(label, s, p) for s, p, _ in rows]),
            added=_encode(P.CURVES[label], [_expected(label, s, p, q) for s, p, q in rows]),
            bcast={u: _encode(P.CURVES[label], [_expected(label, u, p, q) for _, p, q in rows]) for u in _broadcast_scalars(label)})
    return _sets[(label, n)]


# ---------------------------------------------------------------------------------------------- bit-exact downloads
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("label", O.ALL)
def test_subgroup_downloads_equal_the_oracle_and_the_plain_call(curves, label, n):
    """under MSMZ_MUL_SUBGROUP, records and infinity flags of [s_i]P_i, [s_i]P_i + Q_i and [u]P_i + Q_i (u over 1,
    lambda, q - 1, q - lambda and 4 random) == the oracle's AND == what msmz_points_mul downloads, byte for byte; the
    sets hold s = 0, 1, q - 1, P and Q at infinity and Q = +-[s]P in the first wave and in the last one, and per-lane
    scalars of both sign cases in every wave"""
    curve, params, ref = curves(label), P.CURVES[label], _reference(label, n)
    rows = ref["rows"]
    pa = curve.Parallel.pointsFromBigints([p for _, p, _ in rows])
    qa = curve.Parallel.pointsFromBigints([q for _, _, q in rows])
    sa = curve.Parallel.scalarsFromBigints([s for s, _, _ in rows])
    modes = [("resident", (sa, None), ref["plain"]), ("addend", (sa, qa), ref["added"])]
    modes += [(f"broadcast {u:x}", (u, qa), want) for u, want in ref["bcast"].items()]
    for mode, args, want in modes:
        st, h = _mul(curve, pa, n, *args, flags=SUB)
        assert st == 0, (mode, st)
        got = _raw(curve, params, h, n)
        st, h = _mul(curve, pa, n, *args, opts=False)
        assert st == 0, (mode, st)
        plain = _raw(curve, params, h, n)
        bad = [i for i in range(n) if _decode(params, got)[i] != _decode(params, want)[i]] if got != want else []
        assert got == want, (mode, bad[:3])
        assert got == plain, mode
    pa.free(); qa.free(); sa.free()


# ---------------------------------------------------------------------------------------------- scalar_bits
@pytest.mark.parametrize("label", O.ALL)
def test_scalar_bits(curves, label):
    """b in 1, 32, 33, 64, 128, 129, 200 with scalars below 2^b, min(2^b, q) - 1 among them: the oracle's points, with
    and without the vouch (b = 64 with it: still the plain chain); a resident scalar equal to 2^b in the last wave:
    MSMZ_ERR_RANGE, no handle, and the next call succeeds; a broadcast scalar >= 2^b: MSMZ_ERR_RANGE"""
    curve, params = curves(label), P.CURVES[label]
    q, n = params["order"], 65
    rng = random.Random(O.ALL.index(label) + 31)
    g = U.generator(params)
    pool = [U.scale(params, rng.randrange(1, q), g) for _ in range(4)]
    pts = [pool[i % 4] for i in range(n)]
    pa = curve.Parallel.pointsFromBigints(pts)
    for b in (1, 32, 33, 64, 128, 129, 200):
        top = min(1 << b, q)
        special = O.bounded_scalars(label, b, rng, 0)
        assert top - 1 in special
        scalars = [special[i % len(special)] if i < 8 or i == n - 1 else rng.randrange(top) for i in range(n)]
        scalars[n - 1] = top - 1   # (the one lane of the last wave)
        want = _encode(params, [_expected(label, s, p) for s, p in zip(scalars, pts)])
        sa = curve.Parallel.scalarsFromBigints(scalars)
        u = top - 1
        want_u = _encode(params, [_expected(label, u, p) for p in pts])
        for flags in (0, SUB):
            st, h = _mul(curve, pa, n, sa, flags=flags, bits=b)
            assert st == 0, (b, flags)
            assert _raw(curve, params, h, n) == want, (b, flags)
            st, h = _mul(curve, pa, n, u, flags=flags, bits=b)
            assert st == 0, (b, flags)
            assert _raw(curve, params, h, n) == want_u, (b, flags)
        sa.free()
        scalars[n - 1] = 1 << b   # below q for every b here, so an upload takes it
        bad = curve.Parallel.scalarsFromBigints(scalars)
        for flags in (0, SUB):
            assert _mul(curve, pa, n, bad, flags=flags, bits=b) == (MSMZ_ERR_RANGE, 0), (b, flags)
            st, h = _mul(curve, pa, n - 1, bad, flags=flags, bits=b)   # a range clear of it: the context stays usable
            assert st == 0 and h != 0
            assert _raw(curve, params, h, n - 1) == tuple(w[:len(w) * (n - 1) // n] for w in want)
            for s in (1 << b, (1 << b) + 1, q - 1):
                assert _mul(curve, pa, n, s, flags=flags, bits=b) == (MSMZ_ERR_RANGE, 0), (b, flags, s)
        st, h = _mul(curve, pa, n, bad, bits=b + 1)   # and the same set under a bound it keeps
        assert st == 0
        assert _lib().msmz_free(curve._ctx, h) == 0
        bad.free()
    for b in (O.order_bits(label), 256):   # no bound at all: q - 1 passes
        st, h = _mul(curve, pa, n, q - 1, bits=b, flags=SUB)
        assert st == 0
        assert _raw(curve, params, h, n) == _encode(params, [_expected(label, q - 1, p) for p in pts])
    pa.free()


# ---------------------------------------------------------------------------------------------- outside the subgroup
@pytest.mark.parametrize("label", [label for label in O.WEIER if P.CURVES[label]["cofactor"] != 1])
def test_points_outside_the_subgroup_under_the_vouch(curves, label):
    """the order-3 point with x = 0 and another named small-order point among good points of one wave, per-lane scalars
    and a broadcast one: the call returns 0, every other row is the oracle's, the planted rows download as infinity or
    as a point of the curve"""
    curve, params = curves(label), P.CURVES[label]
    q, n = params["order"], 65
    named = M.on_curve_named(label)
    zero_x = [p for p in named if p["x"] == 0][0]
    other = [p for p in named if p["x"] != 0 and U.verdict(params, p) == U.OFF_SUBGROUP][0]
    planted = {3: zero_x, 4: other, 40: zero_x, 41: other}
    rng = random.Random(17)
    g = U.generator(params)
    pool = [U.scale(params, rng.randrange(1, q), g) for _ in range(4)]
    pts = [planted.get(i, pool[i % 4]) for i in range(n)]
    scalars = [rng.randrange(q) for _ in range(n)]
    pa = curve.Parallel.pointsFromBigints(pts)
    sa = curve.Parallel.scalarsFromBigints(scalars)
    aw = B.AffineWeierstrass(params)
    # a broadcast scalar of each sign case (the unequal one runs the shared inversion with the x = 0 lanes in it)
    for args, ss in [((sa,), scalars), ((O.lam(label) - 1,), None), ((O.lam(label) + 1,), None), ((scalars[0],), None)]:
        st, h = _mul(curve, pa, n, *args, flags=SUB)
        assert st == 0
        got = _decode(params, _raw(curve, params, h, n))
        for i in range(n):
            s = ss[i] if ss else args[0]
            if i in planted:
                assert got[i]["isZero"] or aw.is_on_curve((got[i]["x"], got[i]["y"], False)), i
            else:
                assert got[i] == _expected(label, s, pts[i]), i
    pa.free(); sa.free()


# ---------------------------------------------------------------------------------------------- the IPA fold
@pytest.mark.parametrize("label", O.ALL)
def test_ipa_fold_with_a_128_bit_challenge(curves, label):
    """G'_i = G_lo,i + [u] G_hi,i over the halves of ONE handle, u below 2^128, scalar_bits = 128 and the vouch"""
    curve, params = curves(label), P.CURVES[label]
    n = 128
    gens = curve.Parallel.randomPointsFast(n, 31)
    g = [U.pt(p["x"], p["y"], bool(p.get("isZero", False))) for p in curve.Affine.toBigints(gens)]
    u = random.Random(6).randrange(1 << 127, 1 << 128)
    st, h = _mul(curve, gens, n // 2, u, gens, fp=n // 2, fq=0, flags=SUB, bits=128)
    assert st == 0
    want = _encode(params, [M.expected(params, u, g[n // 2 + i], g[i]) for i in range(n // 2)])
    assert _raw(curve, params, h, n // 2) == want
    out = curve.Parallel.mulPoints(u, gens, n // 2, gens, firstPoint=n // 2, scalarBits=128, subgroup=True)
    assert _raw(curve, params, out.handle, n // 2) == want
    gens.free()


# ---------------------------------------------------------------------------------------------- the result as a set
@pytest.mark.parametrize("label", O.WEIER)
def test_result_is_an_ordinary_point_set(curves, label):
    """msm(t, mulPoints(s, P, subgroup=True)) == msm(s t mod q, P) with GLV on (the endomorphism images of the new set are
    read) and off"""
    curve, params = curves(label), P.CURVES[label]
    n, q = 1 << 10, params["order"]
    pts = curve.Parallel.randomPointsFast(n, 11)
    s = curve.Parallel.randomScalars(n, 12)
    t = curve.Parallel.randomScalars(n, 13)
    st_ = curve.Parallel.scalarsFromBigints([a * b % q for a, b in zip(curve.Scalar.toBigints(s), curve.Scalar.toBigints(t))])
    out = curve.Parallel.mulPoints(s, pts, subgroup=True)
    assert len(out) == n and out.kind == "points"
    for glv in (1, 0):
        a = curve.Parallel.msm(t, out, n, False, {"glv": glv})["result"]
        b = curve.Parallel.msm(st_, pts, n, False, {"glv": glv})["result"]
        assert (a["x"], a["y"], bool(a.get("isZero"))) == (b["x"], b["y"], bool(b.get("isZero"))), glv
        assert not a.get("isZero")
    for a in (pts, s, t, st_, out):
        a.free()


# ---------------------------------------------------------------------------------------------- no endomorphism
def test_twisted_edwards_takes_the_vouch_and_changes_nothing(curves):
    label = "ed-on-bls12-377"
    curve, params = curves(label), P.CURVES[label]
    n = 257
    pts = curve.Parallel.randomPointsFast(n, 21)
    add = curve.Parallel.randomPointsFast(n, 22)
    sc = curve.Parallel.randomScalars(n, 23)
    for args in ((sc, add), (random.Random(1).randrange(params["order"]), None)):
        st, h = _mul(curve, pts, n, *args, flags=SUB)
        assert st == 0
        st, h2 = _mul(curve, pts, n, *args, opts=False)
        assert st == 0
        assert _raw(curve, params, h, n) == _raw(curve, params, h2, n)
    for a in (pts, add, sc):
        a.free()


# ---------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("label", O.ALL)
def test_argument_errors(curves, label):
    """unknown flag bits, a non-zero reserved word, scalar_bits of -1 and 257: MSMZ_ERR_ARG and no handle; NULL options
    are msmz_points_mul; the Python surface refuses before the library is asked"""
    from msm_zprize_amd._native import MsmzMul
    curve, params = curves(label), P.CURVES[label]
    n = 65
    pts = curve.Parallel.randomPointsFast(n, 2)
    sc = curve.Parallel.randomScalars(n, 2)
    for kw in (dict(flags=2), dict(flags=SUB | 4), dict(flags=0x80000000), dict(reserved=(1, 0)), dict(reserved=(0, -1)),
               dict(bits=-1), dict(bits=257), dict(flags=SUB, bits=1 << 20)):
        assert _mul(curve, pts, n, sc, **kw) == (MSMZ_ERR_ARG, 0), kw
        assert _mul(curve, pts, n, 1, **kw) == (MSMZ_ERR_ARG, 0), kw
    m = MsmzMul(pts.handle, 0, sc.handle, 0, None, 0, 0)
    h = C.c_uint64(0)
    assert _lib().msmz_points_mul_opts(curve._ctx, C.byref(m), n, None, C.byref(h)) == 0
    null_opts = _raw(curve, params, h.value, n)
    st, hh = _mul(curve, pts, n, sc, opts=False)
    assert st == 0 and _raw(curve, params, hh, n) == null_opts
    for kw in (dict(scalarBits=-1), dict(scalarBits=257), dict(scalarBits=1.0)):
        with pytest.raises(ValueError):
            curve.Parallel.mulPoints(sc, pts, **kw)
    with pytest.raises(ValueError):
        curve.Parallel.mulPoints(1 << 64, pts, scalarBits=64)
    with pytest.raises(TypeError):
        curve.Parallel.mulPoints(sc, pts, subgroup=1)
    with pytest.raises(RuntimeError):   # a resident scalar beyond the bound: the library's MSMZ_ERR_RANGE
        curve.Parallel.mulPoints(sc, pts, scalarBits=8)
    out = curve.Parallel.mulPoints(sc, pts, scalarBits=255, subgroup=True)   # the context stays usable
    st, hh = _mul(curve, pts, n, sc, opts=False)
    assert st == 0 and _raw(curve, params, hh, n) == _raw(curve, params, out.handle, n)
    pts.free(); sc.free()


# ---------------------------------------------------------------------------------------------- multi-engine contexts
@pytest.mark.parametrize("label", ["bls12-377", "ed-on-bls12-377"])
def test_two_engine_context_takes_the_options(mod, curves, label):
    """devices = [0, 0]: both engines get the options (block 0 / the 5 points of block 1 of 2^16 + 5); the downloaded
    bytes equal the single-engine ones and the plain call's; a broken bound on the second engine's share fails the call"""
    params = P.CURVES[label]
    single = curves(label)
    n = (1 << 16) + 5
    u = random.Random(3).randrange(1 << 127, 1 << 128)

    def run(curve):
        pts = curve.Parallel.randomPointsFast(n, 51)
        add = curve.Parallel.randomPointsFast(n, 52)
        sc = curve.Parallel.randomScalars(n, 53)
        outs = []
        for args, kw in (((sc, add), dict(flags=SUB)), ((u, None), dict(flags=SUB, bits=128)), ((sc, add), dict(opts=False))):
            st, h = _mul(curve, pts, n, *args, **kw)
            assert st == 0
            outs.append(_raw(curve, params, h, n))
        refused = [_mul(curve, pts, n, sc, add, flags=SUB, bits=200), _mul(curve, pts, n, u, None, bits=127),
                   _mul(curve, pts, n, sc, None, flags=2)]
        for a in (pts, add, sc):
            a.free()
        return outs, refused

    want, refused = run(single)
    assert want[0] == want[2] and want[0] != want[1] and any(want[0][0])
    assert refused == [(MSMZ_ERR_RANGE, 0), (MSMZ_ERR_RANGE, 0), (MSMZ_ERR_ARG, 0)]
    mod.startThreads(devices=[0, 0])
    mparams = mod.curves.BY_LABEL[label]
    multi = (mod.Weierstrass if mparams["kind"] == "weierstrass" else mod.TwistedEdwards).create(mparams)
    try:
        got, refused = run(multi)
        assert got == want
        assert refused == [(MSMZ_ERR_RANGE, 0), (MSMZ_ERR_RANGE, 0), (MSMZ_ERR_ARG, 0)]
    finally:
        multi.close()
        mod.startThreads()

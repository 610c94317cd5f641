"""msmz_check_points on the GPU (k_check_curve / k_check_subgroup and their twisted-Edwards twins, csrc/check_kernels.h):
every verdict byte, both counts and first_bad against the oracle's verdicts (tests/check_points_util.py), on generated
sets, on sets with planted bad points, on sub-ranges, through every input route, on multi-engine contexts, through the
Python surface, and the argument errors.  No test passes a pointer the engine would have to refuse at a kernel."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

import check_points_util as U
from oracle import c_oracle
from oracle import params as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIER = U.ALL[:3]
CURVE, SUBGROUP, BOTH = 1, 2, 3
MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED = 1, 4
N_PLANTED = 1 << 14


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


def _check(curve, arr, first, count, what, want_verdicts=True):
    """msmz_check_points -> (status, (off_curve, off_subgroup, first_bad), verdict list)"""
    from msm_zprize_amd._native import MsmzCheckResult
    res = MsmzCheckResult()
    buf = C.create_string_buffer(max(count, 1)) if want_verdicts else None
    st = _lib().msmz_check_points(curve._ctx, arr.handle, first, count, what, C.byref(res), buf)
    return st, (res.off_curve, res.off_subgroup, res.first_bad), (list(buf.raw[:count]) if want_verdicts and st == 0 else None)


def _strip(p):
    return {"x": p["x"], "y": p["y"], "isZero": bool(p.get("isZero", False))}


@pytest.fixture(scope="module")
def planted(curves):
    """per curve: a generated set of 2^14 with ~40 planted points, and the verdict the oracle gives EVERY point of it (the
    planted ones by the Python oracle, the generated ones by the C oracle's scalar multiplication)"""
    cache = {}

    def get(label):
        if label not in cache:
            curve, params = curves(label), P.CURVES[label]
            gen = curve.Parallel.randomPointsFast(N_PLANTED, 77)
            good = [_strip(p) for p in curve.Affine.toBigints(gen)]
            gen.free()
            pts, where = U.planted_set(label, good)
            want = [U.verdict(params, q) if i in set(where) else U.verdict_fast(params, q) for i, q in enumerate(pts)]
            cache[label] = dict(pts=pts, where=where, want=want)
        return cache[label]

    return get


def _upload(curve, params, pts, montgomery=False):
    data, inf = U.encode(params, pts, montgomery)
    return curve.Parallel.pointsFromBytes(data, len(pts), inf, montgomery=montgomery)


def _small_msm_is_correct(curve, params):
    n = 300
    pts = curve.Parallel.randomPointsFast(n, 5)
    rng = random.Random(8)
    s = [rng.randrange(params["order"]) for _ in range(n)]
    want = _strip(c_oracle.msm(params, s, [_strip(p) for p in curve.Affine.toBigints(pts)]))
    sc = curve.Parallel.scalarsFromBigints(s)
    assert _strip(curve.Parallel.msm(sc, pts, n)["result"]) == want
    pts.free(); sc.free()


# ---------------------------------------------------------------------------------------------- all-good sets
@pytest.mark.parametrize("label,logn", [(l, 16) for l in U.ALL] + [("bls12-377", 20)])
def test_generated_set_is_good(curves, label, logn):
    curve, n = curves(label), 1 << logn
    arr = curve.Parallel.randomPointsFast(n, 3)
    for what in (CURVE, BOTH):
        st, res, v = _check(curve, arr, 0, n, what)
        print(label, logn, what, res)
        assert st == 0 and res == (0, 0, U.NO_INDEX)
        assert v == [0] * n
    st, res, _ = _check(curve, arr, 0, n, BOTH, want_verdicts=False)   # verdicts is nullable
    assert st == 0 and res == (0, 0, U.NO_INDEX)
    arr.free()


# ---------------------------------------------------------------------------------------------- planted sets
@pytest.mark.parametrize("label", U.ALL)
def test_planted_set(curves, planted, label):
    curve, params, pl = curves(label), P.CURVES[label], planted(label)
    want = pl["want"]
    assert any(v == U.OFF_CURVE for v in want) and (params["cofactor"] == 1 or any(v == U.OFF_SUBGROUP for v in want))
    assert all(want[i] == 0 for i in range(len(want)) if i not in set(pl["where"]))
    arr = _upload(curve, params, pl["pts"])
    st, res, v = _check(curve, arr, 0, len(want), BOTH)
    print(label, res, U.summary(want))
    assert st == 0
    assert v == want
    assert res == U.summary(want)
    # MSMZ_CHECK_SUBGROUP alone implies the curve check
    st, res2, v2 = _check(curve, arr, 0, len(want), SUBGROUP)
    assert st == 0 and v2 == want and res2 == res
    # a second run gives the same answer (atomic counts, atomic min)
    assert _check(curve, arr, 0, len(want), BOTH) == (0, res, want)
    arr.free()


@pytest.mark.parametrize("label", U.ALL)
def test_sub_ranges(curves, planted, label):
    """a bad point just inside and just outside either end of the range; first_bad is an index of the set"""
    curve, params, pl = curves(label), P.CURVES[label], planted(label)
    want, n = pl["want"], len(pl["want"])
    bad = [i for i, v in enumerate(want) if v]
    arr = _upload(curve, params, pl["pts"])
    ranges = [(0, 1), (n - 1, 1), (1, n - 2), (0, n - 1), (1, n - 1)]
    for b in [i for i in bad if 2 <= i < n - 2][:6]:
        ranges += [(b, 300), (b + 1, 300), (max(0, b - 299), 300), (max(0, b - 300), 300), (b, 1), (b - 1, 1), (b + 1, 1)]
    for first, count in ranges:
        count = min(count, n - first)
        st, res, v = _check(curve, arr, first, count, BOTH)
        assert st == 0, (first, count)
        assert v == want[first:first + count], (first, count)
        assert res == U.summary(want[first:first + count], first), (first, count)
    arr.free()


@pytest.mark.parametrize("label", U.ALL)
def test_curve_check_alone(curves, planted, label):
    """what = MSMZ_CHECK_CURVE: no subgroup verdicts, bit 1 stays clear"""
    curve, params, pl = curves(label), P.CURVES[label], planted(label)
    want = [v & U.OFF_CURVE for v in pl["want"]]
    arr = _upload(curve, params, pl["pts"])
    st, res, v = _check(curve, arr, 0, len(want), CURVE)
    assert st == 0 and v == want and res == U.summary(want) and res[1] == 0
    arr.free()


def test_pallas_subgroup_is_the_curve(curves, planted):
    """cofactor 1: MSMZ_CHECK_SUBGROUP gives what MSMZ_CHECK_CURVE gives, verdicts and counts (no chain is run)"""
    curve, params, pl = curves("pallas"), P.PALLAS, planted("pallas")
    arr = _upload(curve, params, pl["pts"])
    a = _check(curve, arr, 0, len(pl["pts"]), CURVE)
    b = _check(curve, arr, 0, len(pl["pts"]), BOTH)
    assert a == b and a[0] == 0 and a[1][1] == 0 and a[1][0] > 0
    arr.free()


# ---------------------------------------------------------------------------------------------- input routes
@pytest.mark.parametrize("label", U.ALL)
def test_input_routes_host(curves, planted, label):
    """msmz_upload_points (GLV images follow the base points on the Weierstrass curves) and msmz_import_points from host
    memory in Montgomery form leave the same verdict bytes"""
    curve, params, pl = curves(label), P.CURVES[label], planted(label)
    n = len(pl["pts"])
    for montgomery in (False, True):
        arr = _upload(curve, params, pl["pts"], montgomery)
        st, res, v = _check(curve, arr, 0, n, BOTH)
        assert st == 0 and v == pl["want"] and res == U.summary(pl["want"]), montgomery
        if params["kind"] == "weierstrass":   # only the n base points are checked and indexed, not the images behind them
            assert _check(curve, arr, n, 1, BOTH)[0] == MSMZ_ERR_ARG
            assert _check(curve, arr, 0, n + 1, BOTH)[0] == MSMZ_ERR_ARG
        arr.free()


def test_input_route_device_tensor():
    """the same planted points from a device tensor, canonical and Montgomery, in a child process that loads torch
    first (the pattern of tests/test_scalar_import_gpu.py)"""
    cases = os.path.join(ROOT, "tests", "check_points_gpu_cases.py")
    code = ("import sys, torch, pytest; "
            "sys.exit(pytest.main([%r, '-x', '-q', '-p', 'no:cacheprovider']))" % cases)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900,
                       stdin=subprocess.DEVNULL)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]


# ---------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("label", U.ALL)
def test_argument_errors(curves, label):
    from msm_zprize_amd._native import MsmzCheckResult
    curve, params = curves(label), P.CURVES[label]
    n = 1000
    arr = curve.Parallel.randomPointsFast(n, 2)
    sc = curve.Parallel.randomScalars(n, 2)
    res = MsmzCheckResult()
    buf = C.create_string_buffer(n)
    f = _lib().msmz_check_points
    cases = [
        (None, arr.handle, 0, n, BOTH, C.byref(res)),            # null context
        (curve._ctx, arr.handle, 0, n, BOTH, None),              # null out
        (curve._ctx, 0xDEAD, 0, n, BOTH, C.byref(res)),          # unknown handle
        (curve._ctx, sc.handle, 0, n, BOTH, C.byref(res)),       # a scalar handle
        (curve._ctx, arr.handle, 0, 0, BOTH, C.byref(res)),      # count == 0
        (curve._ctx, arr.handle, 1, n, BOTH, C.byref(res)),      # first + count beyond the set
        (curve._ctx, arr.handle, n, 1, BOTH, C.byref(res)),
        (curve._ctx, arr.handle, n + 1, 1, BOTH, C.byref(res)),
        (curve._ctx, arr.handle, (1 << 64) - 1, 2, BOTH, C.byref(res)),   # first + count wraps
        (curve._ctx, arr.handle, 0, n, 0, C.byref(res)),         # what == 0
        (curve._ctx, arr.handle, 0, n, 4, C.byref(res)),         # unknown bits
        (curve._ctx, arr.handle, 0, n, 7, C.byref(res)),
    ]
    for ctx, h, first, count, what, out in cases:
        assert f(ctx, h, first, count, what, out, buf) == MSMZ_ERR_ARG, (h, first, count, what)
        _small_msm_is_correct(curve, params)
    if params["kind"] == "weierstrass":
        pre = curve.Parallel.precomputePoints(arr, n, {"c": 8}, 2)
        assert f(curve._ctx, pre.handle, 0, n, BOTH, C.byref(res), buf) == MSMZ_ERR_UNSUPPORTED
        _small_msm_is_correct(curve, params)
        pre.free()
    assert _check(curve, arr, 0, n, BOTH)[:2] == (0, (0, 0, U.NO_INDEX))
    arr.free(); sc.free()


# ---------------------------------------------------------------------------------------------- multi-engine contexts
@pytest.mark.parametrize("label", U.ALL)
def test_multi_engine_contexts(mod, curves, label):
    """[0, 0] and [0, 0, 0]: every engine checks its share; verdicts and first_bad equal the single-engine ones, for the
    whole set and for sub-ranges that start and end inside blocks"""
    params = P.CURVES[label]
    single = curves(label)
    fb = params["fe_bytes"]
    n = 3 * (1 << 16) + 777          # blocks 0..3: several per engine on two engines, a short last block
    gen = single.Parallel.randomPointsFast(n, 21)
    data = C.create_string_buffer(2 * fb * n)
    assert _lib().msmz_download_points(single._ctx, gen.handle, 0, n, data, None) == 0
    gen.free()
    data = bytearray(data.raw)
    bad = [q for q in U.bad_points(label, random.Random(4)) if U.verdict(params, q)]   # (the oracle's bad ones of them)
    where = [5, 65535, 65536, (1 << 17) + 9, 3 * (1 << 16), n - 1, n - 700, 40000]   # first and last block among them
    bad = [bad[k % len(bad)] for k in range(len(where))]
    for k, i in enumerate(where):
        data[2 * fb * i:2 * fb * (i + 1)] = U.encode(params, [bad[k]])[0]
    ranges = [(0, n), (6, n - 6), (65535, 2), (65536, 70000), (100, (1 << 17)), (3 * (1 << 16) - 1, 778), (n - 699, 699)]
    arr = single.Parallel.pointsFromBytes(bytes(data), n)
    want = [_check(single, arr, first, count, BOTH) for first, count in ranges]
    want_curve = _check(single, arr, 0, n, CURVE)
    arr.free()
    assert want[0][1][0] > 0 and (want[0][1][1] > 0) == (params["cofactor"] != 1) and want[0][1][2] == 5
    assert [(i, v) for i, v in enumerate(want[0][2]) if v] == sorted((w, U.verdict(params, bad[k])) for k, w in enumerate(where))
    for devices in ([0, 0], [0, 0, 0]):
        mod.startThreads(devices=devices)
        mparams = mod.curves.BY_LABEL[label]
        multi = (mod.Weierstrass if mparams["kind"] == "weierstrass" else mod.TwistedEdwards).create(mparams)
        try:
            arr = multi.Parallel.pointsFromBytes(bytes(data), n)
            for (first, count), w in zip(ranges, want):
                assert _check(multi, arr, first, count, BOTH) == w, (devices, first, count)
            assert _check(multi, arr, 0, n, CURVE) == want_curve, devices
            assert _check(multi, arr, n, 1, BOTH)[0] == MSMZ_ERR_ARG
            arr.free()
        finally:
            multi.close()
            mod.startThreads()


# ---------------------------------------------------------------------------------------------- Python surface
@pytest.mark.parametrize("label", U.ALL)
def test_python_surface(curves, planted, label):
    curve, params, pl = curves(label), P.CURVES[label], planted(label)
    want, n = pl["want"], len(pl["want"])
    arr = _upload(curve, params, pl["pts"])
    r = curve.Parallel.checkPoints(arr, verdicts=True)
    s = U.summary(want)
    assert (r.ok, r.offCurve, r.offSubgroup, r.firstBad, list(r.verdicts)) == (False, s[0], s[1], s[2], want)
    r = curve.Parallel.checkPoints(arr, 100, subgroup=False, first=200)
    s = U.summary([v & 1 for v in want[200:300]], 200)
    assert (r.offCurve, r.offSubgroup, r.firstBad, r.verdicts) == (s[0], 0, None if s[2] == U.NO_INDEX else s[2], None)
    arr.free()
    # check= on the way in: the failing set is freed again -- the handle it got is unknown afterwards, and the next
    # handle the context gives out is the one after it (handles are numbered in order)
    data, inf = U.encode(params, pl["pts"])
    probe = curve.Parallel.randomPointsFast(4, 1)
    with pytest.raises(ValueError, match="firstBad = %d" % U.summary(want)[2]):
        curve.Parallel.pointsFromBytes(data, n, inf, check="subgroup")
    one = C.create_string_buffer(2 * params["fe_bytes"])
    assert _lib().msmz_download_points(curve._ctx, probe.handle + 1, 0, 1, one, None) == MSMZ_ERR_ARG
    curve_only = [v & 1 for v in want]
    with pytest.raises(ValueError, match="firstBad = %d" % U.summary(curve_only)[2]):
        curve.Parallel.pointsFromBytes(data, n, inf, check="curve")
    assert _lib().msmz_download_points(curve._ctx, probe.handle + 2, 0, 1, one, None) == MSMZ_ERR_ARG
    with pytest.raises(ValueError):
        curve.Parallel.pointsFromBytes(data, n, inf, check="both")
    good = curve.Parallel.randomPointsFast(500, 9)
    gdata = b"".join(p["x"].to_bytes(params["fe_bytes"], "little") + p["y"].to_bytes(params["fe_bytes"], "little")
                     for p in curve.Affine.toBigints(good))
    ok = curve.Parallel.pointsFromBytes(gdata, 500, check="subgroup")
    assert ok.handle == probe.handle + 4 and len(ok) == 500   # (good = +3)
    assert curve.Parallel.checkPoints(ok).ok
    assert curve.Affine.toBigints(ok) == curve.Affine.toBigints(good)
    for a in (probe, good, ok):
        a.free()

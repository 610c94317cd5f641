"""Eight engines in one context (csrc/multi.h), the most MSMZ_MAX_DEVICES allows, all on GPU 0 beside a single-engine
context: the scheduler, the block split and the host folds with every worker busy.  n_set = 8 x 65536 + 777 is the
smallest size at which all eight engines hold a block and engine 0 a second, ragged one.  The split arithmetic itself is
tested without a GPU over mock engines (tests/native/multi_engine_test.cpp, tests/test_multi_engine_cpu.py); this is
the same code over real engines, once.  One run per curve, no loop over engine counts."""
import ctypes as C
import random
import time

import pytest

import check_points_util as U
from oracle import c_oracle
from oracle import params as P
from oracle import prng

pytestmark = pytest.mark.gpu

G, BLK = 8, 1 << 16
N_SET = G * BLK + 777
PSEED, SSEED = 81, 82


def _lib():
    from msm_zprize_amd._native import lib
    return lib()


def _create(mod, label):
    params = mod.curves.BY_LABEL[label]
    return (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)


def _closed_form(label, pseed, sseed, n):
    """sum_i s_i [a_i] G = [sum_i s_i a_i mod q] G over the seeded sets (as tests/test_limits_gpu.py)"""
    c = P.CURVES[label]
    t = prng.sum_of_products_mod(prng.scalars_np(sseed, n, c["order"]), prng.multipliers_np(pseed, n), c["order"])
    return c_oracle.scale(c, t, {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False})


def _same_point(label, a, b):
    """twisted Edwards results carry no infinity flag: the identity is (0, 1)"""
    keys = ("x", "y", "isZero") if P.CURVES[label]["kind"] == "weierstrass" else ("x", "y")
    return all(a.get(k, False) == b.get(k, False) for k in keys)


def _check(curve, arr, first, count, what):
    """msmz_check_points -> (status, (off_curve, off_subgroup, first_bad), verdict bytes)"""
    from msm_zprize_amd._native import MsmzCheckResult
    res = MsmzCheckResult()
    buf = C.create_string_buffer(count)
    st = _lib().msmz_check_points(curve._ctx, arr.handle, first, count, what, C.byref(res), buf)
    return st, (res.off_curve, res.off_subgroup, res.first_bad), buf.raw[:count]


@pytest.mark.parametrize("label", ["bls12-377", "ed-on-bls12-377"])
def test_eight_engines_on_one_gpu(label):
    import msm_zprize_amd as mod
    params = P.CURVES[label]
    weier = params["kind"] == "weierstrass"
    fb = params["fe_bytes"]
    t0 = time.perf_counter()
    single = multi = None
    try:
        mod.startThreads(devices=[0])
        single = _create(mod, label)
        mod.startThreads(devices=[0] * G)
        multi = _create(mod, label)
        mod.startThreads()
        assert _lib().msmz_ctx_n_devices(multi._ctx) == G and _lib().msmz_ctx_n_devices(single._ctx) == 1

        # generated sets are functions of the SET index: the same on both sides of every block boundary and on the tail
        p1, s1 = single.Parallel.randomPointsFast(N_SET, PSEED), single.Parallel.randomScalars(N_SET, SSEED)
        pm, sm = multi.Parallel.randomPointsFast(N_SET, PSEED), multi.Parallel.randomScalars(N_SET, SSEED)
        for first in [k * BLK - 6 for k in range(1, G + 1)] + [N_SET - 12]:
            assert multi.Affine.toBigints(pm, first, 12) == single.Affine.toBigints(p1, first, 12), first
            assert multi.Scalar.toBigints(sm, first, 12) == single.Scalar.toBigints(s1, first, 12), first

        # MSMs: the whole set; engine 7 holds one entry; engines 3..7 idle; engine 0 alone
        fn = "msmUnsafe" if weier else "msm"
        for n in (N_SET, 7 * BLK + 1, 3 * BLK, 100):
            for opts in ([{"glv": 0}, {"glv": 1}] if weier else [{}]):
                want = getattr(single.Parallel, fn)(s1, p1, n, False, dict(opts))["result"]
                got = getattr(multi.Parallel, fn)(sm, pm, n, False, dict(opts))["result"]
                assert got == want, (n, opts)
                if n == N_SET:
                    assert _same_point(label, got, _closed_form(label, PSEED, SSEED, n)), opts

        # check_points over a byte-uploaded copy with bad points in engine 5's block and in the tail
        data = C.create_string_buffer(2 * fb * N_SET)
        assert _lib().msmz_download_points(single._ctx, p1.handle, 0, N_SET, data, None) == 0
        data = bytearray(data.raw)
        bad = [q for q in U.bad_points(label, random.Random(4)) if U.verdict(params, q)]
        where = [5 * BLK + 123, 5 * BLK + BLK - 1, G * BLK, G * BLK + 700, N_SET - 1]
        for k, i in enumerate(where):
            data[2 * fb * i:2 * fb * (i + 1)] = U.encode(params, [bad[k % len(bad)]])[0]
        data = bytes(data)
        a1, am = single.Parallel.pointsFromBytes(data, N_SET), multi.Parallel.pointsFromBytes(data, N_SET)
        want = _check(single, a1, 0, N_SET, 3)
        assert want[0] == 0 and want[1][0] + want[1][1] == len(where) and want[1][2] == where[0]
        assert [i for i, v in enumerate(want[2]) if v] == where
        assert _check(multi, am, 0, N_SET, 3) == want
        first, count = 5 * BLK + 124, 3 * BLK + 600   # starts past the first bad point, ends inside the tail
        want = _check(single, a1, first, count, 3)
        assert want[0] == 0 and want[1][2] == where[1]
        assert _check(multi, am, first, count, 3) == want
    finally:
        mod.startThreads()
        for c in (multi, single):
            if c is not None:
                c.close()
    print(f"eight engines, {label}: {time.perf_counter() - t0:.2f} s")

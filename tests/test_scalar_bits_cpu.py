"""The scalar bit bound (msmz_opts.reserved[1], `scalarBits` in the hosts) where no GPU is needed: the planner
(tests/native/scalar_bits_test.cpp), the export, and the Python host's argument checks."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSMZ_ERR_ARG = 1


def test_planner_sizes_the_windows_from_the_bound():
    """K = ceil((b + 1) / c) for every field, bound and window size; no bound = the plan from before the bound; the top
    window's range, the fold bound, the precomputed copies and the GLV choice under a bound; bad bounds refused"""
    src = os.path.join(ROOT, "tests", "native", "scalar_bits_test.cpp")
    exe = os.path.join(ROOT, "tests", "native", "scalar_bits_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "failures 0" in r.stdout, r.stdout[-4000:]
    assert int(r.stdout.split("checks ")[1].split()[0]) >= 1600000, r.stdout[-400:]
    # the two shapes the GPU error tests name
    assert "bound 64 c 7: status 0 K 10 fold_shift 3 spread 0" in r.stdout
    assert "bound 64 c 17: status 0 K 4 fold_shift 0 spread 2" in r.stdout


@pytest.fixture(scope="module")
def lib():
    from msm_zprize_amd import build
    build.build(verbose=False)
    from msm_zprize_amd import _native
    return _native.lib()


def test_scalar_bits_symbol_and_null_arguments(lib):
    assert hasattr(lib, "msmz_precomputed_scalar_bits")
    b = ctypes.c_int32()
    assert lib.msmz_precomputed_scalar_bits(None, 1, ctypes.byref(b)) == MSMZ_ERR_ARG
    assert lib.msmz_precomputed_scalar_bits(None, 1, None) == MSMZ_ERR_ARG


def test_opts_layout_is_unchanged():
    """the bound rides in reserved[1]: the struct is the 8 int32 it was"""
    from msm_zprize_amd._native import MsmzOpts
    assert ctypes.sizeof(MsmzOpts) == 32
    o = MsmzOpts()
    o.reserved[1] = 64
    assert list(o.reserved) == [0, 64, 0]


class _FakeCurve:
    pass


def _points(n, kind="points"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(_FakeCurve(), 1, n, kind)


def test_scalar_bits_python_validation():
    from msm_zprize_amd.parallel import precompute_args, scalar_bits_arg
    assert scalar_bits_arg({}, "msm") == 0
    assert scalar_bits_arg({"scalarBits": None}, "msm") == 0
    for ok in (0, 1, 64, 253, 256):
        assert scalar_bits_arg({"scalarBits": ok}, "msm") == ok
    for bad in (-1, 257, 2 ** 31, 64.0, "64", True):
        with pytest.raises(ValueError, match="scalarBits"):
            scalar_bits_arg({"scalarBits": bad}, "msm")
        with pytest.raises(ValueError, match="scalarBits"):
            precompute_args(_points(100), 10, {"scalarBits": bad}, 0)
    assert precompute_args(_points(100), 10, {"scalarBits": 64, "c": 9}, 2) == (9, -1, 2)


def test_msm_entry_points_check_scalar_bits_before_the_device():
    """msm, msmUnsafe, msmProjective, msmBatch, msmBatchUnsafe and precomputePoints refuse a bad bound without a context"""
    from msm_zprize_amd.parallel import _Parallel

    class Curve:
        fe_bytes, default_glv, kind, _ctx = 48, -1, "weierstrass", None

    par = _Parallel(Curve())
    pts = _points(8)
    s = b"\1" + b"\0" * 31
    for bad in (-1, 257, 1.5):
        o = {"scalarBits": bad}
        for call in (lambda: par.msm(s * 8, pts, 8, False, o), lambda: par.msmUnsafe(s * 8, pts, 8, False, o),
                     lambda: par.msmProjective(s * 8, pts, 8, o), lambda: par.msmBatch([s * 8], pts, 8, o),
                     lambda: par.msmBatchUnsafe([s * 8], pts, 8, o), lambda: par.precomputePoints(pts, 8, o)):
            with pytest.raises(ValueError, match="scalarBits"):
                call()

"""Precomputed point sets (msmz_precompute_points / msmz_precomputed_info) checks that need no GPU: the exports, argument
errors that need no live context, and the Python API's validation of its arguments."""
import ctypes

import pytest

MSMZ_ERR_ARG = 1


@pytest.fixture(scope="module")
def lib():
    from msm_zprize_amd import build
    build.build(verbose=False)
    from msm_zprize_amd import _native
    return _native.lib()


def test_precompute_symbols_exported(lib):
    for name in ("msmz_precompute_points", "msmz_precomputed_info"):
        assert hasattr(lib, name), name


def test_precompute_null_arguments(lib):
    from msm_zprize_amd._native import MsmzOpts
    o = MsmzOpts()
    h = ctypes.c_uint64()
    assert lib.msmz_precompute_points(None, 1, 16, ctypes.byref(o), 0, ctypes.byref(h)) == MSMZ_ERR_ARG
    assert lib.msmz_precompute_points(None, 1, 16, None, 0, None) == MSMZ_ERR_ARG
    c = ctypes.c_int32()
    assert lib.msmz_precomputed_info(None, 1, ctypes.byref(c), None, None, None, None) == MSMZ_ERR_ARG
    assert lib.msmz_precomputed_info(None, 1, None, None, None, None, None) == MSMZ_ERR_ARG


class _FakeCurve:
    pass


def _points(n, kind="points"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(_FakeCurve(), 1, n, kind)


def test_precompute_python_validation():
    from msm_zprize_amd.parallel import precompute_args
    pts = _points(100)
    assert precompute_args(pts, 100, {}, 0) == (0, -1, 0)
    assert precompute_args(pts, 1, {"c": 9, "glv": 1}, 3) == (9, 1, 3)
    with pytest.raises(TypeError):
        precompute_args(_points(100, "scalars"), 10, {}, 0)
    with pytest.raises(TypeError):
        precompute_args(b"\0" * 96, 1, {}, 0)
    for n in (0, 101, -1, 2.5, True):
        with pytest.raises(ValueError):
            precompute_args(pts, n, {}, 0)
    for f in (1, -1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError):
            precompute_args(pts, 10, {}, f)
    with pytest.raises(ValueError):
        precompute_args(pts, 10, {"c": 25}, 0)
    with pytest.raises(ValueError):
        precompute_args(pts, 10, {"glv": 2}, 0)


def test_msm_argument_checks_take_precomputed_arrays():
    """msm / msmBatch check N against a precomputed array's N (the N it was built for) before anything reaches the
    library, and a precomputed array is refused where points are precomputed"""
    from msm_zprize_amd.parallel import _Parallel, precompute_args

    class Curve:
        fe_bytes, default_glv, kind, _ctx = 48, -1, "weierstrass", None

    par = _Parallel(Curve())
    pre = _points(64, "precomputed")
    s = b"\1" + b"\0" * 31
    with pytest.raises(ValueError, match="point set holds 64"):
        par.msm(s * 65, pre, 65)
    with pytest.raises(ValueError, match="point set holds 64"):
        par.msmUnsafe(s * 65, pre, 0)
    with pytest.raises(ValueError, match="point set holds 64"):
        par.msmBatch([s * 65], pre, 65)
    with pytest.raises(TypeError):
        precompute_args(pre, 10, {}, 0)

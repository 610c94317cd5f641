"""Batched MSM (msmz_msm_batch / msmz_msm_batch_resident) checks that need no GPU: the exports, argument errors that
need no live context, the host sub-batch split, and the Python API's validation of the scalar argument."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "batch_split_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "batch_split_test")
MSMZ_ERR_ARG = 1


@pytest.fixture(scope="module")
def lib():
    from msm_zprize_amd import build
    build.build(verbose=False)
    from msm_zprize_amd import _native
    return _native.lib()


def test_batch_symbols_exported(lib):
    for name in ("msmz_msm_batch", "msmz_msm_batch_resident"):
        assert hasattr(lib, name), name


def test_batch_null_arguments(lib):
    from msm_zprize_amd._native import MsmzOpts
    o = MsmzOpts()
    out = ctypes.create_string_buffer(96)
    inf = (ctypes.c_int * 1)()
    s = b"\0" * 32
    assert lib.msmz_msm_batch(None, 1, s, 1, 1, ctypes.byref(o), out, inf, None) == MSMZ_ERR_ARG
    assert lib.msmz_msm_batch(None, 1, None, 1, 1, ctypes.byref(o), out, inf, None) == MSMZ_ERR_ARG
    assert lib.msmz_msm_batch_resident(None, 1, 2, 1, 1, ctypes.byref(o), out, inf, None) == MSMZ_ERR_ARG


@pytest.fixture(scope="module")
def split():
    deps = [SRC, os.path.join(ROOT, "msm_zprize_amd", "csrc", "multi.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", EXE, SRC])

    def run(cases):
        inp = "".join(f"{r} {e} {c}\n" for r, e, c in cases)
        out = subprocess.run([EXE], input=inp, capture_output=True, text=True, check=True).stdout.split()
        return [int(v) for v in out]

    return run


def test_sub_batch_split(split):
    cap = 1 << 26
    per = 20 * (1 << 16)   # BLS12-377, 2^16 points, no GLV: ~20 windows
    cases = [(64, per, cap), (1, per, cap), (7, per, cap), (64, 1, cap), (5, cap * 2, cap), (100, 3, 10), (0, 5, 10)]
    got = split(cases)
    assert got == [32, 1, 7, 64, 1, 3, 0]
    # dealt evenly, never above the cap, and the sub-batches cover all problems
    for rem, e, c in [(64, per, cap), (100, 3, 10), (1000, 70001, cap), (33, 1 << 24, 1 << 26)]:
        left, sizes = rem, []
        while left:
            b = split([(left, e, c)])[0]
            assert b >= 1 and (b == 1 or b * e <= c)
            sizes.append(b)
            left -= b
        assert sum(sizes) == rem and max(sizes) - min(sizes) <= 1


class _FakeCurve:
    fe_bytes = 48
    default_glv = 1
    kind = "weierstrass"
    _ctx = None


def test_python_batch_scalar_argument():
    from msm_zprize_amd import parallel
    cv = _FakeCurve()
    N = 4
    # one resident array of B x N scalars
    res = parallel.DeviceArray(cv, 1, 12, "scalars")
    assert parallel.batch_scalars(res, N)[::2] == ("resident", 3)
    assert parallel.batch_scalars(res, N, 2)[::2] == ("resident", 2)
    with pytest.raises(ValueError):          # too short for the requested batch
        parallel.batch_scalars(res, N, 4)
    with pytest.raises(ValueError):          # shorter than one vector
        parallel.batch_scalars(parallel.DeviceArray(cv, 1, 3, "scalars"), N)
    with pytest.raises(ValueError):
        parallel.batch_scalars(parallel.DeviceArray(cv, 1, 12, "points"), N)
    # a list of B host arrays: concatenated
    vecs = [bytes([k]) * 32 * N for k in range(3)]
    kind, data, B = parallel.batch_scalars(vecs, N)
    assert (kind, B) == ("host", 3) and data == b"".join(vecs)
    kind, data, B = parallel.batch_scalars([v + b"\0" * 32 for v in vecs], N)   # longer vectors: first N scalars
    assert data == b"".join(vecs)
    with pytest.raises(ValueError):          # unequal lengths
        parallel.batch_scalars([vecs[0], vecs[1] + b"\0" * 32], N)
    with pytest.raises(ValueError):          # shorter than N scalars
        parallel.batch_scalars([v[:-1] for v in vecs], N)
    with pytest.raises(ValueError):
        parallel.batch_scalars([], N)
    with pytest.raises(TypeError):           # a list of resident arrays is refused
        parallel.batch_scalars([res, res], N)
    with pytest.raises(TypeError):           # one flat byte string is not a list of vectors
        parallel.batch_scalars(vecs[0], N)


def test_python_msm_batch_validates_before_the_library():
    from msm_zprize_amd import parallel
    cv = _FakeCurve()
    par = parallel._Parallel(cv)
    pts = parallel.DeviceArray(cv, 1, 4, "points")
    with pytest.raises(ValueError):
        par.msmBatch([b"\0" * 32 * 5], pts, 5)    # N beyond the point set
    with pytest.raises(ValueError):
        par.msmBatchUnsafe([b"\0" * 32 * 4, b"\0" * 32 * 3], pts, 4)
    with pytest.raises(TypeError):
        par.msmBatch([parallel.DeviceArray(cv, 2, 4, "scalars")] * 2, pts, 4)

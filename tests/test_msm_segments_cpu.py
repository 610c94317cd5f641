"""Host-only parts of the segmented MSM (msmz_msm_segments): the exported symbol, the null-context errors, the length
classes the engine deals segments into (segment_classes, csrc/multi.h, through a native driver) and the Python argument
validation.  No GPU."""
import ctypes
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "segment_classes_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "segment_classes_test")
MSMZ_ERR_ARG = 1


@pytest.fixture(scope="module")
def lib():
    from msm_zprize_amd import build
    build.build(verbose=False)
    from msm_zprize_amd import _native
    return _native.lib()


def test_segments_symbol_exported(lib):
    assert hasattr(lib, "msmz_msm_segments")


def test_segments_null_arguments(lib):
    from msm_zprize_amd._native import MsmzOpts, MsmzSegment
    o = MsmzOpts()
    out = ctypes.create_string_buffer(96)
    inf = (ctypes.c_int * 1)()
    segs = (MsmzSegment * 1)(MsmzSegment(0, 0, 1))
    assert lib.msmz_msm_segments(None, 1, 2, segs, 1, ctypes.byref(o), out, inf, None) == MSMZ_ERR_ARG
    assert lib.msmz_msm_segments(None, 1, 2, None, 1, ctypes.byref(o), out, inf, None) == MSMZ_ERR_ARG
    assert lib.msmz_msm_segments(None, 1, 2, segs, 0, None, None, None, None) == MSMZ_ERR_ARG


@pytest.fixture(scope="module")
def classes():
    deps = [SRC, os.path.join(ROOT, "msm_zprize_amd", "csrc", "multi.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", EXE, SRC])

    def run(lengths):
        inp = " ".join(str(n) for n in lengths) + "\n"
        lines = subprocess.run([EXE], input=inp, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(lines) == 2 and lines[0].startswith("order") and lines[1].startswith("starts")
        return [int(v) for v in lines[0].split()[1:]], [int(v) for v in lines[1].split()[1:]]

    return run


def _check(lengths, order, starts):
    """the contract of segment_classes, restated: a bijection; classes by floor(log2 n), each a contiguous slice, shortest
    first, caller order inside"""
    assert sorted(order) == list(range(len(lengths)))
    assert starts[0] == 0 and starts[-1] == len(lengths) and starts == sorted(set(starts))
    bits = [n.bit_length() - 1 for n in lengths]
    seen = []
    for lo, hi in zip(starts, starts[1:]):
        members = order[lo:hi]
        cls = {bits[k] for k in members}
        assert len(cls) == 1
        assert members == sorted(members)            # caller order kept
        seen.append(cls.pop())
    assert seen == sorted(set(bits))                 # one class per bit length, every bit length, ascending
    for lo, hi in zip(starts, starts[1:]):           # the 2x bound the grouping exists for
        ns = [lengths[k] for k in order[lo:hi]]
        assert max(ns) < 2 * min(ns)


def test_segment_classes(classes):
    assert classes([7]) == ([0], [0, 1])                                       # a single segment
    assert classes([300] * 5) == ([0, 1, 2, 3, 4], [0, 5])                     # all equal
    assert classes([1, 1 << 24]) == ([0, 1], [0, 1, 2])                        # the extremes
    assert classes([1 << 24, 1]) == ([1, 0], [0, 1, 2])
    assert classes([2048, 2049, 3000, 4095]) == ([0, 1, 2, 3], [0, 4])         # one class
    assert classes([4095, 4096]) == ([0, 1], [0, 1, 2])                        # a power of two opens the next class
    order, starts = classes([1, 5, 257, 300, 4095, 5, 1, 300])
    assert order == [0, 6, 1, 5, 2, 3, 7, 4] and starts == [0, 2, 4, 7, 8]
    rng = random.Random(17)
    for _ in range(20):
        lengths = [rng.randrange(1, 1 << rng.randrange(1, 26)) for _ in range(rng.randrange(1, 60))]
        _check(lengths, *classes(lengths))
    big = [(1 << 40) + 5, 3, (1 << 63) + 1, 2]                                # 64-bit lengths do not wrap
    _check(big, *classes(big))


class _FakeCurve:
    fe_bytes = 48
    default_glv = 1
    kind = "weierstrass"
    _ctx = None


def test_python_segments_argument():
    from msm_zprize_amd import parallel
    cv = _FakeCurve()
    pts = parallel.DeviceArray(cv, 1, 100, "points")
    pre = parallel.DeviceArray(cv, 3, 100, "precomputed")
    sc = parallel.DeviceArray(cv, 2, 50, "scalars")
    args = parallel.msm_segments_args
    assert args(sc, pts, [(50, 0, 50), (0, 25, 25)]) == [(50, 0, 50), (0, 25, 25)]
    assert args(sc, pre, ((99, 49, 1),)) == [(99, 49, 1)]
    assert args(sc, pts, [[0, 0, 1], [0, 0, 1]]) == [(0, 0, 1), (0, 0, 1)]     # repeats and overlaps are fine
    for bad in ([], [(0, 0, 0)], [(0, 0, -1)], [(-1, 0, 1)], [(0, -1, 1)], [(51, 0, 50)], [(0, 1, 50)], [(100, 0, 1)],
                [(0, 50, 1)], [(0, 0, 1.0)], [(0, 0, True)], [(0, 0, 1), (0, 0, 51)]):
        with pytest.raises(ValueError):
            args(sc, pts, bad)
    for bad in ([(0, 0)], [(0, 0, 1, 1)], [5], ["abc"], 7, "abc", None):
        with pytest.raises(TypeError):
            args(sc, pts, bad)
    with pytest.raises(TypeError):
        args(pts, pts, [(0, 0, 1)])          # points where the scalars belong
    with pytest.raises(TypeError):
        args(sc, sc, [(0, 0, 1)])
    with pytest.raises(TypeError):
        args(b"\0" * 32, pts, [(0, 0, 1)])   # host scalars: upload them first


def test_python_msm_segments_validates_before_the_library():
    from msm_zprize_amd import parallel
    cv = _FakeCurve()
    par = parallel._Parallel(cv)
    pts = parallel.DeviceArray(cv, 1, 4, "points")
    sc = parallel.DeviceArray(cv, 2, 4, "scalars")
    with pytest.raises(ValueError):
        par.msmSegments(sc, pts, [(0, 0, 5)])
    with pytest.raises(ValueError):
        par.msmSegmentsUnsafe(sc, pts, [])
    with pytest.raises(ValueError):
        par.msmSegments(sc, pts, [(0, 0, 4)], {"scalarBits": 300})
    with pytest.raises(TypeError):
        par.msmSegments([b"\0" * 128], pts, [(0, 0, 4)])

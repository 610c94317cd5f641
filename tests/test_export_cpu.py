"""Exports (msmz_export_scalars / msmz_export_points; scalarsToTensor, pointsToTensor, scalarsToBytes, pointsToBytes in
the Python host) where no GPU is needed: fr_to_mont and the generated constant RSTD against Python integers
(tests/native/export_test.cpp), the layout of msmz_dst on the C and the ctypes side, the entry points without a context,
the argument functions on fake tensors, the untouched download route of toBigints, and the import without torch."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSMZ_ERR_ARG = 1
LABELS = ["bls12-377", "pallas", "bls12-381", "ed-on-bls12-377"]
R256 = 1 << 256


def _curves():
    from msm_zprize_amd import curves
    return [curves.BY_LABEL[l] for l in LABELS]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "export_test.cpp")
    exe = os.path.join(ROOT, "tests", "native", "export_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src])

    def run(cases):
        path = tmp_path_factory.mktemp("export") / "in.txt"
        path.write_text("".join("%d %064x\n" % c for c in cases))
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout.splitlines()

    return run


def test_fr_to_mont_matches_python(driver):
    """v * 2^256 mod q for the four scalar fields, on 0, 1, q - 1, 2^256 mod q and a few thousand seeded values, and
    fr_from_mont(fr_to_mont(v)) == v"""
    cases = []
    for f, c in enumerate(_curves()):
        q = c["order"]
        rng = random.Random(200 + f)
        for v in [0, 1, 2, q - 1, q - 2, R256 % q, (q - 1) // 2] + [rng.randrange(q) for _ in range(3000)]:
            cases.append((f, v))
    out = [l for l in driver(cases) if l[0].isdigit()]
    assert len(out) == len(cases)
    for line, (f, v) in zip(out, cases):
        q = _curves()[f]["order"]
        assert line == "%d %064x %064x" % (f, v * R256 % q, v)


def test_rstd_by_its_definition(driver):
    """RSTD < p and == 2^(8 fe_bytes) mod p; and what the kernel does with it: the Montgomery product of a resident
    v R_int with RSTD, (v R_int) RSTD / R_int, is v 2^(8 fe_bytes) mod p -- for N and W as printed"""
    lines = [l.split() for l in driver([]) if l.startswith("const")]
    seen = set()
    for _, f, name, n, w, *limbs in lines:
        c = _curves()[int(f)]
        p = c["modulus"]
        N, W = int(n), int(w)
        limbs = [int(x) for x in limbs]
        assert name == "RSTD" and len(limbs) == N
        val = sum(l << (W * j) for j, l in enumerate(limbs))
        r_int, r_std = 1 << (N * W), 1 << (8 * c["fe_bytes"])
        assert 0 <= val < p and val == r_std % p
        rng = random.Random(300 + int(f))
        for v in [0, 1, p - 1, 0x1234567 % p] + [rng.randrange(p) for _ in range(50)]:
            assert (v * r_int % p) * val * pow(r_int, -1, p) % p == v * r_std % p
        seen.add(int(f))
    assert seen == {0, 1, 2, 3}


def test_struct_layouts(driver):
    """sizeof(msmz_dst) == 40 and every offset equal to msmz_src's, on the C side and the ctypes side"""
    from msm_zprize_amd._native import MsmzDst, MsmzSrc
    got = {l.split()[1]: [int(x) for x in l.split()[2:]] for l in driver([]) if l.startswith("layout")}
    assert set(got) == {"msmz_src", "msmz_dst"}
    assert got["msmz_dst"] == got["msmz_src"] == [40, 0, 8, 16, 20, 24, 32]
    for f in (MsmzSrc, MsmzDst):
        assert [ctypes.sizeof(f), f.ptr.offset, f.stride.offset, f.width.offset, f.flags.offset, f.stream.offset,
                f.is_inf.offset] == got["msmz_dst"]
    assert [n for n, _ in MsmzDst._fields_] == [n for n, _ in MsmzSrc._fields_]


@pytest.fixture(scope="module")
def lib():
    from msm_zprize_amd import build
    build.build(verbose=False)
    from msm_zprize_amd import _native
    return _native.lib()


def test_symbols_and_null_arguments(lib):
    from msm_zprize_amd._native import EXPORTS, MsmzDst
    buf = ctypes.create_string_buffer(b"\xa5" * 64, 64)
    ok = MsmzDst(ctypes.cast(buf, ctypes.c_void_p), 0, 32, 0, None, None)
    for name in ("msmz_export_scalars", "msmz_export_points"):
        assert name in EXPORTS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn(None, 1, 0, 1, ctypes.byref(ok)) == MSMZ_ERR_ARG      # a null ctx
        assert fn(None, 1, 0, 1, None) == MSMZ_ERR_ARG
        # a null dst with something that is not null as ctx: refused before the context is looked at
        assert fn(ctypes.cast(buf, ctypes.c_void_p), 1, 0, 1, None) == MSMZ_ERR_ARG
    assert buf.raw == b"\xa5" * 64


# ---------------------------------------------------------------------------------------------- the Python host
class _Dev:
    def __init__(self, type_, index=None):
        self.type, self.index = type_, index

    def __eq__(self, o):
        return (self.type, self.index) == (o.type, o.index)

    def __repr__(self):
        return self.type if self.index is None else f"{self.type}:{self.index}"


class FakeTensor:
    """the attributes tensor_view reads; a CPU device so torch is never asked for a stream"""

    def __init__(self, shape, strides=None, item=8, device=None, ptr=0x1000):
        self.shape = tuple(shape)
        if strides is None:
            strides, acc = [], 1
            for s in reversed(self.shape):
                strides.insert(0, acc)
                acc *= s
        self._strides, self._item, self.device, self._ptr = tuple(strides), item, device or _Dev("cpu"), ptr

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        return self._strides[i]

    def element_size(self):
        return self._item

    def data_ptr(self):
        return self._ptr


def _arr(n, kind="scalars"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(object(), 7, n, kind)


def test_export_tensor_view_accepts():
    from msm_zprize_amd.parallel import export_tensor_view
    ev = lambda arr, out, first=0, N=None, m=False, kind="scalars", fb=48, **k: export_tensor_view(
        arr, kind, out, first, N, [0], fb, m, "scalarsToTensor", **k)
    v = ev(_arr(100), FakeTensor((100, 4)))
    assert (v["n"], v["width"], v["stride"], v["device"], v["ptr"]) == (100, 32, 32, False, 0x1000)
    assert ev(_arr(100), FakeTensor((40, 4)), 60)["n"] == 40                    # N=None: the rows of `out`
    assert ev(_arr(100), FakeTensor((40, 4)), 7, 33)["n"] == 33                 # fewer entries than rows
    v = ev(_arr(100), FakeTensor((100,)))                                       # 1-D of an 8-byte dtype
    assert (v["width"], v["stride"]) == (8, 8)
    v = ev(_arr(100), FakeTensor((100, 1), strides=(6, 1)))                     # a column of a (100, 6) matrix
    assert (v["width"], v["stride"]) == (8, 48)
    assert ev(_arr(9), FakeTensor((9, 8), item=4), m=True)["montgomery"] is True
    assert ev(_arr(9), FakeTensor((9, 4), item=1))["width"] == 4
    v = ev(_arr(5, "points"), FakeTensor((5, 96), item=1), kind="points", is_inf=FakeTensor((5,), item=1, ptr=0x2000))
    assert (v["width"], v["is_inf"]) == (96, 0x2000)
    assert ev(_arr(5, "points"), FakeTensor((5, 48), item=1), kind="points", compressed=True)["width"] == 48
    assert ev(_arr(5, "points"), FakeTensor((5, 8)), m=True, kind="points", fb=32)["width"] == 64


def test_export_tensor_view_refuses():
    from msm_zprize_amd.parallel import export_tensor_view
    ev = lambda arr, out, first=0, N=None, m=False, kind="scalars", fb=48, **k: export_tensor_view(
        arr, kind, out, first, N, [0], fb, m, "who", **k)
    with pytest.raises(TypeError, match="expected a torch.Tensor"):
        ev(_arr(10), bytearray(320))
    with pytest.raises(TypeError, match="resident scalar array"):
        ev(_arr(10, "points"), FakeTensor((10, 4)))
    with pytest.raises(TypeError, match="resident point array"):
        ev(_arr(10), FakeTensor((10, 96), item=1), kind="points")
    for bad in (FakeTensor((10, 4), strides=(8, 2)), FakeTensor((10, 9), item=4), FakeTensor((10, 3), item=1),
                FakeTensor((10,), item=4), FakeTensor((10, 2, 2)), FakeTensor((0, 4)), FakeTensor((10, 4), strides=(2, 1)),
                FakeTensor((10, 6), item=2, strides=(7, 1)), FakeTensor((10, 4), ptr=0x1002),
                FakeTensor((10, 4), device=_Dev("meta"))):
        with pytest.raises(ValueError):
            ev(_arr(10), bad)
    with pytest.raises(ValueError, match="Montgomery"):
        ev(_arr(10), FakeTensor((10, 1)), m=True)
    with pytest.raises(ValueError, match="context drives"):
        ev(_arr(10), FakeTensor((10, 4), device=_Dev("cuda", 1)))
    with pytest.raises(ValueError, match="a point is 96"):
        ev(_arr(10, "points"), FakeTensor((10, 8)), kind="points")
    with pytest.raises(ValueError, match="a point is 48"):
        ev(_arr(10, "points"), FakeTensor((10, 96), item=1), kind="points", compressed=True)
    with pytest.raises(ValueError, match="is_inf"):
        ev(_arr(5, "points"), FakeTensor((5, 96), item=1), kind="points", is_inf=FakeTensor((4,), item=1))
    # a tensor that is too small for the entries asked for
    with pytest.raises(ValueError, match="12 entries into a tensor of 10 rows"):
        ev(_arr(100), FakeTensor((10, 4)), 0, 12)
    # first / N faults, in the wording every operation over resident arrays shares
    with pytest.raises(ValueError, match=r"who: first = -1"):
        ev(_arr(10), FakeTensor((10, 4)), -1)
    with pytest.raises(ValueError, match=r"who: first = True"):
        ev(_arr(10), FakeTensor((10, 4)), True)
    with pytest.raises(ValueError, match=r"who: first = 10 but the array holds 10"):
        ev(_arr(10), FakeTensor((10, 4)), 10)
    with pytest.raises(ValueError, match=r"who: N = 0"):
        ev(_arr(10), FakeTensor((10, 4)), 0, 0)
    with pytest.raises(ValueError, match=r"who: N = 2\.0"):
        ev(_arr(10), FakeTensor((10, 4)), 0, 2.0)
    with pytest.raises(ValueError, match=r"who: entries \[4, \+10\) from first of an array of 10"):
        ev(_arr(10), FakeTensor((10, 4)), 4)               # N=None takes the tensor's 10 rows: beyond the array
    with pytest.raises(ValueError, match=r"who: entries \[4, \+7\) from first of an array of 10"):
        ev(_arr(10), FakeTensor((10, 4)), 4, 7)


def test_export_range_args():
    from msm_zprize_amd.parallel import export_range_args
    assert export_range_args(_arr(10), "scalars", 0, None, "x") == (0, 10)
    assert export_range_args(_arr(10), "scalars", 7, None, "x") == (7, 3)
    assert export_range_args(_arr(10, "points"), "points", 2, 8, "x") == (2, 8)
    for first, N in ((0, 11), (10, 1), (3, 8), (-1, 1), (0, 0), (0, -1), ("0", 1), (0, "1")):
        with pytest.raises(ValueError, match="x: "):
            export_range_args(_arr(10), "scalars", first, N, "x")
    with pytest.raises(TypeError):
        export_range_args(object(), "scalars", 0, 1, "x")


class _Recorder:
    """stands in for the loaded library: records which entry point a call reaches"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


class _Curve:
    fe_bytes, default_glv, kind, _ctx, devices = 48, -1, "weierstrass", "ctx", [0]
    params = {"order": 97, "modulus": 101, "kind": "weierstrass", "fe_bytes": 48}

    def _point(self, raw, k, is_zero, zero_rule=True):
        return {"x": 0, "y": 0, "isZero": is_zero}


def test_downloads_keep_their_route_and_exports_take_theirs(monkeypatch):
    """Scalar.toBigints and Affine.toBigints still reach msmz_download_*; the byte and tensor exports reach
    msmz_export_* with the descriptor the arguments describe"""
    from msm_zprize_amd import parallel
    from msm_zprize_amd._native import MSMZ_SRC_COMPRESSED, MSMZ_SRC_MONTGOMERY, MSMZ_SRC_SIGN_PARITY
    rec = _Recorder()
    monkeypatch.setattr(parallel, "lib", lambda: rec)
    curve = _Curve()
    sc = parallel.DeviceArray(curve, 5, 10, "scalars")
    pts = parallel.DeviceArray(curve, 6, 10, "points")
    assert parallel._Scalar(curve).toBigints(sc, 2, 3) == [0, 0, 0]
    assert rec.calls[-1][0] == "msmz_download_scalars" and rec.calls[-1][1][:4] == ("ctx", 5, 2, 3)
    assert len(parallel._Affine(curve).toBigints(pts, 1, 4)) == 4
    assert rec.calls[-1][0] == "msmz_download_points" and rec.calls[-1][1][:4] == ("ctx", 6, 1, 4)
    parallel._Affine(curve).toCompressedBytes(pts)
    assert rec.calls[-1][0] == "msmz_download_points_compressed"
    assert all(not name.startswith("msmz_export") for name, _ in rec.calls)

    par = parallel._Parallel(curve)
    assert par.scalarsToBytes(sc, 2, 3, width=8) == bytes(24)
    name, args = rec.calls[-1]
    d = args[4]._obj
    assert name == "msmz_export_scalars" and args[:4] == ("ctx", 5, 2, 3)
    assert (d.width, d.stride, d.flags, d.stream, d.is_inf) == (8, 0, 0, None, None) and d.ptr
    par.scalarsToBytes(sc, montgomery=True)
    d = rec.calls[-1][1][4]._obj
    assert rec.calls[-1][1][1:4] == (5, 0, 10) and (d.width, d.flags) == (32, MSMZ_SRC_MONTGOMERY)
    data, flags = par.pointsToBytes(pts, 4, montgomery=True)
    d = rec.calls[-1][1][4]._obj
    assert rec.calls[-1][0] == "msmz_export_points" and rec.calls[-1][1][1:4] == (6, 4, 6)
    assert (len(data), len(flags), d.width, d.flags) == (96 * 6, 6, 96, MSMZ_SRC_MONTGOMERY) and d.is_inf
    out = FakeTensor((4, 1), strides=(6, 1))
    assert par.scalarsToTensor(sc, out, first=3) is out
    d = rec.calls[-1][1][4]._obj
    assert rec.calls[-1][1][1:4] == (5, 3, 4) and (d.ptr, d.width, d.stride, d.flags) == (0x1000, 8, 48, 0)
    out, fl = FakeTensor((10, 48), item=1), FakeTensor((10,), item=1, ptr=0x3000)
    assert par.pointsToTensor(pts, out, compressed=True, sign="parity", is_inf=fl) == (out, fl)
    d = rec.calls[-1][1][4]._obj
    assert (d.width, d.flags, d.is_inf) == (48, MSMZ_SRC_COMPRESSED | MSMZ_SRC_SIGN_PARITY, 0x3000)
    # refused before the library is reached
    before = len(rec.calls)
    for call in (lambda: par.scalarsToBytes(sc, width=6), lambda: par.scalarsToBytes(sc, width=8, montgomery=True),
                 lambda: par.scalarsToBytes(sc, 4, 7), lambda: par.pointsToBytes(pts, 10),
                 lambda: par.scalarsToTensor(sc, FakeTensor((4, 4)), N=5),
                 lambda: par.pointsToTensor(pts, FakeTensor((10, 96), item=1), montgomery=True, compressed=True),
                 lambda: par.pointsToTensor(pts, FakeTensor((10, 96), item=1), sign="parity")):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: par.scalarsToBytes(pts), lambda: par.pointsToBytes(sc), lambda: par.scalarsToTensor(pts, out),
                 lambda: par.pointsToBytes(pts, montgomery=1)):
        with pytest.raises(TypeError):
            call()
    assert len(rec.calls) == before


def test_package_imports_without_torch():
    code = ("import sys; import msm_zprize_amd, msm_zprize_amd.parallel as p; "
            "assert hasattr(p._Parallel, 'scalarsToTensor') and hasattr(p._Parallel, 'pointsToTensor'); "
            "assert 'torch' not in sys.modules")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)

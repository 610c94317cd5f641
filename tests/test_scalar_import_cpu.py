"""Imports (msmz_import_scalars / _into / msmz_import_points; scalarsFromTensor and friends in the Python host) where no
GPU is needed: fr_from_mont and the generated constants against Python integers (tests/native/scalar_import_test.cpp),
the exports and their argument checks without a context, the struct layouts, the tensor argument function on fake
tensors, and the unchanged defaults of scalarsFromBytes / pointsFromBytes."""
import ctypes
import os
import random
import re
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
    src = os.path.join(ROOT, "tests", "native", "scalar_import_test.cpp")
    exe = os.path.join(ROOT, "tests", "native", "scalar_import_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src])

    def run(cases):
        path = tmp_path_factory.mktemp("scalar_import") / "in.txt"
        path.write_text("".join("%d %064x\n" % c for c in cases))
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout.splitlines()

    return run


def test_fr_from_mont_matches_python(driver):
    """a * 2^-256 mod q for the four scalar fields: v * 2^256 mod q -> v on the edges and a few thousand seeded values,
    and any a < 2^256 (not only residues) gives the canonical value"""
    cases, want = [], []
    for f, c in enumerate(_curves()):
        q = c["order"]
        rinv = pow(R256, -1, q)
        rng = random.Random(100 + f)
        vs = [0, 1, 2, q - 1, q - 2, R256 % q, (q - 1) // 2] + [rng.randrange(q) for _ in range(3000)]
        for v in vs:
            cases.append((f, v * R256 % q))
            want.append((f, v))
        # residues just below q, and raw words up to 2^256 - 1 (the kernel converts before it knows the range verdict)
        for a in [q - 1, q - 2, q - 3, q, q + 1, R256 - 1, R256 - 2] + [rng.randrange(R256) for _ in range(500)]:
            cases.append((f, a))
            want.append((f, a * rinv % q))
    out = [l for l in driver(cases) if not l.startswith("const")]
    assert len(out) == len(want)
    for line, (f, v) in zip(out, want):
        assert line == "%d %064x" % (f, v)


def test_generated_constants_by_their_definitions(driver):
    """q * q' = -1 mod 2^32; R2STD * R_std = R_int^2 mod p with R_int = 2^(N W), R_std = 2^(8 fe_bytes); R2 = R_int^2"""
    lines = [l.split() for l in driver([]) if l.startswith("const")]
    seen = set()
    for _, f, name, *rest in lines:
        c = _curves()[int(f)]
        p, q = c["modulus"], c["order"]
        if name == "QINV32":
            assert (q * int(rest[0], 16) + 1) % (1 << 32) == 0
        else:
            N, W = int(rest[0]), int(rest[1])
            limbs = [int(x) for x in rest[2:]]
            assert len(limbs) == N
            val = sum(l << (W * j) for j, l in enumerate(limbs))
            r_int, r_std = 1 << (N * W), 1 << (8 * c["fe_bytes"])
            assert 0 <= val < p
            if name == "R2STD":
                assert val * r_std % p == r_int * r_int % p
                # what the kernel does with it: fe_mul(v * R_std, R2STD) = v * R_std * R2STD / R_int = v * R_int
                v = 0x1234567 % p
                assert (v * r_std % p) * val * pow(r_int, -1, p) % p == v * r_int % p
            else:
                assert name == "R2" and val == r_int * r_int % p
        seen.add((int(f), name))
    assert seen == {(f, n) for f in range(4) for n in ("QINV32", "R2STD", "R2")}


@pytest.fixture(scope="module")
def lib():
    from msm_zprize_amd import build
    build.build(verbose=False)
    from msm_zprize_amd import _native
    return _native.lib()


def test_symbols_and_null_arguments(lib):
    from msm_zprize_amd._native import MsmzSrc
    for name in ("msmz_import_scalars", "msmz_import_scalars_into", "msmz_import_points", "msmz_alloc_scalars"):
        assert hasattr(lib, name)
    assert lib.msmz_alloc_scalars(None, 8, ctypes.byref(ctypes.c_uint64())) == MSMZ_ERR_ARG
    buf = ctypes.create_string_buffer(64)
    ok = MsmzSrc(ctypes.cast(buf, ctypes.c_void_p), 0, 32, 0, None, None)
    h = ctypes.c_uint64()
    assert lib.msmz_import_scalars(None, ctypes.byref(ok), 1, ctypes.byref(h)) == MSMZ_ERR_ARG
    assert lib.msmz_import_scalars(None, None, 1, ctypes.byref(h)) == MSMZ_ERR_ARG
    assert lib.msmz_import_scalars_into(None, 1, 0, ctypes.byref(ok), 1) == MSMZ_ERR_ARG
    assert lib.msmz_import_scalars_into(None, 1, 0, None, 1) == MSMZ_ERR_ARG
    assert lib.msmz_import_points(None, ctypes.byref(ok), 1, ctypes.byref(h)) == MSMZ_ERR_ARG
    assert lib.msmz_import_points(None, None, 1, None) == MSMZ_ERR_ARG


def test_struct_layouts():
    from msm_zprize_amd._native import MsmzOpts, MsmzSrc
    assert ctypes.sizeof(MsmzOpts) == 32
    assert ctypes.sizeof(MsmzSrc) == 40
    # the C side: sizeof and the offsets of every field
    src = ("#include <stddef.h>\n#include <stdio.h>\n#include \"%s\"\nint main(){printf(\"%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n\","
           "sizeof(msmz_src),offsetof(msmz_src,ptr),offsetof(msmz_src,stride),offsetof(msmz_src,width),"
           "offsetof(msmz_src,flags),offsetof(msmz_src,stream),offsetof(msmz_src,is_inf),sizeof(msmz_opts));return 0;}\n"
           % os.path.join(ROOT, "include", "msmz.h"))
    exe = os.path.join(ROOT, "tests", "native", "scalar_import_test") + "_layout"
    try:
        subprocess.run(["gcc", "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
        got = [int(x) for x in subprocess.check_output([exe], text=True, stdin=subprocess.DEVNULL).split()]
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    f = MsmzSrc
    assert got == [ctypes.sizeof(f), f.ptr.offset, f.stride.offset, f.width.offset, f.flags.offset, f.stream.offset,
                   f.is_inf.offset, 32]


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


def test_tensor_view_accepts():
    from msm_zprize_amd.parallel import tensor_view
    tv = lambda t, m=False, kind="scalars", fb=48, **k: tensor_view(t, [0], kind, fb, m, "scalarsFromTensor", **k)
    v = tv(FakeTensor((100, 4)))
    assert (v["n"], v["width"], v["stride"], v["device"], v["ptr"], v["stream"]) == (100, 32, 32, False, 0x1000, 0)
    assert tv(FakeTensor((100,)))["width"] == 8                                   # 1-D of an 8-byte dtype
    v = tv(FakeTensor((100, 1), strides=(6, 1)))                                  # a column view of a (100, 6) matrix
    assert (v["width"], v["stride"]) == (8, 48)
    v = tv(FakeTensor((100,), strides=(6,)))
    assert (v["width"], v["stride"]) == (8, 48)
    assert tv(FakeTensor((7, 8), item=4), True)["montgomery"] is True             # 8 x uint32 = 32 bytes
    assert tv(FakeTensor((7, 4), item=1))["width"] == 4
    assert tv(FakeTensor((1, 4), strides=(0, 1)))["stride"] == 32                 # one row: its stride does not matter
    v = tv(FakeTensor((5, 96), item=1), kind="points", is_inf=FakeTensor((5,), item=1, ptr=0x2000))
    assert (v["width"], v["is_inf"]) == (96, 0x2000)
    assert tv(FakeTensor((5, 8)), True, kind="points", fb=32)["width"] == 64


def test_tensor_view_refuses():
    from msm_zprize_amd.parallel import tensor_view
    tv = lambda t, m=False, kind="scalars", fb=48, devs=(0,), **k: tensor_view(t, list(devs), kind, fb, m, "who", **k)
    with pytest.raises(TypeError):
        tv(b"\0" * 32)
    bad = [FakeTensor((10, 4), strides=(8, 2)),          # last dimension not contiguous
           FakeTensor((10, 9), item=4),                  # width 36
           FakeTensor((10, 3), item=1),                  # width 3
           FakeTensor((10, 5)),                          # width 40
           FakeTensor((10,), item=4),                    # 1-D of a 4-byte dtype
           FakeTensor((10, 2, 2)), FakeTensor((0, 4)),
           FakeTensor((10, 4), strides=(2, 1)),          # rows overlap
           FakeTensor((10, 6), item=2, strides=(7, 1)),  # row stride 14 bytes: not a multiple of 4
           FakeTensor((10, 4), ptr=0x1002), FakeTensor((10, 4), ptr=0),
           FakeTensor((10, 4), device=_Dev("meta"))]
    for t in bad:
        with pytest.raises(ValueError):
            tv(t)
    with pytest.raises(ValueError, match="Montgomery"):
        tv(FakeTensor((10, 1)), True)                    # Montgomery with width 8
    with pytest.raises(ValueError, match="context drives"):
        tv(FakeTensor((10, 4), device=_Dev("cuda", 1)))  # wrong device (refused before torch is asked for a stream)
    with pytest.raises(ValueError, match="context drives"):
        tv(FakeTensor((10, 4), device=_Dev("cuda", 3)), devs=(0, 1))
    with pytest.raises(ValueError, match="a point is 96"):
        tv(FakeTensor((10, 8)), kind="points")
    with pytest.raises(ValueError):
        tv(FakeTensor((10,)), kind="points")
    for flags in (FakeTensor((4,), item=1), FakeTensor((5,), item=4), FakeTensor((5, 1), item=1),
                  FakeTensor((5,), item=1, strides=(2,)), FakeTensor((5,), item=1, device=_Dev("cuda", 0))):
        with pytest.raises(ValueError, match="is_inf"):
            tv(FakeTensor((5, 96), item=1), kind="points", is_inf=flags)
    with pytest.raises(ValueError, match="belong to points"):
        tv(FakeTensor((5, 4)), is_inf=FakeTensor((5,), item=1))


def test_scalar_width_arg():
    from msm_zprize_amd.parallel import scalar_width_arg
    for w in (4, 8, 12, 16, 20, 24, 28, 32):
        assert scalar_width_arg(w, False, "x") == w
    assert scalar_width_arg(32, True, "x") == 32
    for w in (0, 2, 3, 6, 36, 64, -4, 8.0, "8", True, None):
        with pytest.raises(ValueError, match="width"):
            scalar_width_arg(w, False, "x")
    with pytest.raises(ValueError, match="Montgomery"):
        scalar_width_arg(8, True, "x")


class _Recorder:
    """stands in for the loaded library: records which entry point a call reaches"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_byte_routes_keep_their_defaults(monkeypatch):
    """scalarsFromBytes / pointsFromBytes without the new keywords call msmz_upload_*, with the same arguments as
    before; with them, msmz_import_*"""
    from msm_zprize_amd import parallel
    from msm_zprize_amd._native import MSMZ_SRC_MONTGOMERY
    rec = _Recorder()
    monkeypatch.setattr(parallel, "lib", lambda: rec)

    class Curve:
        fe_bytes, default_glv, kind, _ctx, devices = 48, -1, "weierstrass", "ctx", [0]

    par = parallel._Parallel(Curve())
    data = bytes(range(64))
    arr = par.scalarsFromBytes(data)
    assert (arr.n, arr.kind) == (2, "scalars")
    name, args = rec.calls[-1]
    assert name == "msmz_upload_scalars" and args[:3] == ("ctx", data, 2)
    par.scalarsFromBytes(data, 1)
    assert rec.calls[-1][0] == "msmz_upload_scalars" and rec.calls[-1][1][2] == 1
    par.scalarsFromBytes(data, width=32, montgomery=False)
    assert rec.calls[-1][0] == "msmz_upload_scalars"
    pts = bytes(96 * 3)
    par.pointsFromBytes(pts)
    assert rec.calls[-1][0] == "msmz_upload_points" and rec.calls[-1][1][:4] == ("ctx", pts, None, 3)
    par.pointsFromBytes(pts, 2, b"\1\0")
    assert rec.calls[-1][0] == "msmz_upload_points" and rec.calls[-1][1][1:4] == (pts, b"\1\0", 2)
    par.pointsFromBytes(pts, montgomery=False)
    assert rec.calls[-1][0] == "msmz_upload_points"
    # the new forms
    arr = par.scalarsFromBytes(data, width=8)
    assert arr.n == 8 and rec.calls[-1][0] == "msmz_import_scalars"
    src = rec.calls[-1][1][1]._obj
    assert (src.width, src.stride, src.flags, src.stream, src.is_inf, rec.calls[-1][1][2]) == (8, 0, 0, None, None, 8)
    par.scalarsFromBytes(data, montgomery=True)
    src = rec.calls[-1][1][1]._obj
    assert rec.calls[-1][0] == "msmz_import_scalars" and (src.width, src.flags) == (32, MSMZ_SRC_MONTGOMERY)
    par.pointsFromBytes(pts, 3, b"\0\1\0", montgomery=True)
    src = rec.calls[-1][1][1]._obj
    assert rec.calls[-1][0] == "msmz_import_points" and (src.width, src.flags) == (96, MSMZ_SRC_MONTGOMERY) and src.is_inf
    for bad in (dict(width=36), dict(width=6), dict(width=8, montgomery=True)):
        with pytest.raises(ValueError):
            par.scalarsFromBytes(data, **bad)
    with pytest.raises(ValueError):
        par.scalarsFromBytes(data, 9, width=8)


def test_msm_batch_list_routes():
    """host byte vectors take the old route; a list holding a resident array still is a TypeError in batch_scalars, and
    only GPU tensors / resident arrays count as a device list"""
    from msm_zprize_amd.parallel import DeviceArray, batch_scalars, is_device_list
    res = DeviceArray(object(), 1, 8, "scalars")
    gpu = FakeTensor((8, 4), device=_Dev("cuda", 0))
    assert is_device_list([gpu, gpu]) and is_device_list([gpu, res])
    for other in ([b"\0" * 256], [res, b"\0" * 256], [FakeTensor((8, 4))], [], res, b"\0" * 32, [res, res]):
        assert not is_device_list(other)
    with pytest.raises(TypeError, match="resident arrays"):
        batch_scalars([res, res], 8)
    # a bare tensor is neither: (B, N) of int64 and (B * N, 32) of uint8 would both be plausible readings
    assert not is_device_list(FakeTensor((5, 8), device=_Dev("cuda", 0)))
    from msm_zprize_amd.parallel import _Parallel

    class Curve:
        fe_bytes, default_glv, kind, _ctx, devices = 48, -1, "weierstrass", None, [0]

    with pytest.raises(TypeError, match="bare tensor"):
        _Parallel(Curve()).msmBatch(FakeTensor((5, 8), device=_Dev("cuda", 0)), DeviceArray(object(), 1, 8, "points"), 8)


def test_package_imports_without_torch_and_without_the_oracle():
    """no module of the package imports torch at module level (scalarsFromTensor asks it for a stream lazily), and none
    imports the oracle"""
    pkg = os.path.join(ROOT, "msm_zprize_amd")
    top = re.compile(r"^(import|from)\s+(\S+)")
    for name in sorted(os.listdir(pkg)):
        if not name.endswith(".py"):
            continue
        for line in open(os.path.join(pkg, name)):
            m = top.match(line)   # (module level: no indentation)
            if m:
                mod = m.group(2).split(".")[0]
                assert mod != "torch", (name, line)
            assert not re.match(r"^\s*(import|from)\s+oracle\b", line), (name, line)
    code = ("import sys; import msm_zprize_amd, msm_zprize_amd.parallel; "
            "assert 'torch' not in sys.modules and 'oracle' not in sys.modules")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)

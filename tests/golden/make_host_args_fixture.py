"""The argument checks of msm_zprize_amd/parallel.py as a table of calls, good and bad, and what each one gives.

    python tests/golden/make_host_args_fixture.py        # writes tests/golden/host_args_parity.json

cases() lists (label, thunk, new): the thunk makes one call through public names only -- the module-level *_args
functions and the methods of Curve.Parallel that validate before they touch the library, on a fake curve with
DeviceArray(None, handle, n, kind) fakes and the group order 1009.  `new` is the message a later commit gives where it
deliberately unified a wording (None: the recorded message holds).  record() runs the table -> {label: {"ok": value} or
{"err": [class name, message]}}, bytes as hex.  host_args_parity.json is that record made at the commit BEFORE the host
bindings were restructured; tests/test_host_args_parity_cpu.py runs the same table on the code under test and compares."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "host_args_parity.json")
Q = 1009


class FakeDevice:
    def __init__(self, type_, index=None):
        self.type, self.index = type_, index

    def __str__(self):
        return self.type if self.index is None else f"{self.type}:{self.index}"

    def __eq__(self, other):
        return (self.type, self.index) == (other.type, other.index)


class FakeTensor:
    """the tensor attributes tensor_view reads"""

    def __init__(self, shape, item=4, strides=None, device=None, ptr=4096):
        self.shape = tuple(shape)
        self._item, self._ptr = item, ptr
        self._strides = tuple(strides) if strides is not None else \
            tuple(math.prod(shape[i + 1:]) for i in range(len(shape)))
        self.device = device or FakeDevice("cpu")

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        return self._strides[i]

    def element_size(self):
        return self._item

    def data_ptr(self):
        return self._ptr

    def __repr__(self):
        return f"T{list(self.shape)}x{self._item}s{list(self._strides)}@{self._ptr}/{self.device}"


class FakeCurve:
    params = {"order": Q}
    fe_bytes = 48
    devices = [0]
    kind = "weierstrass"
    default_glv = -1
    _ctx = None


def arr(n=100, handle=1, kind="scalars", tag=""):
    from msm_zprize_amd.parallel import DeviceArray
    a = DeviceArray(None, handle, n, kind)
    a.tag = tag
    return a


def desc(v):
    from msm_zprize_amd.parallel import DeviceArray
    if isinstance(v, DeviceArray):
        return f"<{v.kind}:{v.n}@{v.handle}{getattr(v, 'tag', '')}>"
    if isinstance(v, (bytes, bytearray, memoryview)):
        return f"b[{len(v)}]"
    if isinstance(v, (list, tuple)) and len(v) > 4 and all(isinstance(e, (bytes, bytearray)) for e in v):
        return f"[{len(v)} x {desc(v[0])}]"
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(desc(e) for e in v) + "]"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {desc(e)}" for k, e in v.items()) + "}"
    return repr(v)


def encode(v):
    from msm_zprize_amd.parallel import CheckResult, DeviceArray
    if isinstance(v, DeviceArray):
        return {"DeviceArray": [v.handle, v.n, v.kind]}
    if isinstance(v, (bytes, bytearray)):
        return {"hex": bytes(v).hex()}
    if isinstance(v, (list, tuple)):
        return [encode(e) for e in v]
    if isinstance(v, dict):
        return {str(k): encode(e) for k, e in v.items()}
    if isinstance(v, CheckResult):
        return repr(v)
    return v


def cases():
    import msm_zprize_amd.parallel as M
    P = M._Parallel(FakeCurve())
    out, seen = [], set()

    def add(fn, *args, new=None, **kw):
        name = getattr(fn, "__name__", str(fn))
        label = f"{name}({', '.join([desc(a) for a in args] + [f'{k}={desc(v)}' for k, v in kw.items()])})"
        if label not in seen:   # the loops below meet some calls twice
            seen.add(label)
            out.append((label, lambda: fn(*args, **kw), new))

    x, y, z, w = arr(100, 1), arr(80, 2), arr(60, 3), arr(100, 4)
    x2 = arr(100, 1, tag="'")                       # a second object for the handle of x
    pts, pts2, pre = arr(100, 11, "points"), arr(80, 12, "points"), arr(100, 13, "precomputed")
    wrong = [pts, None, 7, True, 1.5, b"x" * 32, "s"]
    bad_first = [-1, True, False, 1.0, "1", None]
    bad_n = [0, -1, True, 1.0, "1", 1 << 32, (1 << 32) + 5]

    # ---------------------------------------------------------------------------------------- the range block, 4 times
    # mulPoints: (scalars, points, N, addend, firstPoint, firstScalar, firstAddend, order)
    def mul(scalars=x, points=pts, N=None, addend=None, firstPoint=0, firstScalar=0, firstAddend=0):
        return M.mul_points_args(scalars, points, N, addend, firstPoint, firstScalar, firstAddend, Q)
    mul.__name__ = "mul_points_args"

    def fits(first, n, name, size):   # the unified wording of "N does not fit"
        return f"entries [{first}, +{n}) from {name} of an array of {size}"

    add(mul)
    add(mul, N=40, addend=pts2, firstPoint=60, firstScalar=60, firstAddend=40)
    add(mul, 5), add(mul, 0), add(mul, Q - 1), add(mul, Q), add(mul, -1), add(mul, 1 << 300)
    add(mul, 5, addend=pts, firstPoint=50, N=50)
    add(mul, 5, N=1 << 32, new="mulPoints: " + fits(0, 1 << 32, "firstPoint", 100))
    add(mul, 5, N=(1 << 32) + 1, new="mulPoints: " + fits(0, (1 << 32) + 1, "firstPoint", 100))
    add(mul, x, arr(1 << 33, 14, "points"), 1 << 32, new="mulPoints: " + fits(0, 1 << 32, "firstScalar", 100))
    add(mul, arr(1 << 33, 5), arr(1 << 33, 14, "points"), 1 << 32)     # mulPoints has no bound on N
    for v in wrong:
        if v is not None:
            add(mul, addend=v)
        if v is not pts:
            add(mul, points=v)
        if not (isinstance(v, int) and not isinstance(v, bool)):
            add(mul, scalars=v)
    add(mul, points=pre), add(mul, addend=pre), add(mul, addend=x), add(mul, scalars=pre)
    for name, size in (("firstPoint", 100), ("firstScalar", 100), ("firstAddend", 80)):
        for v in bad_first + [size, size + 1, size - 1, 1]:
            add(mul, addend=pts2, **{name: v})
    add(mul, firstAddend=1), add(mul, 5, firstScalar=1), add(mul, 5, firstScalar=0), add(mul, 5, firstScalar=True)
    for v in bad_n:
        add(mul, N=v, new="mulPoints: " + fits(0, v, "firstPoint", 100) if type(v) is int and v > 100 else None)
    add(mul, N=100), add(mul, N=101, new="mulPoints: " + fits(0, 101, "firstPoint", 100))
    add(mul, N=81, addend=pts2, new="mulPoints: " + fits(0, 81, "firstAddend", 80))
    add(mul, N=80, addend=pts2), add(mul, N=51, firstScalar=50, new="mulPoints: " + fits(50, 51, "firstScalar", 100))
    add(mul, N=41, firstPoint=60, firstScalar=70, new="mulPoints: " + fits(60, 41, "firstPoint", 100))
    add(mul, N=31, firstPoint=60, firstScalar=70, new="mulPoints: " + fits(70, 31, "firstScalar", 100))
    # double faults: which one is reported
    add(mul, points=x, addend=x, scalars=pts), add(mul, addend=x, scalars=None), add(mul, Q, addend=7)
    add(mul, Q, firstPoint=-1), add(mul, firstPoint=-1, firstScalar=-2, N=0), add(mul, firstScalar=100, firstPoint=100)
    add(mul, firstAddend=3, firstPoint=200), add(mul, N=0, firstPoint=100), add(mul, N=True, firstAddend=1)
    add(mul, N=200, addend=pts2, firstAddend=79, new="mulPoints: " + fits(0, 200, "firstPoint", 100))

    # combineScalars: (a, x, b, y, N, firstX, firstY, out, firstOut, firstA, firstB, order, who)
    def comb(a=1, x=x, b=None, y=None, N=None, firstX=0, firstY=0, out=None, firstOut=0, firstA=0, firstB=0, **kw):
        return M.combine_scalars_args(a, x, b, y, N, firstX, firstY, out, firstOut, firstA, firstB, Q, **kw)
    comb.__name__ = "combine_scalars_args"

    add(comb), add(comb, 5), add(comb, 0), add(comb, Q - 1, x, 1, y), add(comb, z, x, w, y), add(comb, z, x, 3, y, out=w)
    add(comb, 2, x, 3, y, 40, 10, 20, w, 30), add(comb, z, x, w, y, 20, 1, 2, x, 3, 4, 5)
    add(comb, who="innerProduct"), add(comb, 1, x, 1, y, who="innerProduct"), add(comb, 1, pts, who="innerProduct")
    add(comb, 1, x, 1, y, 81, who="innerProduct"), add(comb, 1, x, None, None, None, 100, who="innerProduct")
    for v in wrong:
        if v is not None:
            add(comb, out=v), add(comb, 1, x, 1, v)
        add(comb, 1, v)
        if not (isinstance(v, int) and not isinstance(v, bool)):
            add(comb, v), add(comb, 1, x, v, y)
    add(comb, 1, x, 1), add(comb, 1, x, None, y), add(comb, Q), add(comb, -1), add(comb, 1, x, Q, y), add(comb, 1, x, 1 << 256, y)
    for name, size in (("firstX", 100), ("firstY", 80), ("firstA", 60), ("firstB", 100), ("firstOut", 100)):
        for v in bad_first + [size, size + 1, size - 1, 1]:
            add(comb, z, x, w, y, out=x2, N=1, **{name: v})
    for name in ("firstY", "firstA", "firstB", "firstOut"):
        add(comb, **{name: 1}), add(comb, **{name: True}), add(comb, **{name: 0})
    add(comb, 3, x, 4, y, firstA=1), add(comb, 3, x, 4, y, firstB=2), add(comb, 3, x, z, y, firstB=59)
    for v in bad_n + [100, 101]:
        add(comb, N=v)
    add(comb, 1, x, 1, y, 80), add(comb, 1, x, 1, y, 81), add(comb, z, x, 1, y, 61), add(comb, 1, x, 1, y, 51, 0, 30)
    add(comb, 1, x, 1, y, out=z, N=61), add(comb, 1, x, 1, y, out=z, N=41, firstOut=20), add(comb, 1, x, 1, y, out=z, firstOut=20)
    for o in (x, x2):
        for d in (0, 1, 39, 40):
            add(comb, 1, x, N=40, out=o, firstOut=d), add(comb, 1, x, N=40, firstX=40, out=o, firstOut=40 - d)
            add(comb, o, w, N=40, firstA=10, out=x, firstOut=10 + d), add(comb, 1, w, 1, o, N=40, firstY=5, out=x, firstOut=5 + d)
            add(comb, 2, w, x, o, N=40, firstB=d, out=o)
    add(comb, 1, x, 1, x, 40, 0, 40, x, 20), add(comb, 1, x, 1, x, 40, 0, 40, x, 40), add(comb, 1, x, 1, x, 40, 1, 40, x, 0)
    # double faults
    add(comb, None, pts), add(comb, None, x, 1), add(comb, 1, x, 1, pts, out=7), add(comb, Q, x, None, y), add(comb, Q, x, out=7)
    add(comb, Q, x, Q + 1, y), add(comb, 1.5, x, Q, y), add(comb, Q, firstX=-1), add(comb, firstX=-1, firstOut=-2, N=0)
    add(comb, firstX=100, firstA=1), add(comb, firstA=1, firstX=100), add(comb, firstB=1, firstA=1), add(comb, N=0, firstOut=1)
    add(comb, N=101, out=x, firstOut=1), add(comb, 1, x, 1, y, 90, out=x, firstOut=5), add(comb, N=True, out=x, firstOut=1)
    add(comb, 1, x, 1, x2, 40, 1, 2, x, 0), add(comb, 1, x, 1, y, 81, out=z)

    # scalarRecurrence: (a, b, N, init, reverse, exclusive, firstA, firstB, out, firstOut, order, who)
    def rec(a=x, b=y, N=None, init=None, reverse=False, exclusive=False, firstA=0, firstB=0, out=None, firstOut=0, **kw):
        return M.scalar_recurrence_args(a, b, N, init, reverse, exclusive, firstA, firstB, out, firstOut, Q, **kw)
    rec.__name__ = "scalar_recurrence_args"

    add(rec), add(rec, None, x), add(rec, x, None, exclusive=True), add(rec, 7, y, reverse=True, exclusive=True, init=0)
    add(rec, 5, None, 10), add(rec, 0, None, 10), add(rec, Q - 1, y, init=Q - 1, reverse=True), add(rec, x, y, firstA=30, firstB=20)
    add(rec, x, y, 50, out=x), add(rec, who="prefixSums"), add(rec, None, None, 5, who="prefixSums")
    for v in wrong:
        if v is not None:
            add(rec, v, y), add(rec, x, y, out=v)
            add(rec, x, v)
        if not (isinstance(v, int) and not isinstance(v, bool)) and v is not None:
            add(rec, init=v)
    add(rec, x, 7), add(rec, None, None, 5), add(rec, None, None), add(rec, reverse=1), add(rec, exclusive=0), add(rec, exclusive=None)
    for v in (Q, -1, 1 << 256):
        add(rec, v, y), add(rec, init=v)
    add(rec, 3, None), add(rec, 3, None, out=w), add(rec, None, None, out=w)
    for name, size in (("firstA", 100), ("firstB", 80), ("firstOut", 100)):
        for v in bad_first + [size, size + 1, size - 1, 1]:
            add(rec, out=x2, N=1, **{name: v})
    add(rec, 3, y, firstA=2), add(rec, x, None, firstB=2), add(rec, x, None, firstOut=2), add(rec, None, y, firstA=True)
    for v in bad_n + [80, 81]:
        add(rec, N=v)
    add(rec, N=51, firstA=50), add(rec, N=10, firstB=71), add(rec, N=10, out=y, firstOut=71), add(rec, 3, None, 1 << 32)
    for o in (x, x2):
        for d in (0, 1, 39, 40):
            add(rec, x, None, 40, out=o, firstOut=d), add(rec, None, x, 40, firstB=40, out=o, firstOut=40 - d)
            add(rec, w, o, 40, firstB=d, out=o, firstOut=0)
    add(rec, x, x, 40, firstA=0, firstB=50, out=x, firstOut=50), add(rec, x, x, 40, firstA=0, firstB=50, out=x, firstOut=25)
    # double faults
    add(rec, pts, pts), add(rec, None, None, out=7), add(rec, x, y, out=7, init=1.5), add(rec, init=True, reverse=1)
    add(rec, reverse=1, exclusive=1), add(rec, Q, y, init=Q), add(rec, Q, y, reverse=1), add(rec, 3, None, firstA=1)
    add(rec, 3, None, 0), add(rec, firstA=-1, firstB=-1, N=0), add(rec, firstB=80, firstA=100), add(rec, N=0, firstOut=1)
    add(rec, x, None, 101, out=x, firstOut=1), add(rec, x, None, True, out=x, firstOut=1), add(rec, init=Q, firstA=-1)

    # invertScalars: (x, N, first, out, firstOut, who)
    def inv(x=x, N=None, first=0, out=None, firstOut=0, **kw):
        return M.invert_scalars_args(x, N, first, out, firstOut, **kw)
    inv.__name__ = "invert_scalars_args"

    add(inv), add(inv, x, None, 30, y, 20), add(inv, x, 50, 0, x, 0), add(inv, x, 50, 0, x, 50), add(inv, who="batchInverse", N=0)
    for v in wrong:
        add(inv, v)
        if v is not None:
            add(inv, out=v)
    for name, size in (("first", 100), ("firstOut", 80)):
        for v in bad_first + [size, size + 1, size - 1, 1]:
            add(inv, out=y, N=1, **{name: v})
    add(inv, firstOut=1), add(inv, firstOut=True), add(inv, firstOut=0)
    for v in bad_n + [100, 101]:
        add(inv, N=v)
    add(inv, N=2, first=99), add(inv, N=10, out=y, firstOut=71), add(inv, N=81, out=y)
    for o in (x, x2):
        for d in (0, 1, 39, 40):
            add(inv, x, 40, 0, o, d), add(inv, x, 40, 40, o, 40 - d)
    add(inv, pts, out=pts), add(inv, None, 0), add(inv, first=-1, firstOut=-1), add(inv, first=100, N=0), add(inv, N=0, firstOut=3)
    add(inv, x, 101, 0, x, 1), add(inv, x, True, 0, x, 1), add(inv, x, 60, 50, x, 49)

    # ------------------------------------------------------------------------------------- the other module functions
    add(M.check_points_args, pts, None, True, 0), add(M.check_points_args, pts, 10, False, 90), add(M.check_points_args, pts, 1, 1, 99)
    for v in wrong + [pre, x]:
        if v is not pts:
            add(M.check_points_args, v, None, True, 0)
    for v in bad_first + [100, 101, 99]:
        add(M.check_points_args, pts, None, True, v)
    for v in bad_n + [100, 101]:
        add(M.check_points_args, pts, v, True, 0)
    add(M.check_points_args, pts, 11, True, 90), add(M.check_points_args, x, 0, True, -1), add(M.check_points_args, pts, 0, True, -1)
    add(M.check_points_args, pts, 0, True, 100)

    seg = M.msm_segments_args
    add(seg, x, pts, [(0, 0, 100)]), add(seg, x, pre, [(50, 0, 50), (0, 50, 50)]), add(seg, y, pts, ((20, 0, 80), [0, 79, 1], (0, 0, 1)))
    for v in wrong:
        if v is not pts:
            add(seg, x, v, [(0, 0, 1)])
        add(seg, v, pts, [(0, 0, 1)])
    add(seg, pre, pts, [(0, 0, 1)]), add(seg, pts, x, [(0, 0, 1)]), add(seg, 7, 7, 7)
    for v in (None, 7, "abc", b"abc", x, iter([(0, 0, 1)]), [], (), [(0, 0)], [(0, 0, 1, 1)], ["abc"], [b"abc"], [7], [None],
              [(0, 0, 1), 7], {}, {(0, 0, 1): 1}):
        if not hasattr(v, "__next__"):
            add(seg, x, pts, v)
    for bad in (-1, True, 1.0, "1", None):
        for k in range(3):
            s = [0, 0, 1]
            s[k] = bad
            add(seg, x, pts, [(0, 0, 1), tuple(s)])
    add(seg, x, pts, [(0, 0, 0)]), add(seg, x, pts, [(0, 0, 101)]), add(seg, x, pts, [(1, 0, 100)]), add(seg, x, pts, [(0, 1, 100)])
    add(seg, y, pts, [(0, 0, 81)]), add(seg, y, pts, [(20, 1, 80)]), add(seg, x, pts, [(-1, -1, 0)]), add(seg, x, pts, [(100, 100, 1)])
    add(seg, x, pts, [(0, 0, 1 << 64)]), add(seg, x, pts, [(1 << 64, 0, 1)])

    for v in (None, "curve", "subgroup", "both", "", 0, 1, True, b"curve"):
        add(M.check_arg, v, "pointsFromBytes")
    add(M.check_arg, "x", "pointsFromTensor")

    pc = M.precompute_args
    add(pc, pts, 100, {}, 0), add(pc, pts, 1, {"c": 16, "glv": 1, "scalarBits": 64}, 2), add(pc, pts, 50, {"c": None, "glv": 0}, 3)
    add(pc, pts, 50, {"c": 24, "glv": -1}, (1 << 32) - 1), add(pc, pts, 50, {"c": True, "glv": True}, 0)
    for v in wrong + [pre]:
        if v is not pts:
            add(pc, v, 10, {}, 0)
    for v in bad_n[:5] + [101, None]:
        add(pc, pts, v, {}, 0)
    for v in (1, -1, True, 2.0, "2", None, 1 << 32):
        add(pc, pts, 10, {}, v)
    for o in ({"c": 25}, {"c": -1}, {"c": "x"}, {"c": "16"}, {"c": 1}, {"glv": 2}, {"glv": -2}, {"glv": "x"}, {"glv": None}, {"scalarBits": 257},
              {"scalarBits": -1}, {"scalarBits": True}, {"scalarBits": 0}, {"scalarBits": 256}, {"scalarBits": None}, {"scalarBits": 1.0}):
        add(pc, pts, 10, o, 0)
    add(pc, x, 0, {"c": 25}, 1), add(pc, pts, 0, {"c": 25}, 1), add(pc, pts, 10, {"c": 25}, 1), add(pc, pts, 10, {"c": 25, "glv": 2}, 0)
    add(pc, pts, 10, {"glv": 2, "scalarBits": 300}, 0)

    for o in ({}, {"scalarBits": None}, {"scalarBits": 0}, {"scalarBits": 1}, {"scalarBits": 256}, {"scalarBits": 257}, {"scalarBits": -1},
              {"scalarBits": True}, {"scalarBits": 64.0}, {"scalarBits": "64"}):
        add(M.scalar_bits_arg, o, "msm")
    add(M.scalar_bits_arg, {"scalarBits": 300}, "msmSegments")

    for v in (4, 8, 32, 28, 0, 2, 6, 36, 33, True, 8.0, "8", None, -4):
        add(M.scalar_width_arg, v, False, "scalarsFromBytes")
    add(M.scalar_width_arg, 32, True, "scalarsFromBytes"), add(M.scalar_width_arg, 8, True, "scalarsFromTensor")
    add(M.scalar_width_arg, 6, True, "scalarsFromTensor")

    gpu, gpu1, cpu = FakeDevice("cuda", 0), FakeDevice("cuda", 1), FakeDevice("cpu")
    tg = FakeTensor((4, 8), device=gpu)
    for v in (x, b"abc", bytearray(3), "abc", 7, None, [], [x], [x, y], [b"a" * 32], [tg], [tg, x], [x, tg], [tg, b"a" * 32],
              [FakeTensor((4, 8))], (tg, tg), tg, [FakeTensor((4, 8), device=gpu1)]):
        add(M.is_device_list, v)

    tv = M.tensor_view
    add(tv, FakeTensor((5, 8)), [0], "scalars", 48, False, "scalarsFromTensor")
    add(tv, FakeTensor((5,), item=8), [0], "scalars", 48, False, "scalarsFromTensor")
    add(tv, FakeTensor((5, 2), item=4, strides=(12, 1)), [0], "scalars", 48, False, "scalarsFromTensor")
    add(tv, FakeTensor((1, 8), strides=(999, 1)), [0], "scalars", 48, True, "scalarsFromTensor")
    add(tv, FakeTensor((3, 96), item=1), [0], "points", 48, True, "pointsFromTensor")
    add(tv, FakeTensor((3, 96), item=1), [0], "points", 48, False, "pointsFromTensor", FakeTensor((3,), item=1))
    add(tv, FakeTensor((3, 96), item=1), [0], "points", 48, False, "pointsFromTensor", FakeTensor((5,), item=1))
    for t in (7, b"abc", None, [1, 2], x):
        add(tv, t, [0], "scalars", 48, False, "scalarsFromTensor")
    for t in (FakeTensor((5, 8), strides=(16, 2)), FakeTensor((5,), item=4), FakeTensor((5, 2, 2)), FakeTensor((0, 8)), FakeTensor((5, 9)),
              FakeTensor((5, 1), item=2), FakeTensor((5, 2), item=8, strides=(1, 1)), FakeTensor((5, 8), ptr=0), FakeTensor((5, 8), ptr=4098),
              FakeTensor((5, 2), item=4, strides=(1 << 22, 1)), FakeTensor((5, 3), item=2, strides=(3, 1)),
              FakeTensor((5, 8), device=FakeDevice("meta")), FakeTensor((5, 8), device=gpu1), FakeTensor((5, 4), item=4)):
        add(tv, t, [0], "scalars", 48, False, "scalarsFromTensor")
        add(tv, t, [0], "scalars", 48, True, "scalarsInto")
    for t in (FakeTensor((3,), item=8), FakeTensor((3, 95), item=1), FakeTensor((3, 64), item=1), FakeTensor((3, 24), item=4, strides=(25, 1))):
        add(tv, t, [0, 1], "points", 48, False, "pointsFromTensor")
    add(tv, FakeTensor((5, 8)), [0], "scalars", 48, False, "scalarsFromTensor", FakeTensor((5,), item=1))
    for f in (FakeTensor((2,), item=1), FakeTensor((3,), item=4), FakeTensor((3, 1), item=1), FakeTensor((3,), item=1, strides=(2,)),
              FakeTensor((3,), item=1, device=gpu)):
        add(tv, FakeTensor((3, 96), item=1), [0], "points", 48, False, "pointsFromTensor", f)

    bs = M.batch_scalars
    v32 = [bytes(64)] * 3
    add(bs, x, 10), add(bs, x, 10, 3), add(bs, x, 100), add(bs, x, 101), add(bs, x, 10, 11), add(bs, x, 10, 0), add(bs, x, 10, -1)
    add(bs, x, 10, "3"), add(bs, pts, 10), add(bs, x, 0), add(bs, x, -1), add(bs, pts, 0), add(bs, v32, 2), add(bs, v32, 1), add(bs, v32, 3)
    add(bs, v32, 2, 3), add(bs, v32, 2, 2), add(bs, [bytes(64), bytes(96)], 2), add(bs, [], 2), add(bs, (), 2), add(bs, b"abc", 2)
    add(bs, "abc", 2), add(bs, 7, 2), add(bs, None, 2), add(bs, [x], 2), add(bs, [x, bytes(64)], 2), add(bs, [bytearray(64), memoryview(bytes(64))], 2)
    add(bs, [bytes(64), 7], 2), add(bs, [x], 0)

    out.append(("CheckResult repr ok", lambda: repr(M.CheckResult(True, 0, 0, None)), None))
    out.append(("CheckResult repr bad", lambda: repr(M.CheckResult(False, 2, 1, 5, b"\x01")), None))

    # --------------------------------------------------------- methods that validate before they touch the library
    for r, n, b in ((True, 4, 1), (1.5, 4, 1), ("2", 4, 1), (None, 4, 1), (-1, 4, 1), (Q, 4, 1), (2, 4, True), (2, 4, 2.0), (2, 4, Q), (2, 4, -1),
                    (2, 0, 1), (2, -1, 1), (2, True, 1), (2, 1.0, 1), (2, 1 << 32, 1), (2, None, 1), (True, 0, Q), (Q, 0, 1.5), (Q, 0, Q),
                    (2, 0, Q), (1.5, True, True)):
        add(P.scalarPowers, r, n, b)
    add(P.scalarPowers, Q, 4)
    for p, zz, kw in ((y, True, {}), (y, 1.5, {}), (y, None, {}), (y, "5", {}), (pts, 5, {}), (None, 5, {}), (7, 5, {}), (pts, 1.5, {}),
                      (y, Q, {}), (y, -1, {}), (y, 5, {"N": 0}), (y, 5, {"N": 81}), (y, 5, {"first": 80}), (y, 5, {"first": -1}),
                      (y, 5, {"N": True}), (y, 5, {"N": 41, "first": 40}), (y, Q, {"N": 0})):
        add(P.divideByLinear, p, zz, **kw)
    t58 = FakeTensor((5, 8))
    for d in wrong:
        add(P.scalarsInto, d, 0, t58)
    add(P.scalarsInto, pts, 0, 7), add(P.scalarsInto, x, 0, 7), add(P.scalarsInto, x, 0, FakeTensor((5, 9))), add(P.scalarsInto, x, -1, 7)
    for v in bad_first + [96, 100, 1 << 40]:
        add(P.scalarsInto, x, v, t58)
    add(P.scalarsInto, x, 0, FakeTensor((5, 2), item=4), True), add(P.scalarsInto, x, -1, FakeTensor((0, 8)))
    for data, kw in ((bytes(96), {"check": "both"}), (bytes(96), {"check": 1}), (bytes(95), {}), (bytes(0), {}), (bytes(96), {"n": 2}),
                     (bytes(96), {"n": 0}), (bytes(96), {"n": -1}), (bytes(192), {"n": 2, "is_inf": b"\x00"}), (bytes(95), {"check": "curve"}),
                     (bytes(95), {"check": "bogus"}), (bytes(96), {"n": 2, "is_inf": b"", "check": "subgroup"}), (bytes(96), {"n": 2, "montgomery": True}),
                     (bytes(192), {"n": 2, "is_inf": b"\x00", "montgomery": True}), (bytearray(10), {"n": 1})):
        add(P.pointsFromBytes, data, **kw)
    for data, kw in ((bytes(31), {}), (bytes(0), {}), (bytes(32), {"n": 2}), (bytes(32), {"n": 0}), (bytes(32), {"n": -1}), (bytes(32), {"width": 6}),
                     (bytes(32), {"width": 36}), (bytes(32), {"width": True}), (bytes(32), {"width": 8, "montgomery": True}),
                     (bytes(32), {"width": 8, "n": 5}), (bytes(3), {"width": 4}), (bytes(32), {"width": 0, "n": 0}), (bytes(31), {"montgomery": True}),
                     (bytes(32), {"width": 6, "montgomery": True, "n": 0})):
        add(P.scalarsFromBytes, data, **kw)
    for s, p, n, o in ((x, pts, 0, None), (x, pts, -1, None), (x, pts, 101, None), (y, pts, 81, None), (bytes(64), pts, 3, None),
                       (bytes(63), pts, 2, None), (x, pts, 0, {"scalarBits": 300}), (x, pts, 10, {"scalarBits": 300}), (x, pts, 10, {"scalarBits": True}),
                       (x, pts, 0, {"c": "x"}), (x, pts, 0, {"glv": "x", "scalarBits": 300}), (x, pts, 0, {"useSafeAdditions": "x"}),
                       (x, pts, 0, {"reduceAffine": "x"}), (y, pts, 101, None), (bytes(0), pts, 1, {})):
        add(P.msm, s, p, n, False, o)
        add(P.msmUnsafe, s, p, n, True, o)
    add(P.msmProjective, x, pts, 0), add(P.msmProjective, x, pts, 0, {"scalarBits": -1}), add(P.msmProjective, bytes(32), pts, 2, {"glv": "x"})
    bare = FakeTensor((4, 8), device=gpu)
    for s, p, n, o in ((bare, pts, 4, None), (FakeTensor((4, 8)), pts, 4, None), (bare, pts, 0, None), (bare, pts, 101, {"scalarBits": 300}),
                       (x, pts, 0, None), (x, pts, 101, None), ([], pts, 4, None), ([x], pts, 4, None), (pts, pts, 4, None), (b"abc", pts, 4, None),
                       (x, pts, 10, {"scalarBits": 300}), (x, pts, 10, {"batch": 11, "scalarBits": 300}), (v32, pts, 2, {"scalarBits": -1}),
                       (v32, pts, 3, {"scalarBits": -1}), (x, pts, 10, {"c": "x"}), (x, pts, 10, {"buckets": "x"}), (x, pts, 10, {"glv": None}),
                       ([bare, x], pts, 200, None)):
        add(P.msmBatch, s, p, n, o)
        add(P.msmBatchUnsafe, s, p, n, o)
    for s, p, g, o in ((x, pts, [], None), (x, x, [(0, 0, 1)], None), (b"", pts, [(0, 0, 1)], {"scalarBits": 300}), (x, pts, [(0, 0, 101)], {"scalarBits": 300}),
                       (x, pts, [(0, 0, 1)], {"scalarBits": 300}), (x, pts, [(0, 0, 1)], {"c": "x"}), (x, pre, [(0, 0, 1)], {"buckets": []}),
                       (x, pts, [(0, 0, 1)], {"useSafeAdditions": "x", "scalarBits": 300})):
        add(P.msmSegments, s, p, g, o)
        add(P.msmSegmentsUnsafe, s, p, g, o)
    for p, n, o, f in ((x, 10, None, 0), (pts, 0, None, 0), (pts, 10, None, 1), (pts, 10, {"c": 25}, 0), (pts, 10, {"glv": 2}, 0),
                       (pts, 10, {"scalarBits": 300}, 0), (pts, 101, {"scalarBits": 300}, 1), (pre, 10, {}, 0)):
        add(P.precomputePoints, p, n, o, f)
    add(P.checkPoints, x), add(P.checkPoints, pts, 0), add(P.checkPoints, pts, None, True, 100), add(P.checkPoints, pts, 5, first=96, verdicts=True)
    add(P.mulPoints, 5, x), add(P.mulPoints, Q, pts), add(P.mulPoints, x, pts, 101, new="mulPoints: " + fits(0, 101, "firstPoint", 100))
    add(P.mulPoints, x, pts, addend=pts2, firstAddend=80), add(P.mulPoints, True, pts)
    add(P.combineScalars, 1, pts), add(P.combineScalars, Q, x), add(P.combineScalars, 1, x, N=101), add(P.combineScalars, 1, x, N=40, out=x, firstOut=1)
    add(P.innerProduct, pts), add(P.innerProduct, x, pts), add(P.innerProduct, x, y, 81), add(P.innerProduct, x, None, None, 100), add(P.innerProduct, x, firstY=1)
    add(P.scalarRecurrence, None, None), add(P.scalarRecurrence, Q, y), add(P.scalarRecurrence, x, y, 40, out=x, firstOut=1)
    add(P.prefixProducts, pts), add(P.prefixProducts, x, 101), add(P.prefixProducts, x, 40, out=x, firstOut=1), add(P.prefixProducts, x, first=100)
    add(P.prefixSums, pts), add(P.prefixSums, x, 0), add(P.prefixSums, x, 40, first=61), add(P.prefixSums, x, init=Q)
    add(P.invertScalars, pts), add(P.invertScalars, x, 101), add(P.invertScalars, x, 40, out=x, firstOut=39), add(P.invertScalars, x, out=7)

    return out


def record(table=None):
    res = {}
    for label, thunk, new in (cases() if table is None else table):
        try:
            res[label] = {"ok": encode(thunk())}
        except Exception as e:   # noqa: BLE001 -- whatever the call raises is what is recorded
            res[label] = {"err": [type(e).__name__, str(e)]}
    return res


if __name__ == "__main__":
    rec = record()
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} cases ({sum('err' in v for v in rec.values())} refused) -> {OUT}")

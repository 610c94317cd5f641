"""Exports on the GPU (msmz_export_scalars / msmz_export_points; scalarsToTensor, pointsToTensor, scalarsToBytes,
pointsToBytes): every form against Python integers and against the downloads, byte for byte, into host and device
memory, packed and strided, with the bytes around the records checked; round trips through the imports; the range and
argument errors; pinned host memory; a destination behind a torch stream; a two-engine context on one GPU.  Device
memory comes from torch tensors.

These cases run in a child process of their own (tests/test_export_gpu.py starts it): torch carries its own copy of the
HIP runtime, and a process may hold only one -- whichever is loaded first serves both, so torch is imported here before
anything loads libmsmz.so.

Not tested on purpose, as in the import cases: a pageable host pointer passed WITH MSMZ_SRC_DEVICE, and a device range
that runs off its allocation into memory the process owns.  The engine's pointer classification (ResidentSets::vouch,
reused unchanged) must refuse them; if it were wrong the kernel would fault the GPU, and no test here may be able to do
that."""
import torch as _torch_first  # noqa: F401  (before libmsmz.so: one HIP runtime per process, see above)

import ctypes as C
import random

import pytest

from oracle import c_oracle
from oracle import params as P

pytestmark = pytest.mark.gpu

ALL = ["bls12-377", "pallas", "bls12-381", "ed-on-bls12-377"]
WEIER = ALL[:3]
MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
R256 = 1 << 256
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)   # one lane, around one wave, around one workgroup, several workgroups
FIRST = 7                                      # off a wave boundary
TOTAL = FIRST + max(SIZES) + 5


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


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


def _L():
    from msm_zprize_amd._native import lib
    return lib()


def _strip(p):
    return {"x": p["x"], "y": p["y"], "isZero": bool(p.get("isZero", False))}


def _enc(vals, width=32):
    return b"".join(int(v).to_bytes(width, "little") for v in vals)


def _scalars(top, n, seed):
    """n seeded values below `top`, with top - 1, 0 and 1 at FIRST, FIRST + 1, FIRST + 2 and top - 1 at the end"""
    rng = random.Random(seed)
    s = [rng.randrange(top) for _ in range(n)]
    for i, v in zip((FIRST, FIRST + 1, FIRST + 2, n - 1), (top - 1, 0, 1, top - 1)):
        if 0 <= i < n:
            s[i] = v
    return s


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _dest(torch, n, width, device, strided):
    """(whole, out): `out` = n rows of `width` bytes inside `whole`, all 0xA5, with a guard row before and after; strided:
    rows width + 24 bytes apart and the record 8 bytes into its row"""
    whole = torch.full((n + 2, width + 24 if strided else width), 0xA5, dtype=torch.uint8, device=device)
    return whole, (whole[1:n + 1, 8:8 + width] if strided else whole[1:n + 1])


def _holds(whole, n, width, strided, want):
    """`whole` holds the n records of `want` where _dest put `out`, and 0xA5 everywhere else"""
    row = width + 24 if strided else width
    exp = bytearray(b"\xa5" * (row * (n + 2)))
    at = 8 if strided else 0
    for i in range(n):
        exp[(i + 1) * row + at:(i + 1) * row + at + width] = want[i * width:(i + 1) * width]
    return _bytes(whole) == bytes(exp)


def _dst(ptr, stride=0, width=32, flags=0, stream=None, is_inf=None):
    from msm_zprize_amd._native import MsmzDst
    return MsmzDst(ptr, stride, width, flags, stream, is_inf)


def _download_scalars(curve, handle, first, n):
    buf = C.create_string_buffer(32 * n)
    assert _L().msmz_download_scalars(curve._ctx, handle, first, n, buf) == 0
    return buf.raw


def _download_points(curve, handle, first, n):
    buf, inf = C.create_string_buffer(2 * curve.fe_bytes * n), C.create_string_buffer(n)
    assert _L().msmz_download_points(curve._ctx, handle, first, n, buf, inf) == 0
    return buf.raw, inf.raw


def _download_compressed(curve, handle, first, n, flag):
    buf, inf = C.create_string_buffer(curve.fe_bytes * n), C.create_string_buffer(n)
    assert _L().msmz_download_points_compressed(curve._ctx, handle, first, n, buf, inf, flag) == 0
    return buf.raw, inf.raw


def _plant(curve, arr, index, value):
    """make `value` (>= q) entry `index` of a resident set, through a refused msmz_import_scalars_into (which converts
    before it reports: tests/test_scalar_ops_gpu.py)"""
    from msm_zprize_amd._native import MsmzSrc
    raw = _enc([value])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _L().msmz_import_scalars_into(curve._ctx, arr.handle, index, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert curve.Scalar.toBigints(arr, index, 1) == [value]


# ---------------------------------------------------------------------------------------------- 1. scalar forms
@pytest.mark.parametrize("label", ALL)
def test_scalar_forms(curves, torch, label):
    """widths 4, 8, 16, 32 x packed / strided x host / device destination x every size: the records are the planted
    values (0, 1, 2^(8 width) - 1 capped at q - 1, seeded ones), every byte around them is still 0xA5; Montgomery records
    are v * 2^256 mod q; the host export with flags 0, width 32, stride 0 is the download"""
    curve = curves(label)
    q = P.CURVES[label]["order"]
    par = curve.Parallel
    for width in (4, 8, 16, 32):
        vals = _scalars(min(q, 1 << (8 * width)), TOTAL, 10 * width)
        arr = par.scalarsFromBytes(_enc(vals), TOTAL)
        for n in SIZES:
            want = _enc(vals[FIRST:FIRST + n], width)
            for device in ("cpu", "cuda"):
                for strided in (False, True):
                    whole, out = _dest(torch, n, width, device, strided)
                    assert par.scalarsToTensor(arr, out, first=FIRST) is out
                    assert _holds(whole, n, width, strided, want), (width, n, device, strided)
            assert par.scalarsToBytes(arr, FIRST, n, width=width) == want, (width, n)
        # a new tensor on the GPU; fewer entries than `out` has rows: the rows behind them stay
        t = par.scalarsToTensor(arr, first=FIRST, N=65, width=width)
        assert t.device.type == "cuda" and tuple(t.shape) == (65, width) and _bytes(t) == _enc(vals[FIRST:FIRST + 65], width)
        whole, out = _dest(torch, 65, width, "cuda", True)
        par.scalarsToTensor(arr, out, first=FIRST, N=64)
        assert _holds(whole, 65, width, True, _enc(vals[FIRST:FIRST + 64], width) + b"\xa5" * width)
        if width == 8:   # 1-D tensors of an 8-byte dtype, also as a column of a wider matrix
            for device in ("cpu", "cuda"):
                t = torch.full((257,), -1, dtype=torch.int64, device=device)
                par.scalarsToTensor(arr, t, first=FIRST)
                assert _bytes(t) == _enc(vals[FIRST:FIRST + 257], 8)
                m = torch.full((257, 3), -1, dtype=torch.int64, device=device)
                par.scalarsToTensor(arr, m[:, 1], first=FIRST)
                assert _bytes(m[:, 1]) == _enc(vals[FIRST:FIRST + 257], 8)
                assert _bytes(m[:, 0]) == _bytes(m[:, 2]) == b"\xff" * (8 * 257)
        if width == 32:
            for n in SIZES:
                mont = _enc([v * R256 % q for v in vals[FIRST:FIRST + n]])
                for device in ("cpu", "cuda"):
                    for strided in (False, True):
                        whole, out = _dest(torch, n, 32, device, strided)
                        par.scalarsToTensor(arr, out, first=FIRST, montgomery=True)
                        assert _holds(whole, n, 32, strided, mont), (n, device, strided)
                assert par.scalarsToBytes(arr, FIRST, n, montgomery=True) == mont
                # flags 0, width 32, stride 0, host: the download, byte for byte
                buf = C.create_string_buffer(32 * n)
                d = _dst(C.addressof(buf), 0, 32)
                assert _L().msmz_export_scalars(curve._ctx, arr.handle, FIRST, n, C.byref(d)) == 0
                assert buf.raw == _download_scalars(curve, arr.handle, FIRST, n) == _enc(vals[FIRST:FIRST + n])
        arr.free()
    # the specials of the Montgomery form: 0, 1, q - 1, 2^256 mod q
    vals = [0, 1, q - 1, R256 % q, q - 2]
    arr = par.scalarsFromBytes(_enc(vals), len(vals))
    assert par.scalarsToBytes(arr, montgomery=True) == _enc([v * R256 % q for v in vals])
    arr.free()


# ---------------------------------------------------------------------------------------------- 2. round trips
def _some_points(curve, label, n, seed, torch):
    """a resident set of n points with rows at infinity on the Weierstrass curves (imported with is_inf), and its
    download"""
    gen = curve.Parallel.randomPointsFast(n, seed)
    xy, _ = _download_points(curve, gen.handle, 0, n)
    gen.free()
    flags = bytes(1 if (i % 7 == 3 or i == n - 1) and label in WEIER else 0 for i in range(n))
    arr = curve.Parallel.pointsFromBytes(xy, n, is_inf=flags)
    return arr, _download_points(curve, arr.handle, 0, n)


@pytest.mark.parametrize("label", ALL)
def test_round_trips(curves, torch, label):
    """scalarsFromTensor(scalarsToTensor(x, form), form) downloads as x for every form; the same for points: canonical,
    Montgomery, compressed with both signs, with is_inf"""
    curve = curves(label)
    par = curve.Parallel
    q = P.CURVES[label]["order"]
    n = 257
    for width, mont in ((4, False), (8, False), (16, False), (32, False), (32, True)):
        vals = _scalars(min(q, 1 << (8 * width)), n + FIRST, width + (100 if mont else 0))
        x = par.scalarsFromBytes(_enc(vals), len(vals))
        for device in ("cuda", "cpu"):
            t = par.scalarsToTensor(x, first=FIRST, width=width, montgomery=mont)
            t = t if device == "cuda" else t.cpu()
            y = par.scalarsFromTensor(t, montgomery=mont)
            assert curve.Scalar.toBigints(y) == vals[FIRST:], (width, mont, device)
            y.free()
        x.free()
    pts, (xy, inf) = _some_points(curve, label, n, 41, torch)
    assert (sum(inf) > 0) == (label in WEIER)
    for kw in ({}, {"montgomery": True}, {"compressed": True}, {"compressed": True, "sign": "parity"}):
        for device in ("cuda", "cpu"):
            if device == "cuda":
                t, fl = par.pointsToTensor(pts, is_inf=True, **kw)
            else:
                rec = curve.fe_bytes * (1 if kw.get("compressed") else 2)
                t = torch.zeros((n, rec), dtype=torch.uint8)
                t, fl = par.pointsToTensor(pts, t, is_inf=torch.full((n,), 7, dtype=torch.uint8), **kw)
            assert _bytes(fl) == inf
            back = par.pointsFromTensor(t, is_inf=fl, **kw)
            assert _download_points(curve, back.handle, 0, n) == (xy, inf), (kw, device)
            back.free()
    pts.free()


# ---------------------------------------------------------------------------------------------- 3. overflow and range
@pytest.mark.parametrize("label", ["pallas", "bls12-377"])
def test_overflow_and_range(curves, torch, mod, label):
    """an entry equal to 2^(8 width) at the first, a middle and the last index of the range is MSMZ_ERR_RANGE, outside the
    range it is not read; an entry >= q is MSMZ_ERR_RANGE in every form; a good call afterwards is correct"""
    curve = curves(label)
    par = curve.Parallel
    q = P.CURVES[label]["order"]
    n, total = 257, 257 + FIRST + 3

    def refused(arr, width, mont=False):
        for device in ("cpu", "cuda"):
            whole, out = _dest(torch, n, width, device, True)
            with pytest.raises(mod._native.MsmzError) as e:
                par.scalarsToTensor(arr, out, first=FIRST, montgomery=mont)
            assert e.value.status == MSMZ_ERR_RANGE, (width, mont, device)
            # nothing outside the addressed records is written
            assert _holds(whole, n, width, True, _bytes(out)), (width, mont, device)
        with pytest.raises(mod._native.MsmzError) as e:
            par.scalarsToBytes(arr, FIRST, n, width=width, montgomery=mont)
        assert e.value.status == MSMZ_ERR_RANGE

    def fine(arr, vals, width, mont=False):
        want = _enc([v * R256 % q for v in vals[FIRST:FIRST + n]]) if mont else _enc(vals[FIRST:FIRST + n], width)
        for device in ("cpu", "cuda"):
            whole, out = _dest(torch, n, width, device, True)
            par.scalarsToTensor(arr, out, first=FIRST, montgomery=mont)
            assert _holds(whole, n, width, True, want), (width, mont, device)

    for width in (4, 8, 16):
        good = _scalars(1 << (8 * width), total, 7 * width)   # (2^(8 width) - 1 is among them, at FIRST)
        for at in (FIRST, FIRST + 129, FIRST + n - 1):
            bad = list(good)
            bad[at] = 1 << (8 * width)
            arr = par.scalarsFromBytes(_enc(bad), total)
            refused(arr, width)
            fine(arr, bad, 32)
            arr.free()
        out_of_range = list(good)
        out_of_range[FIRST - 1] = out_of_range[FIRST + n] = 1 << (8 * width)
        arr = par.scalarsFromBytes(_enc(out_of_range), total)
        fine(arr, out_of_range, width)
        arr.free()
    good = _scalars(1 << 32, total, 99)
    for at, value in ((FIRST, q), (FIRST + 129, R256 - 1), (FIRST + n - 1, q + 5)):
        arr = par.scalarsFromBytes(_enc(good), total)
        _plant(curve, arr, at, value)
        for width in (4, 8, 16, 32):
            refused(arr, width)
        refused(arr, 32, True)
        arr.free()
        arr = par.scalarsFromBytes(_enc(good), total)
        for index in (FIRST - 1, FIRST + n):   # outside the range: not read
            _plant(curve, arr, index, value)
        for width in (4, 8, 16, 32):
            fine(arr, good, width)
        fine(arr, good, 32, True)
        arr.free()


# ---------------------------------------------------------------------------------------------- 4. point forms
def _mont_xy(params, xy, inf):
    """the download's bytes -> what the Montgomery form holds: v * 2^(8 fe_bytes) mod p, infinity rows all zero"""
    p, fb = params["modulus"], params["fe_bytes"]
    out = bytearray()
    for i in range(len(inf)):
        for k in (0, 1):
            v = int.from_bytes(xy[(2 * i + k) * fb:(2 * i + k + 1) * fb], "little")
            out += (0 if inf[i] else (v << (8 * fb)) % p).to_bytes(fb, "little")
    return bytes(out)


@pytest.mark.parametrize("label", ALL)
def test_point_forms(curves, torch, label):
    """canonical, Montgomery and compressed (both signs) records against Affine.toBigints, Affine.toCompressedBytes and
    the two downloads, for every size, host and device, packed and strided, with and without is_inf; rows at infinity
    imported with is_inf and made by mulPoints with scalar 0 (the identity (0, 1) on the twisted Edwards curve); the
    endomorphism images of a Weierstrass set and a range of a precomputed handle"""
    from msm_zprize_amd._native import MSMZ_SRC_COMPRESSED, MSMZ_SRC_DEVICE, MSMZ_SRC_MONTGOMERY, MSMZ_SRC_SIGN_PARITY
    curve = curves(label)
    par = curve.Parallel
    params = P.CURVES[label]
    fb, p = params["fe_bytes"], params["modulus"]
    weier = label in WEIER
    pts, (xy, inf) = _some_points(curve, label, TOTAL, 17, torch)
    big = curve.Affine.toBigints(pts)
    assert _canon(params, big) == xy and bytes(1 if b["isZero"] else 0 for b in big) == inf
    forms = {"canon": ({}, 2 * fb, xy), "mont": ({"montgomery": True}, 2 * fb, _mont_xy(params, xy, inf))}
    for sign in ("largest", "parity"):
        comp, cinf = curve.Affine.toCompressedBytes(pts, sign=sign)
        assert (comp, cinf) == _download_compressed(curve, pts.handle, 0, TOTAL, MSMZ_SRC_SIGN_PARITY if sign == "parity" else 0)
        assert cinf == inf
        forms[sign] = ({"compressed": True, "sign": sign}, fb, comp)
    for name, (kw, rec, full) in forms.items():
        for n in SIZES:
            want, winf = full[FIRST * rec:(FIRST + n) * rec], inf[FIRST:FIRST + n]
            for device in ("cpu", "cuda"):
                for strided in (False, True):
                    whole, out = _dest(torch, n, rec, device, strided)
                    assert par.pointsToTensor(pts, out, first=FIRST, **kw) is out
                    assert _holds(whole, n, rec, strided, want), (name, n, device, strided)
                    whole, out = _dest(torch, n, rec, device, strided)
                    flags = torch.full((n + 2,), 0xA5, dtype=torch.uint8, device=device)
                    par.pointsToTensor(pts, out, first=FIRST, is_inf=flags[1:n + 1], **kw)
                    assert _holds(whole, n, rec, strided, want), (name, n, device, strided)
                    assert _bytes(flags) == b"\xa5" + winf + b"\xa5", (name, n, device, strided)
        if not kw.get("compressed"):
            data, flags = par.pointsToBytes(pts, FIRST, 257, **kw)
            assert (data, flags) == (full[FIRST * rec:(FIRST + 257) * rec], inf[FIRST:FIRST + 257])
    # flags 0, stride 0, host: the download, byte for byte, is_inf included
    buf, fl = C.create_string_buffer(2 * fb * TOTAL), C.create_string_buffer(TOTAL)
    d = _dst(C.addressof(buf), 0, 0, 0, None, C.addressof(fl))
    assert _L().msmz_export_points(curve._ctx, pts.handle, 0, TOTAL, C.byref(d)) == 0
    assert (buf.raw, fl.raw) == (xy, inf)
    # every row at infinity: [0] P
    zero = par.mulPoints(0, pts, 65)
    zxy, zinf = _download_points(curve, zero.handle, 0, 65)
    ident = bytes(2 * fb) if weier else (bytes(fb) + (1).to_bytes(fb, "little"))
    assert zxy == ident * 65 and zinf == (b"\1" if weier else b"\0") * 65
    for kw, want in (({}, zxy), ({"montgomery": True}, _mont_xy(params, zxy, zinf)),
                     ({"compressed": True}, curve.Affine.toCompressedBytes(zero)[0]),
                     ({"compressed": True, "sign": "parity"}, curve.Affine.toCompressedBytes(zero, sign="parity")[0])):
        t, flags = par.pointsToTensor(zero, is_inf=True, **kw)
        assert _bytes(t) == want and _bytes(flags) == zinf, kw
        if weier:
            assert want == bytes(len(want))   # the all-zero record in every form
    if not weier:   # the identity in the requested form: (0, 2^256 mod p) as Montgomery residues
        assert _mont_xy(params, zxy, zinf) == (bytes(fb) + ((1 << (8 * fb)) % p).to_bytes(fb, "little")) * 65
    zero.free()
    # ranges the downloads keep readable: the endomorphism images [n, 2n) of a Weierstrass set, the copies of a
    # precomputed handle -- each equal to the download, into host and device memory
    ranges = []
    pre = None
    if weier:
        ranges.append((pts.handle, TOTAL - 5, 70))
        pre = par.precomputePoints(pts, 300, {}, 0)
        assert pre.info["records"] >= 600
        ranges.append((pre.handle, 295, 200))
    for handle, first, n in ranges:
        dxy, dinf = _download_points(curve, handle, first, n)
        for flag in (0, MSMZ_SRC_MONTGOMERY, MSMZ_SRC_COMPRESSED, MSMZ_SRC_COMPRESSED | MSMZ_SRC_SIGN_PARITY):
            rec = fb if flag & MSMZ_SRC_COMPRESSED else 2 * fb
            want = (_download_compressed(curve, handle, first, n, flag & MSMZ_SRC_SIGN_PARITY)[0] if flag & MSMZ_SRC_COMPRESSED
                    else _mont_xy(params, dxy, dinf) if flag else dxy)
            buf, fl = C.create_string_buffer(rec * n), C.create_string_buffer(n)
            d = _dst(C.addressof(buf), 0, rec, flag, None, C.addressof(fl))
            assert _L().msmz_export_points(curve._ctx, handle, first, n, C.byref(d)) == 0
            assert (buf.raw, fl.raw) == (want, dinf), (first, n, flag)
            t = torch.full((n, rec), 0xA5, dtype=torch.uint8, device="cuda")
            tf = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            d = _dst(t.data_ptr(), 0, rec, flag | MSMZ_SRC_DEVICE, None, tf.data_ptr())
            assert _L().msmz_export_points(curve._ctx, handle, first, n, C.byref(d)) == 0
            assert (_bytes(t), _bytes(tf)) == (want, dinf), (first, n, flag)
        # one record past the end
        have = 2 * TOTAL if handle == pts.handle else None
        if have:
            d = _dst(C.addressof(buf), 0, 0)
            assert _L().msmz_export_points(curve._ctx, handle, have - 1, 2, C.byref(d)) == MSMZ_ERR_ARG
            assert _L().msmz_export_points(curve._ctx, handle, have - 1, 1, C.byref(d)) == 0
    if pre is not None:
        pre.free()
    pts.free()


def _canon(params, big):
    fb = params["fe_bytes"]
    return b"".join(b["x"].to_bytes(fb, "little") + b["y"].to_bytes(fb, "little") for b in big)


# ---------------------------------------------------------------------------------------------- 5. usable where it lies
@pytest.mark.parametrize("label", ALL)
def test_result_is_usable_where_it_lies(curves, torch, label):
    """a torch reduction over the exported GPU tensor equals the same reduction over the downloaded bytes; an MSM over
    re-imported scalars and points (n = 257) equals the C oracle"""
    curve = curves(label)
    par = curve.Parallel
    params = P.CURVES[label]
    n = 257
    sc = par.randomScalars(n + FIRST, 5)
    pts = par.randomPointsFast(n + FIRST, 6)
    t = par.scalarsToTensor(sc, first=FIRST)
    raw = _download_scalars(curve, sc.handle, FIRST, n)
    assert int(t.to(torch.int64).sum().item()) == sum(raw)
    words = torch.frombuffer(bytearray(raw), dtype=torch.int32).reshape(n, 8).to(torch.int64)
    assert torch.equal(t.view(torch.int32).to(torch.int64).sum(dim=0).cpu(), words.sum(dim=0))
    tp = par.pointsToTensor(pts, first=FIRST)
    assert int(tp.to(torch.int64).sum().item()) == sum(_download_points(curve, pts.handle, FIRST, n)[0])
    scalars = curve.Scalar.toBigints(sc, FIRST, n)
    points = [_strip(b) for b in curve.Affine.toBigints(pts, FIRST, n)]
    want = _strip(c_oracle.msm(params, scalars, points))
    for skw, pkw in (({}, {}), ({"montgomery": True}, {"montgomery": True}), ({}, {"compressed": True}),
                     ({"montgomery": True}, {"compressed": True, "sign": "parity"})):
        s2 = par.scalarsFromTensor(par.scalarsToTensor(sc, first=FIRST, **skw), **skw)
        tp, fl = par.pointsToTensor(pts, first=FIRST, is_inf=True, **pkw)
        p2 = par.pointsFromTensor(tp, is_inf=fl, **pkw)
        assert _strip(par.msm(s2, p2, n)["result"]) == want, (skw, pkw)
        s2.free()
        p2.free()
    sc.free()
    pts.free()


# ---------------------------------------------------------------------------------------------- 6. argument errors
def test_argument_errors(curves, torch):
    """every MSMZ_ERR_ARG case of the header, on a host and on a device destination: refused before any launch, the
    destination (0xA5) unchanged; the Python layer refuses a tensor that is too small"""
    from msm_zprize_amd._native import (MSMZ_SRC_COMPRESSED, MSMZ_SRC_DEFAULT_STREAM, MSMZ_SRC_DEVICE, MSMZ_SRC_MONTGOMERY,
                                        MSMZ_SRC_SIGN_PARITY)
    curve = curves("pallas")   # fe_bytes 32: a point record is 64 bytes, a compressed one 32
    L = _L()
    n = 64
    sc = curve.Parallel.scalarsFromBytes(_enc(_scalars(1 << 32, n, 3)), n)
    pts = curve.Parallel.randomPointsFast(n, 1)
    dev = torch.full((n + 1, 80), 0xA5, dtype=torch.uint8, device="cuda")
    dev_inf = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    host = C.create_string_buffer(b"\xa5" * (80 * (n + 1)), 80 * (n + 1))
    host_inf = C.create_string_buffer(b"\xa5" * n, n)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ES, EP = L.msmz_export_scalars, L.msmz_export_points
    for ptr, inf_ptr, flag in ((dev.data_ptr(), dev_inf.data_ptr(), MSMZ_SRC_DEVICE),
                               (C.addressof(host), C.addressof(host_inf), 0)):
        def d(**k):
            return _dst(k.get("ptr", ptr), k.get("stride", 0), k.get("width", 32), k.get("flags", flag),
                        k.get("stream"), k.get("is_inf"))
        bad_scalars = [d(width=0), d(width=36), d(width=6), d(width=2), d(stride=16), d(stride=34), d(stride=1 << 24),
                       d(ptr=ptr + 2), d(ptr=None), d(flags=flag | 64), d(flags=flag | 32),
                       d(width=8, flags=flag | MSMZ_SRC_MONTGOMERY), d(flags=flag | MSMZ_SRC_COMPRESSED),
                       d(flags=flag | MSMZ_SRC_SIGN_PARITY), d(flags=flag | MSMZ_SRC_COMPRESSED | MSMZ_SRC_SIGN_PARITY),
                       d(is_inf=inf_ptr), d(stream=side.cuda_stream, flags=flag | MSMZ_SRC_DEFAULT_STREAM)]
        if not flag:   # a stream, or the null stream, without MSMZ_SRC_DEVICE
            bad_scalars += [d(stream=side.cuda_stream), d(flags=MSMZ_SRC_DEFAULT_STREAM)]
        for b in bad_scalars:
            assert ES(curve._ctx, sc.handle, 0, n, C.byref(b)) == MSMZ_ERR_ARG
        ok = d()
        for handle, first, cnt in ((sc.handle, 0, 0), (sc.handle, 1, n), (sc.handle, n, 1), (sc.handle, n + 1, 0),
                                   (sc.handle, 2 ** 64 - 1, 2), (sc.handle, 0, n + 1), (pts.handle, 0, 1), (12345, 0, 1)):
            assert ES(curve._ctx, handle, first, cnt, C.byref(ok)) == MSMZ_ERR_ARG, (handle, first, cnt)
        assert ES(curve._ctx, sc.handle, 0, n, None) == MSMZ_ERR_ARG
        assert ES(None, sc.handle, 0, n, C.byref(ok)) == MSMZ_ERR_ARG
        # points: the width is 0 or 64 (compressed: 0 or 32)
        bad_points = [d(width=32), d(width=96), d(width=64, stride=32), d(width=64, stride=66), d(width=64, stride=1 << 24),
                      d(width=64, ptr=ptr + 2), d(width=64, ptr=None), d(width=64, flags=flag | 32),
                      d(width=64, flags=flag | MSMZ_SRC_SIGN_PARITY),
                      d(width=32, flags=flag | MSMZ_SRC_COMPRESSED | MSMZ_SRC_MONTGOMERY),
                      d(width=64, flags=flag | MSMZ_SRC_COMPRESSED), d(width=32, flags=flag | MSMZ_SRC_MONTGOMERY),
                      d(width=64, stream=side.cuda_stream, flags=flag | MSMZ_SRC_DEFAULT_STREAM)]
        if not flag:
            bad_points += [d(width=64, stream=side.cuda_stream), d(width=64, flags=MSMZ_SRC_DEFAULT_STREAM)]
        for b in bad_points:
            assert EP(curve._ctx, pts.handle, 0, n, C.byref(b)) == MSMZ_ERR_ARG
        okp = d(width=0, is_inf=inf_ptr)
        for handle, first, cnt in ((pts.handle, 0, 0), (pts.handle, 2 * n, 1), (pts.handle, 2 * n - 1, 2),
                                   (pts.handle, 2 ** 64 - 1, 2), (pts.handle, 0, 2 * n + 1), (sc.handle, 0, 1), (12345, 0, 1)):
            assert EP(curve._ctx, handle, first, cnt, C.byref(okp)) == MSMZ_ERR_ARG, (handle, first, cnt)
        assert EP(curve._ctx, pts.handle, 0, n, None) == MSMZ_ERR_ARG
        assert EP(None, pts.handle, 0, n, C.byref(okp)) == MSMZ_ERR_ARG
    # nothing was written
    assert _bytes(dev) == b"\xa5" * (80 * (n + 1)) and _bytes(dev_inf) == b"\xa5" * n
    assert host.raw == b"\xa5" * (80 * (n + 1)) and host_inf.raw == b"\xa5" * n
    # the Python layer: a tensor that is too small, on either side; the wrong kind of array
    for device in ("cpu", "cuda"):
        with pytest.raises(ValueError, match="into a tensor of 10 rows"):
            curve.Parallel.scalarsToTensor(sc, torch.zeros((10, 32), dtype=torch.uint8, device=device), N=11)
        with pytest.raises(ValueError, match="of an array of 64"):
            curve.Parallel.scalarsToTensor(sc, torch.zeros((65, 32), dtype=torch.uint8, device=device))
        with pytest.raises(ValueError, match="a point is 64"):
            curve.Parallel.pointsToTensor(pts, torch.zeros((n, 32), dtype=torch.uint8, device=device))
        with pytest.raises(ValueError, match="is_inf"):
            curve.Parallel.pointsToTensor(pts, torch.zeros((n, 64), dtype=torch.uint8, device=device),
                                          is_inf=torch.zeros((n - 1,), dtype=torch.uint8, device=device))
    with pytest.raises(TypeError):
        curve.Parallel.scalarsToTensor(pts)
    # the context is as usable as before, and good calls are correct
    assert ES(curve._ctx, sc.handle, 0, n, C.byref(_dst(C.addressof(host), 80, 32))) == 0
    assert host.raw[:32] == _download_scalars(curve, sc.handle, 0, 1) and host.raw[32:80] == b"\xa5" * 48
    sc.free()
    pts.free()


# ---------------------------------------------------------------------------------------------- 7. pinned host memory
def test_pinned_host_memory_as_a_device_destination(curves, torch):
    """MSMZ_SRC_DEVICE over pinned host memory: the runtime knows it, the kernel writes it in place"""
    from msm_zprize_amd._native import MSMZ_SRC_DEVICE, MSMZ_SRC_MONTGOMERY
    curve = curves("pallas")
    q = P.CURVES["pallas"]["order"]
    n = 1000
    vals = _scalars(1 << 64, n + FIRST, 5)
    arr = curve.Parallel.scalarsFromBytes(_enc(vals), len(vals))
    whole = torch.full((n + 2, 32), 0xA5, dtype=torch.uint8).pin_memory()
    assert whole.is_pinned()
    for width, stride, flags, want in ((8, 32, 0, _enc(vals[FIRST:], 8)), (32, 0, MSMZ_SRC_MONTGOMERY, _enc([v * R256 % q for v in vals[FIRST:]]))):
        whole.fill_(0xA5)
        d = _dst(whole[1:].data_ptr(), stride, width, flags | MSMZ_SRC_DEVICE)
        assert _L().msmz_export_scalars(curve._ctx, arr.handle, FIRST, n, C.byref(d)) == 0
        exp = bytearray(b"\xa5" * (32 * (n + 2)))
        for i in range(n):
            exp[32 * (i + 1):32 * (i + 1) + width] = want[i * width:(i + 1) * width]
        assert _bytes(whole) == bytes(exp), width
    # through the Python layer a pinned tensor is a CPU tensor: the host route, the same bytes
    out = whole[1:n + 1]
    whole.fill_(0xA5)
    curve.Parallel.scalarsToTensor(arr, out, first=FIRST, montgomery=True)
    assert _bytes(out) == _enc([v * R256 % q for v in vals[FIRST:]])
    pts = curve.Parallel.randomPointsFast(n, 9)
    pw = torch.full((n + 2, 64), 0xA5, dtype=torch.uint8).pin_memory()
    pf = torch.full((n + 2,), 0xA5, dtype=torch.uint8).pin_memory()
    d = _dst(pw[1:].data_ptr(), 0, 0, MSMZ_SRC_DEVICE, None, pf[1:].data_ptr())
    assert _L().msmz_export_points(curve._ctx, pts.handle, 0, n, C.byref(d)) == 0
    xy, inf = _download_points(curve, pts.handle, 0, n)
    assert _bytes(pw) == b"\xa5" * 64 + xy + b"\xa5" * 64 and _bytes(pf) == b"\xa5" + inf + b"\xa5"
    arr.free()
    pts.free()


# ---------------------------------------------------------------------------------------------- 8. ordering
def test_export_behind_a_torch_stream(curves, torch):
    """The destination is overwritten on a non-default torch stream -- long fills, then a fill of the destination itself --
    and exported into with that stream in the descriptor, with no torch.cuda.synchronize() in between; afterwards it
    holds the export.  This exercises the event path (record on the stream that last touches the destination, wait on
    the engine's).  It cannot PROVE the ordering: a missing wait would only show if the fills happen to be still
    running when the export kernel starts."""
    curve = curves("bls12-377")
    n = 1 << 16
    sc = curve.Parallel.randomScalars(n, 21)
    want = _download_scalars(curve, sc.handle, 0, n)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != 0
        big = torch.empty(1 << 26, dtype=torch.int64, device="cuda")   # 512 MiB per fill
        t = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        for k in range(24):
            big.fill_(k)
        t.fill_(0xA5)
        out = curve.Parallel.scalarsToTensor(sc, t)
    assert out is t
    # the export has returned: the GPU has written everything, any stream may read it
    assert _bytes(t) == want
    torch.cuda.synchronize()
    sc.free()


# ---------------------------------------------------------------------------------------------- 9. several engines, one GPU
def test_two_engines_on_one_gpu(mod, curves, torch):
    """devices = [0, 0], n = 2^16 + 257: host exports of scalars and points, in every form, equal the single-engine bytes;
    a device destination is MSMZ_ERR_UNSUPPORTED"""
    from msm_zprize_amd._native import MSMZ_SRC_DEVICE
    params = P.BLS12_377
    q, fb = params["order"], params["fe_bytes"]
    n = (1 << 16) + 257
    first = (1 << 16) - 100   # the range crosses the boundary between the two engines' blocks
    cnt = n - first
    single = curves("bls12-377")
    nvals = _scalars(1 << 64, n, 77)
    narrow = _enc(nvals)
    want = {}
    for name, ctx in (("single", single), ("multi", None)):
        if ctx is None:
            mod.startThreads(devices=[0, 0])
            ctx = mod.Weierstrass.create(mod.curves.bls12377Params)
        par = ctx.Parallel
        try:
            sc, s8, pts = par.randomScalars(n, 3), par.scalarsFromBytes(narrow, n), par.randomPointsFast(n, 4)
            got = {"s32": par.scalarsToBytes(sc), "smont": par.scalarsToBytes(sc, montgomery=True),
                   "s8": par.scalarsToBytes(s8, width=8), "s8range": par.scalarsToBytes(s8, first, cnt, width=16),
                   "p": par.pointsToBytes(pts), "pmont": par.pointsToBytes(pts, first, cnt, montgomery=True)}
            for key, kw in (("ccanon", {}), ("cmont", {"montgomery": True}), ("clargest", {"compressed": True}),
                            ("cparity", {"compressed": True, "sign": "parity"})):
                rec = fb * (1 if kw.get("compressed") else 2)
                whole, out = _dest(torch, cnt, rec, "cpu", True)
                flags = torch.full((cnt,), 0xA5, dtype=torch.uint8)
                par.pointsToTensor(pts, out, first=first, is_inf=flags, **kw)
                assert _holds(whole, cnt, rec, True, _bytes(out))
                got[key] = (_bytes(out), _bytes(flags))
            whole, out = _dest(torch, cnt, 8, "cpu", True)
            par.scalarsToTensor(s8, out, first=first)
            assert _holds(whole, cnt, 8, True, _enc(nvals[first:], 8))
            if name == "multi":
                assert got == want
                assert got["s32"] == _download_scalars(ctx, sc.handle, 0, n)
                t = torch.full((cnt, 32), 0xA5, dtype=torch.uint8, device="cuda")
                d = _dst(t.data_ptr(), 0, 32, MSMZ_SRC_DEVICE)
                assert _L().msmz_export_scalars(ctx._ctx, sc.handle, first, cnt, C.byref(d)) == MSMZ_ERR_UNSUPPORTED
                d = _dst(t.data_ptr(), 0, 0, MSMZ_SRC_DEVICE)
                assert _L().msmz_export_points(ctx._ctx, pts.handle, 0, 10, C.byref(d)) == MSMZ_ERR_UNSUPPORTED
                assert _bytes(t) == b"\xa5" * (32 * cnt)
                with pytest.raises(mod._native.MsmzError) as e:
                    par.scalarsToTensor(sc, t, first=first)
                assert e.value.status == MSMZ_ERR_UNSUPPORTED
                with pytest.raises(ValueError, match="host memory only"):
                    par.scalarsToTensor(sc)
            else:
                want = got
            for a in (sc, s8, pts):
                a.free()
        finally:
            if name == "multi":
                ctx.close()
                mod.startThreads()

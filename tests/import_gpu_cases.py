"""Imports on the GPU (msmz_import_scalars / _into / msmz_import_points; scalarsFromTensor, pointsFromTensor, scalarsInto):
the conversion in isolation (download(import(x)) against Python integers), whole MSMs over imported handles bit-exact
against the C oracle and against the same call over uploaded handles, the error paths, a three-engine context on one GPU,
and an import ordered behind a non-default torch stream.  Device memory comes from torch tensors.

These cases run in a child process of their own (tests/test_scalar_import_gpu.py starts it): torch carries its own copy
of the HIP runtime, and a process may hold only one -- whichever is loaded first serves both, so torch is imported
here before anything loads libmsmz.so.  In a process that already runs the library on the system's runtime (the rest of
the suite) torch would find no GPU.

Not tested on purpose: a pageable host pointer passed WITH MSMZ_SRC_DEVICE.  The engine's pointer classification must
refuse it; if it were wrong the kernel would fault the GPU, and no test here may be able to do that."""
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


def _strip(p):
    return {"x": p["x"], "y": p["y"], "isZero": bool(p.get("isZero", False))}


def _enc(vals, width=32):
    return b"".join(int(v).to_bytes(width, "little") for v in vals)


def _tensor(torch, data, n, width, device, strided=False):
    """n records of `width` bytes as a (n, width) uint8 tensor; strided: a column view of a wider matrix (rows
    width + 24 bytes apart, the records 8 bytes into them)"""
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8)[:n * width].reshape(n, width)
    if strided:
        wide = torch.full((n, width + 24), 0xA5, dtype=torch.uint8)
        wide[:, 8:8 + width] = t
        wide = wide.to(device)
        return wide[:, 8:8 + width]
    return t.to(device)


def _scalars(q, bits, n, seed):
    top = min(q, 1 << bits)
    rng = random.Random(seed)
    s = [rng.randrange(top) for _ in range(n)]
    for i, v in zip((0, 1, 2, n - 1), (top - 1, 0, 1, top - 1)):
        if 0 <= i < n:
            s[i] = v
    return s


def _mont_points(params, pts):
    p, fb = params["modulus"], params["fe_bytes"]
    r = 1 << (8 * fb)
    return b"".join((pt["x"] * r % p).to_bytes(fb, "little") + (pt["y"] * r % p).to_bytes(fb, "little") for pt in pts)


def _canon_points(params, pts):
    fb = params["fe_bytes"]
    return b"".join(pt["x"].to_bytes(fb, "little") + pt["y"].to_bytes(fb, "little") for pt in pts)


# ---------------------------------------------------------------------------------------------- conversion in isolation
@pytest.mark.parametrize("label", ALL)
def test_scalar_conversion(curves, torch, label):
    """widths 4, 8, 16, 32 x packed / strided x host / device source: download(import(x)) == zero-extended x; the byte
    route with width; Montgomery records v * 2^256 mod q download as v; width 32 canonical host import == upload"""
    curve = curves(label)
    q = P.CURVES[label]["order"]
    n = 3000
    for width in (4, 8, 16, 32):
        vals = _scalars(q, 8 * width, n, width)
        data = _enc(vals, width)
        for device in ("cpu", "cuda"):
            for strided in (False, True):
                arr = curve.Parallel.scalarsFromTensor(_tensor(torch, data, n, width, device, strided))
                assert curve.Scalar.toBigints(arr) == vals, (width, device, strided)
                arr.free()
        arr = curve.Parallel.scalarsFromBytes(data, n, width=width)
        assert curve.Scalar.toBigints(arr) == vals, width
        arr.free()
    vals = _scalars(q, 64, n, 9)
    for device in ("cpu", "cuda"):   # 1-D tensors of an 8-byte dtype, also as a column of a wider matrix
        t = torch.frombuffer(bytearray(_enc(vals, 8)), dtype=torch.int64).to(device)
        arr = curve.Parallel.scalarsFromTensor(t)
        assert curve.Scalar.toBigints(arr) == vals
        arr.free()
        m = torch.zeros((n, 3), dtype=torch.int64, device=device)
        m[:, 1] = t
        arr = curve.Parallel.scalarsFromTensor(m[:, 1])
        assert curve.Scalar.toBigints(arr) == vals
        arr.free()
    vals = [0, 1, q - 1, q - 2, R256 % q] + _scalars(q, 256, n - 5, 11)
    mont = _enc([v * R256 % q for v in vals])
    for device in ("cpu", "cuda"):
        for strided in (False, True):
            arr = curve.Parallel.scalarsFromTensor(_tensor(torch, mont, n, 32, device, strided), montgomery=True)
            assert curve.Scalar.toBigints(arr) == vals, (device, strided)
            arr.free()
    arr = curve.Parallel.scalarsFromBytes(mont, n, montgomery=True)
    assert curve.Scalar.toBigints(arr) == vals
    arr.free()
    # width 32, canonical, host, packed: what msmz_upload_scalars leaves, byte for byte
    from msm_zprize_amd._native import MsmzSrc, lib
    data = _enc(vals)
    up = curve.Parallel.scalarsFromBytes(data, n)
    h = C.c_uint64()
    src = MsmzSrc(C.cast(C.c_char_p(data), C.c_void_p), 0, 32, 0, None, None)
    assert lib().msmz_import_scalars(curve._ctx, C.byref(src), n, C.byref(h)) == 0
    a, b = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n)
    assert lib().msmz_download_scalars(curve._ctx, up.handle, 0, n, a) == 0
    assert lib().msmz_download_scalars(curve._ctx, h.value, 0, n, b) == 0
    assert a.raw == b.raw == data
    assert lib().msmz_free(curve._ctx, h.value) == 0
    up.free()


@pytest.mark.parametrize("label", ALL)
def test_point_conversion(curves, torch, label):
    """download_points(import(points)) == the canonical points: Montgomery and canonical form, host and device source,
    packed and strided, with and without infinity flags"""
    curve = curves(label)
    params = P.CURVES[label]
    weier = label in WEIER
    n = 700
    gen = curve.Parallel.randomPointsFast(n, 31)
    pts = [_strip(p) for p in curve.Affine.toBigints(gen)]
    gen.free()
    fb = params["fe_bytes"]
    flags = bytes(1 if i % 7 == 3 else 0 for i in range(n))
    zero = {"x": 0, "y": 0, "isZero": True}
    for mont, data in ((True, _mont_points(params, pts)), (False, _canon_points(params, pts))):
        for device in ("cpu", "cuda"):
            for strided in (False, True):
                t = _tensor(torch, data, n, 2 * fb, device, strided)
                arr = curve.Parallel.pointsFromTensor(t, montgomery=mont)
                assert [_strip(p) for p in curve.Affine.toBigints(arr)] == pts, (mont, device, strided)
                arr.free()
                if weier:
                    fl = torch.frombuffer(bytearray(flags), dtype=torch.uint8).to(device)
                    arr = curve.Parallel.pointsFromTensor(t, montgomery=mont, is_inf=fl)
                    want = [zero if f else p for f, p in zip(flags, pts)]
                    assert [_strip(p) for p in curve.Affine.toBigints(arr)] == want, (mont, device, strided)
                    arr.free()
        if mont:
            arr = curve.Parallel.pointsFromBytes(data, n, montgomery=True)
            assert [_strip(p) for p in curve.Affine.toBigints(arr)] == pts
            arr.free()


def test_pinned_host_memory_as_a_device_source(curves, torch):
    """MSMZ_SRC_DEVICE over pinned host memory: the runtime knows it, the kernel reads it in place"""
    from msm_zprize_amd._native import MSMZ_SRC_DEVICE, MsmzSrc, lib
    curve = curves("pallas")
    q = P.CURVES["pallas"]["order"]
    n = 5000
    vals = _scalars(q, 64, n, 5)
    t = torch.frombuffer(bytearray(_enc(vals, 8)), dtype=torch.int64).pin_memory()
    assert t.is_pinned()
    h = C.c_uint64()
    src = MsmzSrc(t.data_ptr(), 0, 8, MSMZ_SRC_DEVICE, None, None)
    assert lib().msmz_import_scalars(curve._ctx, C.byref(src), n, C.byref(h)) == 0
    buf = C.create_string_buffer(32 * n)
    assert lib().msmz_download_scalars(curve._ctx, h.value, 0, n, buf) == 0
    assert buf.raw == _enc(vals)
    assert lib().msmz_free(curve._ctx, h.value) == 0
    # a range that runs past the end of the allocation it starts in is refused before any launch (n is far beyond
    # what the pinned buffer or any device block holds)
    far = MsmzSrc(t.data_ptr(), 1 << 20, 8, MSMZ_SRC_DEVICE, None, None)
    assert lib().msmz_import_scalars(curve._ctx, C.byref(far), 1 << 22, C.byref(h)) == MSMZ_ERR_ARG
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    far = MsmzSrc(d.data_ptr(), 1 << 23, 8, MSMZ_SRC_DEVICE, None, None)   # 2^23-byte steps: 32 TiB in all
    assert lib().msmz_import_scalars(curve._ctx, C.byref(far), 1 << 22, C.byref(h)) == MSMZ_ERR_ARG
    null = MsmzSrc(None, 0, 8, MSMZ_SRC_DEVICE, None, None)
    assert lib().msmz_import_scalars(curve._ctx, C.byref(null), n, C.byref(h)) == MSMZ_ERR_ARG


# ---------------------------------------------------------------------------------------------- whole MSMs
@pytest.mark.parametrize("n", [1, 3, 257, 4096, 1 << 16])
@pytest.mark.parametrize("label", ALL)
def test_msm_over_imported_handles(curves, torch, label, n):
    """msm and msmUnsafe, GLV off / on: 64-bit scalars imported at width 8 with scalarBits = 64, full-length Montgomery
    scalars with Montgomery points -- result == oracle == the same call over uploaded handles"""
    curve = curves(label)
    params = P.CURVES[label]
    q = params["order"]
    gen = curve.Parallel.randomPointsFast(n, 100 + n)
    pts = [_strip(p) for p in curve.Affine.toBigints(gen)]
    fb = params["fe_bytes"]
    mpts = curve.Parallel.pointsFromTensor(_tensor(torch, _mont_points(params, pts), n, 2 * fb, "cuda"), montgomery=True)
    short = _scalars(q, 64, n, n + 1)
    full = _scalars(q, 256, n, n + 2)
    want_short = _strip(c_oracle.msm(params, short, pts))
    want_full = _strip(c_oracle.msm(params, full, pts))
    s8 = curve.Parallel.scalarsFromTensor(torch.frombuffer(bytearray(_enc(short, 8)), dtype=torch.int64).cuda())
    s8h = curve.Parallel.scalarsFromBytes(_enc(short, 8), n, width=8)
    sm = curve.Parallel.scalarsFromTensor(_tensor(torch, _enc([v * R256 % q for v in full]), n, 32, "cuda"), montgomery=True)
    up_short = curve.Parallel.scalarsFromBytes(_enc(short), n)
    up_full = curve.Parallel.scalarsFromBytes(_enc(full), n)
    for fn in ("msm", "msmUnsafe"):
        for glv in ((0, 1) if label in WEIER else (0,)):
            run = lambda s, p, o: _strip(getattr(curve.Parallel, fn)(s, p, n, False, dict(o, glv=glv))["result"])
            for sc in (s8, s8h):
                assert run(sc, mpts, {"scalarBits": 64}) == want_short, (fn, glv)
                assert run(sc, gen, {}) == want_short, (fn, glv)
            assert run(up_short, gen, {"scalarBits": 64}) == want_short, (fn, glv)
            assert run(sm, mpts, {}) == want_full, (fn, glv)
            assert run(up_full, gen, {}) == want_full, (fn, glv)
            assert run(sm, gen, {}) == run(up_full, mpts, {}) == want_full, (fn, glv)
    for a in (gen, mpts, s8, s8h, sm, up_short, up_full):
        a.free()


@pytest.mark.parametrize("label", WEIER)
def test_precomputed_set_from_imported_points(curves, torch, label):
    curve = curves(label)
    params = P.CURVES[label]
    q, fb, n = params["order"], params["fe_bytes"], 3000
    gen = curve.Parallel.randomPointsFast(n, 8)
    pts = [_strip(p) for p in curve.Affine.toBigints(gen)]
    mpts = curve.Parallel.pointsFromTensor(_tensor(torch, _mont_points(params, pts), n, 2 * fb, "cuda", True), montgomery=True)
    s = _scalars(q, 64, n, 3)
    want = _strip(c_oracle.msm(params, s, pts))
    sc = curve.Parallel.scalarsFromTensor(torch.frombuffer(bytearray(_enc(s, 8)), dtype=torch.int64).cuda())
    for glv in (0, 1):
        pre = curve.Parallel.precomputePoints(mpts, n, {"glv": glv, "scalarBits": 64}, 0)
        ref = curve.Parallel.precomputePoints(gen, n, {"glv": glv, "scalarBits": 64}, 0)
        assert _strip(curve.Parallel.msm(sc, pre, n)["result"]) == want
        assert _strip(curve.Parallel.msm(sc, ref, n)["result"]) == want
        assert curve.Affine.toBigints(pre) == curve.Affine.toBigints(ref)
        pre.free()
        ref.free()
    for a in (gen, mpts, sc):
        a.free()


@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_msm_batch_over_a_list_of_device_tensors(curves, torch, label):
    """B = 5 device tensors (assembled into one resident set with scalarsInto) == the same vectors as host bytes; a
    resident array may stand in the list; the assembled set is freed"""
    curve = curves(label)
    params = P.CURVES[label]
    q, n, B = params["order"], 2500, 5
    gen = curve.Parallel.randomPointsFast(n, 12)
    pts = [_strip(p) for p in curve.Affine.toBigints(gen)]
    vecs = [_scalars(q, 64, n, 50 + k) for k in range(B)]
    want = [_strip(c_oracle.msm(params, v, pts)) for v in vecs]
    host = [_enc(v) for v in vecs]
    tens = [torch.frombuffer(bytearray(_enc(v, 8)), dtype=torch.int64).cuda() for v in vecs]
    for o in ({}, {"scalarBits": 64}, {"glv": 1}):
        assert [_strip(r) for r in curve.Parallel.msmBatch(host, gen, n, o)] == want
        assert [_strip(r) for r in curve.Parallel.msmBatch(tens, gen, n, o)] == want
        assert [_strip(r) for r in curve.Parallel.msmBatchUnsafe(tens, gen, n, o)] == want
    res = curve.Parallel.scalarsFromBytes(host[2], n)
    mixed = tens[:2] + [res] + tens[3:]
    assert [_strip(r) for r in curve.Parallel.msmBatch(mixed, gen, n)] == want
    # scalarsInto by hand: vectors of different widths into one set
    from msm_zprize_amd._native import lib
    h = C.c_uint64()
    assert lib().msmz_alloc_scalars(curve._ctx, B * n, C.byref(h)) == 0
    from msm_zprize_amd.parallel import DeviceArray
    dst = DeviceArray(curve, h.value, B * n, "scalars")
    assert curve.Scalar.toBigints(dst, 0, 3) == [0, 0, 0] and curve.Scalar.toBigints(dst, B * n - 2) == [0, 0]
    assert lib().msmz_alloc_scalars(curve._ctx, 0, C.byref(h)) == MSMZ_ERR_ARG
    with pytest.raises(TypeError, match="bare tensor"):
        curve.Parallel.msmBatch(torch.stack(tens), gen, n)
    for k in range(B):
        t = tens[k] if k % 2 else _tensor(torch, host[k], n, 32, "cuda", strided=True)
        curve.Parallel.scalarsInto(dst, k * n, t)
    assert curve.Scalar.toBigints(dst) == [s for v in vecs for s in v]
    assert [_strip(r) for r in curve.Parallel.msmBatch(dst, gen, n)] == want
    with pytest.raises(ValueError):
        curve.Parallel.scalarsInto(dst, (B - 1) * n + 1, tens[0])
    with pytest.raises(TypeError):
        curve.Parallel.scalarsInto(gen, 0, tens[0])
    for a in (gen, res, dst):
        a.free()


# ---------------------------------------------------------------------------------------------- errors
def test_range_errors_leave_the_context_usable(curves, torch, mod):
    curve = curves("bls12-377")
    params = P.BLS12_377
    q, p, fb, n = params["order"], params["modulus"], params["fe_bytes"], 4000
    gen = curve.Parallel.randomPointsFast(n, 2)
    pts = [_strip(x) for x in curve.Affine.toBigints(gen)]
    good = _scalars(q, 256, n, 1)
    want = _strip(c_oracle.msm(params, good, pts))

    def still_fine():
        sc = curve.Parallel.scalarsFromTensor(_tensor(torch, _enc(good), n, 32, "cuda"))
        assert _strip(curve.Parallel.msm(sc, gen, n)["result"]) == want
        sc.free()

    for at in (0, 2049, n - 1):
        for bad_value, mont in ((q, False), (R256 - 1, False), (q, True), (q + 5, True)):
            bad = list(good)
            bad[at] = bad_value
            for device in ("cpu", "cuda"):
                with pytest.raises(mod._native.MsmzError) as e:
                    curve.Parallel.scalarsFromTensor(_tensor(torch, _enc(bad), n, 32, device), montgomery=mont)
                assert e.value.status == MSMZ_ERR_RANGE, (at, bad_value, mont, device)
        still_fine()
    for mont in (False, True):
        data = bytearray(_mont_points(params, pts) if mont else _canon_points(params, pts))
        data[2 * fb * 17 + fb:2 * fb * 18] = p.to_bytes(fb, "little")   # y of point 17 = p
        for device in ("cpu", "cuda"):
            with pytest.raises(mod._native.MsmzError) as e:
                curve.Parallel.pointsFromTensor(_tensor(torch, bytes(data), n, 2 * fb, device), montgomery=mont)
            assert e.value.status == MSMZ_ERR_RANGE, (mont, device)
        with pytest.raises(mod._native.MsmzError) as e:
            curve.Parallel.pointsFromBytes(bytes(data), n, montgomery=mont)
        assert e.value.status == MSMZ_ERR_RANGE
    still_fine()
    # a width-8 import is checked against q only; the bit bound of a later MSM is checked there, as for uploads
    s = _scalars(q, 32, n, 4)
    s[n // 2] = 1 << 40
    sc = curve.Parallel.scalarsFromTensor(torch.frombuffer(bytearray(_enc(s, 8)), dtype=torch.int64).cuda())
    with pytest.raises(mod._native.MsmzError) as e:
        curve.Parallel.msm(sc, gen, n, False, {"scalarBits": 32})
    assert e.value.status == MSMZ_ERR_RANGE
    assert _strip(curve.Parallel.msm(sc, gen, n, False, {"scalarBits": 64})["result"]) == _strip(c_oracle.msm(params, s, pts))
    sc.free()
    still_fine()
    gen.free()


def test_argument_errors(curves, torch):
    from msm_zprize_amd._native import MSMZ_SRC_DEVICE, MSMZ_SRC_MONTGOMERY, MsmzSrc, lib
    curve = curves("pallas")
    L = lib()
    n = 64
    dev = torch.zeros((n, 40), dtype=torch.uint8, device="cuda")
    host = C.create_string_buffer(40 * n)
    sc = curve.Parallel.randomScalars(n, 1)
    pts = curve.Parallel.randomPointsFast(n, 1)
    h = C.c_uint64()
    for ptr, flag in ((dev.data_ptr(), MSMZ_SRC_DEVICE), (C.cast(host, C.c_void_p).value, 0)):
        ok = lambda **k: MsmzSrc(k.get("ptr", ptr), k.get("stride", 0), k.get("width", 32), k.get("flags", flag), None, None)
        assert L.msmz_import_scalars(curve._ctx, C.byref(ok()), n, C.byref(h)) == 0
        assert L.msmz_free(curve._ctx, h.value) == 0
        bad = [ok(width=0), ok(width=36), ok(width=6), ok(width=2), ok(stride=16), ok(stride=34), ok(stride=1 << 24),
               ok(ptr=ptr + 2), ok(ptr=None), ok(flags=flag | 8), ok(flags=flag | 64), ok(width=8, flags=flag | MSMZ_SRC_MONTGOMERY)]
        for b in bad:
            assert L.msmz_import_scalars(curve._ctx, C.byref(b), n, C.byref(h)) == MSMZ_ERR_ARG
            assert L.msmz_import_scalars_into(curve._ctx, sc.handle, 0, C.byref(b), n) == MSMZ_ERR_ARG
        assert L.msmz_import_scalars(curve._ctx, C.byref(ok()), 0, C.byref(h)) == MSMZ_ERR_ARG
        assert L.msmz_import_scalars(curve._ctx, C.byref(ok()), n, None) == MSMZ_ERR_ARG
        # _into: past the end (also with a wrapping sum), on a point handle, on no handle
        assert L.msmz_import_scalars_into(curve._ctx, sc.handle, 0, C.byref(ok()), n) == 0
        assert L.msmz_import_scalars_into(curve._ctx, sc.handle, n - 1, C.byref(ok()), 1) == 0
        for first, cnt in ((1, n), (n, 1), (n + 1, 0), (2 ** 64 - 1, 2), (0, n + 1)):
            assert L.msmz_import_scalars_into(curve._ctx, sc.handle, first, C.byref(ok()), cnt) == MSMZ_ERR_ARG
        assert L.msmz_import_scalars_into(curve._ctx, pts.handle, 0, C.byref(ok()), 1) == MSMZ_ERR_ARG
        assert L.msmz_import_scalars_into(curve._ctx, 12345, 0, C.byref(ok()), 1) == MSMZ_ERR_ARG
        # points: the width is 0 or 2 * fe_bytes (64 here)
        for b in (ok(width=32), ok(width=96), ok(width=64, stride=32)):
            assert L.msmz_import_points(curve._ctx, C.byref(b), 8, C.byref(h)) == MSMZ_ERR_ARG
        assert L.msmz_import_points(curve._ctx, C.byref(ok(width=64)), 1 << 29, C.byref(h)) == MSMZ_ERR_ARG
    # a stream without MSMZ_SRC_DEVICE
    s = MsmzSrc(C.cast(host, C.c_void_p).value, 0, 32, 0, 1, None)
    assert L.msmz_import_scalars(curve._ctx, C.byref(s), n, C.byref(h)) == MSMZ_ERR_ARG
    # the context is as usable as before
    assert len(curve.Scalar.toBigints(sc)) == n
    sc.free()
    pts.free()


# ---------------------------------------------------------------------------------------------- several engines, one GPU
def test_three_engines_on_one_gpu(mod, torch):
    """devices = [0, 0, 0]: an import (device or host source) equals an upload -- same downloads, same MSM -- and
    msmz_import_scalars_into is unsupported"""
    from msm_zprize_amd._native import MSMZ_SRC_DEVICE, MsmzSrc, lib
    params = P.BLS12_377
    q, fb = params["order"], params["fe_bytes"]
    n = (1 << 17) + 4321
    mod.startThreads(devices=[0, 0, 0])
    multi = mod.Weierstrass.create(mod.curves.bls12377Params)
    try:
        gen = multi.Parallel.randomPointsFast(n, 6)
        pts = [_strip(p) for p in multi.Affine.toBigints(gen)]
        s = _scalars(q, 64, n, 7)
        want = _strip(c_oracle.msm(params, s, pts))
        up = multi.Parallel.scalarsFromBytes(_enc(s), n)
        t = torch.frombuffer(bytearray(_enc(s, 8)), dtype=torch.int64).cuda()
        mp = _mont_points(params, pts)
        for device in ("cuda", "cpu"):
            sc = multi.Parallel.scalarsFromTensor(t.to(device))
            assert multi.Scalar.toBigints(sc) == s
            mpts = multi.Parallel.pointsFromTensor(_tensor(torch, mp, n, 2 * fb, device, strided=True), montgomery=True)
            assert [_strip(p) for p in multi.Affine.toBigints(mpts, n - 100, 100)] == pts[-100:]
            for glv in (0, 1):
                o = {"glv": glv, "scalarBits": 64}
                assert _strip(multi.Parallel.msm(sc, mpts, n, False, o)["result"]) == want
                assert _strip(multi.Parallel.msm(up, gen, n, False, o)["result"]) == want
            src = MsmzSrc(t.data_ptr(), 0, 8, MSMZ_SRC_DEVICE, None, None)
            assert lib().msmz_import_scalars_into(multi._ctx, sc.handle, 0, C.byref(src), 16) == MSMZ_ERR_UNSUPPORTED
            sc.free()
            mpts.free()
        with pytest.raises(TypeError):
            multi.Parallel.msmBatch([t, t], gen, n)
        h = C.c_uint64()
        assert lib().msmz_alloc_scalars(multi._ctx, 16, C.byref(h)) == MSMZ_ERR_UNSUPPORTED
    finally:
        multi.close()
        mod.startThreads()


# ---------------------------------------------------------------------------------------------- ordering
def test_import_behind_a_torch_stream(curves, torch):
    """The tensor is produced on a non-default torch stream -- long fills, then the write of the real values -- and imported
    with that stream in the descriptor, with no torch.cuda.synchronize() in between; the MSM result is correct.  This
    exercises the event path (record on the producer's stream, wait on the engine's).  It cannot PROVE the ordering: a
    missing wait would only show if the fills happen to be still running when the import kernel starts."""
    curve = curves("bls12-377")
    params = P.BLS12_377
    q, n = params["order"], 1 << 16
    gen = curve.Parallel.randomPointsFast(n, 3)
    pts = [_strip(p) for p in curve.Affine.toBigints(gen)]
    s = _scalars(q, 64, n, 21)
    want = _strip(c_oracle.msm(params, s, pts))
    real = torch.frombuffer(bytearray(_enc(s, 8)), dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != 0
        big = torch.empty(1 << 26, dtype=torch.int64, device="cuda")   # 512 MiB per fill
        t = torch.full((n,), -1, dtype=torch.int64, device="cuda")     # (-1 = 2^64 - 1: a wrong but valid scalar)
        for k in range(24):
            big.fill_(k)
        t.copy_(real)
        sc = curve.Parallel.scalarsFromTensor(t)
        t.fill_(0)   # the import has returned: the source may be overwritten
    got = _strip(curve.Parallel.msmUnsafe(sc, gen, n, False, {"glv": 0, "scalarBits": 64})["result"])
    assert got == want
    assert curve.Scalar.toBigints(sc, 0, 64) == s[:64]
    torch.cuda.synchronize()
    sc.free()
    gen.free()

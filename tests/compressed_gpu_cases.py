"""Compressed point sets on the GPU (msmz_import_points with MSMZ_SRC_COMPRESSED, msmz_download_points_compressed;
pointsFromBytes / pointsFromTensor(compressed=True), Affine.toCompressedBytes): the round trip against Python integers
(tests/compressed_util.py), the decompressed handle as an ordinary point set, every refusal, and a two-engine context.
n = 321: a partial wave and a partial block.  Device memory comes from torch tensors, so -- like
tests/import_gpu_cases.py -- these cases run in a child process (tests/test_compressed_gpu.py starts it) that imports
torch before anything loads libmsmz.so.

No case hands the engine a pointer it would have to refuse at a kernel."""
import torch as _torch_first  # noqa: F401  (before libmsmz.so: one HIP runtime per process)

import ctypes as C
import random

import pytest

import check_points_util as U
import compressed_util as Z
from oracle import params as P

pytestmark = pytest.mark.gpu

N = 321
MSMZ_ERR_ARG, MSMZ_ERR_RANGE, MSMZ_ERR_POINT = 1, 6, 7
COMPRESSED, PARITY, MONTGOMERY = 8, 16, 2


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


@pytest.fixture(scope="module")
def sets():
    """per curve, computed once and left unchanged: the points, their flags, the x || y bytes an upload takes"""
    cache = {}

    def get(label):
        if label not in cache:
            params = P.CURVES[label]
            pts, flags = Z.round_trip_points(label, N)
            xy, inf = U.encode(params, pts)
            cache[label] = dict(pts=pts, flags=flags, xy=xy, inf=inf)
        return cache[label]

    return get


def _strip(p):
    return {"x": p["x"], "y": p["y"], "isZero": bool(p.get("isZero", False))}


def _tensor(torch, data, n, width, device, strided):
    """n records of `width` bytes as a (n, width) uint8 tensor; strided: rows width + 8 bytes apart inside a wider matrix"""
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8)[:n * width].reshape(n, width)
    if strided:
        wide = torch.full((n, width + 8), 0xA5, dtype=torch.uint8)
        wide[:, :width] = t
        return wide.to(device)[:, :width]
    return t.to(device)


def _import(curve, recs, n, flags=0, is_inf=None, width=0, stride=0):
    """msmz_import_points of a host buffer -> (status, handle)"""
    from msm_zprize_amd._native import MsmzSrc, lib
    buf = C.create_string_buffer(bytes(recs), len(recs))
    inf = None if is_inf is None else C.create_string_buffer(bytes(is_inf), len(is_inf))
    src = MsmzSrc(C.cast(buf, C.c_void_p), stride, width, flags, None, None if inf is None else C.cast(inf, C.c_void_p))
    h = C.c_uint64(0)
    st = lib().msmz_import_points(curve._ctx, C.byref(src), n, C.byref(h))
    return st, h.value


# ---------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("label", U.ALL)
def test_round_trip(curves, sets, torch, label):
    """records from Python integers -> import (host buffer, CPU tensor, GPU tensor; packed and at stride fe_bytes + 8; both
    conventions) -> msmz_download_points equals the points, msmz_download_points_compressed equals the records under
    either convention, whole and on a sub-range"""
    curve, params, s = curves(label), P.CURVES[label], sets(label)
    fb = params["fe_bytes"]
    pts, flags = s["pts"], s["flags"]
    rng = random.Random(3)
    for sign in Z.SIGNS:
        recs = Z.records(params, pts, flags, sign, rng)
        arrs = [curve.Parallel.pointsFromBytes(recs, N, is_inf=flags, compressed=True, sign=sign)]
        for device in ("cuda", "cpu"):
            for strided in (False, True):
                t = _tensor(torch, recs, N, fb, device, strided)
                f = torch.frombuffer(bytearray(flags), dtype=torch.uint8).to(device)
                arrs.append(curve.Parallel.pointsFromTensor(t, is_inf=f, compressed=True, sign=sign))
        for arr in arrs:
            assert [_strip(q) for q in curve.Affine.toBigints(arr)] == pts
        arr = arrs[1]
        for out_sign in Z.SIGNS:
            assert curve.Affine.toCompressedBytes(arr, sign=out_sign) == Z.want_compressed(params, pts, out_sign)
            got = curve.Affine.toCompressedBytes(arr, 40, 130, sign=out_sign)
            assert got == Z.want_compressed(params, pts[40:170], out_sign)
        for arr in arrs:
            arr.free()


@pytest.mark.parametrize("label", U.ALL)
def test_generated_set_survives_compression(curves, label):
    """for a randomPointsFast set S: import(download_compressed(S)) downloads equal to S"""
    curve = curves(label)
    gen = curve.Parallel.randomPointsFast(N, 21)
    want = curve.Affine.toBigints(gen)
    for sign in Z.SIGNS:
        recs, inf = curve.Affine.toCompressedBytes(gen, sign=sign)
        assert inf == bytes(N)
        back = curve.Parallel.pointsFromBytes(recs, N, compressed=True, sign=sign)
        assert curve.Affine.toBigints(back) == want
        back.free()
    gen.free()


# ---------------------------------------------------------------------------------------------- an ordinary set
@pytest.mark.parametrize("label", U.ALL)
def test_the_set_is_ordinary(curves, sets, label):
    """msm and msmBatch over the decompressed handle == the same calls over the uploaded handle (GLV on: the endomorphism
    images are right), checkPoints finds nothing off the curve, precomputePoints takes it"""
    curve, params, s = curves(label), P.CURVES[label], sets(label)
    weier = params["kind"] == "weierstrass"
    rng = random.Random(8)
    recs = Z.records(params, s["pts"], s["flags"], "largest", rng)
    dec = curve.Parallel.pointsFromBytes(recs, N, is_inf=s["flags"], compressed=True)
    up = curve.Parallel.pointsFromBytes(s["xy"], N, is_inf=s["inf"])
    q = params["order"]
    vecs = [b"".join(rng.randrange(q).to_bytes(32, "little") for _ in range(N)) for _ in range(2)]
    sc = curve.Parallel.scalarsFromBytes(vecs[0], N)
    opts = {"glv": 1} if weier else {}
    assert curve.Parallel.msm(sc, dec, N, False, opts)["result"] == curve.Parallel.msm(sc, up, N, False, opts)["result"]
    assert curve.Parallel.msmBatch(vecs, dec, N, opts) == curve.Parallel.msmBatch(vecs, up, N, opts)
    res = curve.Parallel.checkPoints(dec, subgroup=False)
    assert res.ok and res.offCurve == 0
    if weier:
        pre = curve.Parallel.precomputePoints(dec, N, {"glv": 1})
        assert curve.Parallel.msm(sc, pre, N)["result"] == curve.Parallel.msm(sc, up, N, False, opts)["result"]
        pre.free()
    checked = curve.Parallel.pointsFromBytes(recs, N, is_inf=s["flags"], compressed=True, check="curve")
    assert len(checked) == N
    for a in (dec, up, sc, checked):
        a.free()


# ---------------------------------------------------------------------------------------------- refusals
def _still_fine(curve, params):
    """no handle leaked into a usable state is observable only indirectly: the context still computes the right MSM"""
    g = U.generator(params)
    xy, _ = U.encode(params, [g, g])
    pts = curve.Parallel.pointsFromBytes(xy, 2)
    sc = curve.Parallel.scalarsFromBytes((3).to_bytes(32, "little") + (4).to_bytes(32, "little"), 2)
    got = _strip(curve.Parallel.msm(sc, pts, 2)["result"])
    assert got == _strip(U.scale(params, 7, g))
    pts.free()
    sc.free()


@pytest.mark.parametrize("label", U.ALL)
def test_refusals(curves, sets, label):
    from msm_zprize_amd._native import lib
    curve, params, s = curves(label), P.CURVES[label], sets(label)
    p, fb = params["modulus"], params["fe_bytes"]
    rng = random.Random(13)
    flagless = [q if not q["isZero"] else U.generator(params) for q in s["pts"]]   # (no flags: every record is read)
    good = bytearray(b"".join(Z.record(params, q, "largest") for q in flagless))

    def planted(rec, where):
        b = bytearray(good)
        for i in where:
            b[i * fb:(i + 1) * fb] = rec
        return bytes(b)

    assert _import(curve, good, N, COMPRESSED)[0] == 0
    bad_root = Z.non_residue_wire(params, rng).to_bytes(fb, "little")
    too_big = p.to_bytes(fb, "little")                                    # a coordinate >= p once the sign bit is masked
    too_big_signed = (p | (1 << (8 * fb - 1))).to_bytes(fb, "little")
    for where in ([0], [N // 2], [N - 1]):
        for flags in (COMPRESSED, COMPRESSED | PARITY):
            assert _import(curve, planted(bad_root, where), N, flags) == (MSMZ_ERR_POINT, 0)
        assert _import(curve, planted(too_big, where), N, COMPRESSED) == (MSMZ_ERR_RANGE, 0)
    assert _import(curve, planted(too_big_signed, [5]), N, COMPRESSED) == (MSMZ_ERR_RANGE, 0)
    both = bytearray(planted(bad_root, [0, 200]))
    both[100 * fb:101 * fb] = too_big
    assert _import(curve, bytes(both), N, COMPRESSED) == (MSMZ_ERR_RANGE, 0)   # RANGE beats POINT
    if fb == 48:   # bit 6 of the last byte (an arkworks infinity flag): the coordinate is >= 2^382 > p
        g = bytearray(Z.record(params, U.generator(params), "largest"))
        g[-1] |= 0x40
        assert _import(curve, planted(bytes(g), [7]), N, COMPRESSED) == (MSMZ_ERR_RANGE, 0)
    for wire in Z.zero_root_wires(params):   # a sign bit on a zero root
        rec = (wire | (1 << (8 * fb - 1))).to_bytes(fb, "little")
        for flags in (COMPRESSED, COMPRESSED | PARITY):
            assert _import(curve, planted(rec, [64]), N, flags) == (MSMZ_ERR_POINT, 0)
        assert _import(curve, planted(wire.to_bytes(fb, "little"), [64]), N, COMPRESSED)[0] == 0
    # a flagged record is not read: the same bad bytes under a flag are fine
    flags = bytearray(N)
    flags[0] = flags[N - 1] = 1
    both[100 * fb:101 * fb] = good[100 * fb:101 * fb]
    both[200 * fb:201 * fb] = too_big
    flags[200] = 1
    both[N * fb - fb:] = bad_root
    st, h = _import(curve, bytes(both), N, COMPRESSED, is_inf=flags)
    assert st == 0 and lib().msmz_free(curve._ctx, h) == 0
    # MSMZ_ERR_ARG, before any launch
    for fl, width in ((COMPRESSED | MONTGOMERY, 0), (PARITY, 0), (PARITY | MONTGOMERY, 0), (COMPRESSED, 2 * fb),
                      (COMPRESSED, fb - 4), (COMPRESSED | 32, 0), (COMPRESSED | PARITY, 2 * fb)):
        assert _import(curve, bytes(good) * 2, N, fl, width=width) == (MSMZ_ERR_ARG, 0), (fl, width)
    assert _import(curve, good, N, COMPRESSED, width=fb)[0] == 0
    assert _import(curve, good, N, 0, width=fb) == (MSMZ_ERR_ARG, 0)          # one coordinate is no x || y record
    from msm_zprize_amd._native import MsmzSrc
    sbuf = C.create_string_buffer(32 * 4)
    for fl in (COMPRESSED, PARITY, COMPRESSED | PARITY):                        # either flag on a scalar source
        src = MsmzSrc(C.cast(sbuf, C.c_void_p), 0, 32, fl, None, None)
        h = C.c_uint64(0)
        assert lib().msmz_import_scalars(curve._ctx, C.byref(src), 4, C.byref(h)) == MSMZ_ERR_ARG and h.value == 0
    # the download side
    arr = curve.Parallel.pointsFromBytes(bytes(good), N, compressed=True)
    out, inf = C.create_string_buffer(N * fb), C.create_string_buffer(N)
    dl = lib().msmz_download_points_compressed
    assert dl(curve._ctx, arr.handle, 0, N, out, inf, 0) == 0 and dl(curve._ctx, arr.handle, 0, N, out, None, PARITY) == 0
    # (a Weierstrass set holds 2 N records, the endomorphism images behind the points: the rules of msmz_download_points)
    for first, count, o, fl in ((0, N, None, 0), (0, N, out, COMPRESSED), (0, N, out, 1), (1, 2 * N, out, 0), (2 * N, 1, out, 0)):
        assert dl(curve._ctx, arr.handle, first, count, o, inf, fl) == MSMZ_ERR_ARG
    assert dl(curve._ctx, arr.handle + 1000, 0, 1, out, inf, 0) == MSMZ_ERR_ARG
    arr.free()
    with pytest.raises(mod_error()) as e:
        curve.Parallel.pointsFromBytes(planted(bad_root, [3]), N, compressed=True)
    assert e.value.status == MSMZ_ERR_POINT and "not a point" in str(e.value)
    _still_fine(curve, params)


def mod_error():
    from msm_zprize_amd._native import MsmzError
    return MsmzError


# ---------------------------------------------------------------------------------------------- several engines, one GPU
@pytest.mark.parametrize("label", ["bls12-377", "ed-on-bls12-377"])
def test_two_engines_on_one_gpu(mod, sets, torch, label):
    """devices = [0, 0]: a compressed import (host or device source) equals the upload, the compressed download equals
    the records, and a bad record is refused with the same status; on BLS12-377 also a set of 2^16 + 321 points, which
    both engines hold a share of"""
    params, s = P.CURVES[label], sets(label)
    fb = params["fe_bytes"]
    rng = random.Random(17)
    recs = Z.records(params, s["pts"], s["flags"], "parity", rng)
    mod.startThreads(devices=[0, 0])
    multi = (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(mod.curves.BY_LABEL[label])
    try:
        up = multi.Parallel.pointsFromBytes(s["xy"], N, is_inf=s["inf"])
        want = multi.Affine.toBigints(up)
        assert [_strip(q) for q in want] == s["pts"]
        f = torch.frombuffer(bytearray(s["flags"]), dtype=torch.uint8)
        arrs = [multi.Parallel.pointsFromBytes(recs, N, is_inf=s["flags"], compressed=True, sign="parity"),
                multi.Parallel.pointsFromTensor(_tensor(torch, recs, N, fb, "cuda", True), is_inf=f.cuda(), compressed=True,
                                                sign="parity")]
        for arr in arrs:
            assert multi.Affine.toBigints(arr) == want
            assert multi.Affine.toCompressedBytes(arr, sign="largest") == Z.want_compressed(params, s["pts"], "largest")
            assert multi.Affine.toCompressedBytes(arr, 300, 21, sign="parity") == Z.want_compressed(params, s["pts"][300:], "parity")
            arr.free()
        bad = bytearray(recs)
        assert not s["flags"][12]
        bad[12 * fb:13 * fb] = Z.non_residue_wire(params, rng).to_bytes(fb, "little")
        assert _import(multi, bytes(bad), N, COMPRESSED | PARITY, is_inf=s["flags"]) == (MSMZ_ERR_POINT, 0)
        up.free()
        if label == "bls12-377":
            # a set that both engines hold a share of (blocks of 2^16 records are dealt round-robin): records compressed by
            # the device itself; a bad record on either share is refused, and RANGE on one engine beats POINT on the other
            n = (1 << 16) + N
            p = params["modulus"]
            gen = multi.Parallel.randomPointsFast(n, 5)
            want = multi.Affine.toBigints(gen)
            for sign in Z.SIGNS:
                big, inf = multi.Affine.toCompressedBytes(gen, sign=sign)
                assert inf == bytes(n)
                back = multi.Parallel.pointsFromBytes(big, n, compressed=True, sign=sign)
                assert multi.Affine.toBigints(back) == want
                assert multi.Affine.toCompressedBytes(back, (1 << 16) - 10, 30, sign=sign) == (big[((1 << 16) - 10) * fb:((1 << 16) + 20) * fb], bytes(30))
                back.free()
            no_root, too_big = Z.non_residue_wire(params, rng).to_bytes(fb, "little"), p.to_bytes(fb, "little")
            for plant, status in (({5: no_root}, MSMZ_ERR_POINT), ({(1 << 16) + 7: no_root}, MSMZ_ERR_POINT),
                                  ({(1 << 16) + 7: too_big}, MSMZ_ERR_RANGE), ({5: no_root, (1 << 16) + 7: too_big}, MSMZ_ERR_RANGE),
                                  ({5: too_big, (1 << 16) + 7: no_root}, MSMZ_ERR_RANGE)):
                b = bytearray(big)
                for i, rec in plant.items():
                    b[i * fb:(i + 1) * fb] = rec
                assert _import(multi, bytes(b), n, COMPRESSED | PARITY) == (status, 0), sorted(plant)
            gen.free()
    finally:
        multi.close()
        mod.startThreads()

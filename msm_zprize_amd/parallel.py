"""Host-side mirror of the reference's curve factories (`src/parallel.ts`).

    from msm_zprize_amd import Weierstrass, startThreads, stopThreads
    from msm_zprize_amd.curves import bls12377Params
    startThreads()                                   # parallel.ts:291-315  (here: pick the GPU)
    Curve = Weierstrass.create(bls12377Params)       # parallel.ts:40-177
    points = Curve.Parallel.randomPointsFast(N)      # handles to device-resident inputs
    scalars = Curve.Parallel.randomScalars(N)
    out = Curve.Parallel.msmUnsafe(scalars, points, N, True)       # {"result": ..., "log": [...]}
    Curve.Affine.toBigint(out["result"])             # {"x": .., "y": .., "isZero": ..}

Same names, argument order and error behaviour as the reference where Python allows (the reference's
"pointers" into wasm memory become handle objects for device memory; its promises become plain
return values).  Everything below the `Parallel` methods runs in HIP through the C ABI of
include/msmz.h -- this module contains no arithmetic.
"""
import ctypes as C

from . import _native
from ._native import MsmzCheckResult, MsmzFixedBase, MsmzLog, MsmzMul, MsmzMulOpts, MsmzNtt, MsmzOpts, MsmzScalarRec, MsmzScalarTerm, MsmzSegment, MsmzSrc, lib
from ._native import check as _check   # (`check=` is a public keyword of pointsFromBytes / pointsFromTensor)

_state = {"devices": None}

MAX_DEVICES = 8


def startThreads(n=None, device=None, devices=None):
    """parallel.ts:291-315.  The reference spawns n-1 workers that share one MSM; here the workers are GPUs:
    `n` = number of GPUs a curve context drives (devices 0..n-1; every input set is split over them and the
    partial sums are added on the host -- msmz_create with n_devices = n).  `device` picks one GPU (default:
    LOCAL_RANK or 0, the one-process-per-GPU launch of bench.py); `devices` lists ids explicitly (an id may
    repeat: several engines on one GPU, used to rehearse the scheduler)."""
    import os
    if devices is None:
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0")) if n in (None, 1) else 0
        devices = [int(device) + i for i in range(int(n) if n else 1)]
    devices = [int(d) for d in devices]
    if not 1 <= len(devices) <= MAX_DEVICES:
        raise ValueError(f"startThreads: 1..{MAX_DEVICES} devices, got {len(devices)}")
    _state["devices"] = devices
    lib()  # fail early if the HIP library is not built
    return devices[0] if len(devices) == 1 else devices


def stopThreads():
    """parallel.ts:317-320."""
    _state["devices"] = None


class DeviceArray:
    """A device-resident input array (the reference's wasm-memory pointer lists)."""

    def __init__(self, curve, handle, n, kind):
        self.curve, self.handle, self.n, self.kind = curve, handle, n, kind

    def __len__(self):
        return self.n

    def free(self):
        if self.handle is not None:
            _check(lib().msmz_free(self.curve._ctx, self.handle), "msmz_free")
            self.handle = None


class SparseMatrix:
    """A device-resident sparse matrix (msmz_matrix_create): `shape` = (rows, columns), `nnz` its non-zeros, `orientations`
    the products it was built for ("rows": M x, "cols": M^T x, "both")."""

    def __init__(self, curve, handle, shape, nnz, orientations):
        self.curve, self.handle, self.shape, self.nnz, self.orientations = curve, handle, shape, nnz, orientations

    def free(self):
        if self.handle is not None:
            _check(lib().msmz_free(self.curve._ctx, self.handle), "msmz_free")
            self.handle = None


def _is_int(v):
    """an int, and not a bool"""
    return isinstance(v, int) and not isinstance(v, bool)


def _is_array(v, *kinds):
    """a resident array of one of `kinds`"""
    return isinstance(v, DeviceArray) and v.kind in kinds


def _resident(curve, kind, n, name, *args, after=(), out=None):
    """msmz_<name>(ctx, *args, &handle, *after) -> the resident array the call made: n entries of `kind`.  With `out` the
    call writes into that array (its handle goes in) and `out` comes back: the "out given or new" convention."""
    h = C.c_uint64(0 if out is None else out.handle)
    _check(getattr(lib(), name)(curve._ctx, *args, C.byref(h), *after), name)
    return DeviceArray(curve, h.value, n, kind) if out is None else out


class _Scalar:
    def __init__(self, curve):
        self._c = curve
        self.modulus = curve.params["order"]
        self.sizeInBits = (self.modulus - 1).bit_length()

    def toBigints(self, arr, first=0, count=None):
        """readBigint over a range (scripts/msm-weierstrass.ts:74-78)."""
        count = arr.n - first if count is None else count
        buf = C.create_string_buffer(32 * count)
        _check(lib().msmz_download_scalars(self._c._ctx, arr.handle, first, count, buf), "msmz_download_scalars")
        raw = buf.raw
        return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(count)]


class _Affine:
    def __init__(self, curve):
        self._c = curve

    def toBigint(self, point):
        """curve-affine.ts:220-233 -- {x, y, isZero}; accepts an MSM result or a canonical record."""
        return dict(point)

    def toBigints(self, arr, first=0, count=None):
        count = arr.n - first if count is None else count
        fb = self._c.fe_bytes
        buf = C.create_string_buffer(2 * fb * count)
        inf = C.create_string_buffer(count)
        _check(lib().msmz_download_points(self._c._ctx, arr.handle, first, count, buf, inf), "msmz_download_points")
        raw, flags = buf.raw, inf.raw
        return [self._c._point(raw, i, flags[i] != 0, zero_rule=False) for i in range(count)]

    def toCompressedBytes(self, arr, first=0, count=None, sign="largest"):
        """Points [first, first + count) of a resident point array as compressed records (msmz_download_points_compressed):
        -> (count * fe_bytes bytes, count flag bytes).  A record is the wire coordinate (x; y on the twisted Edwards
        curve), little-endian, with the sign of the other coordinate in bit 7 of the last byte; sign="largest": the bit
        says the canonical value is above (p - 1) / 2, sign="parity": that it is odd.  A point at infinity is an
        all-zero record with flag 1.  pointsFromBytes(..., compressed=True, sign=sign, is_inf=flags) reads them back."""
        first, count = compressed_range_args(arr, first, count, "toCompressedBytes")
        flag = sign_arg(sign, "toCompressedBytes")
        fb = self._c.fe_bytes
        buf = C.create_string_buffer(fb * count)
        inf = C.create_string_buffer(count)
        _check(lib().msmz_download_points_compressed(self._c._ctx, arr.handle, first, count, buf, inf, flag),
               "msmz_download_points_compressed")
        return buf.raw, inf.raw

    def compressPoint(self, point, sign="largest"):
        """An MSM result (or any {x, y, isZero}) as one compressed record, on the host: -> (fe_bytes bytes, isZero)."""
        return compress_point(self._c.params, point, sign)


class _Parallel:
    """Curve.Parallel (parallel.ts:135-145 / 250-258)."""

    def __init__(self, curve):
        self._c = curve

    # -- inputs ---------------------------------------------------------------------------------
    def randomPointsFast(self, n, seed=0x6D736D7A):
        return _resident(self._c, "points", n, "msmz_random_points", n, seed)

    def randomScalars(self, n, seed=0x6D736D7A):
        return _resident(self._c, "scalars", n, "msmz_random_scalars", n, seed)

    def pointsFromBytes(self, data, n=None, is_inf=None, montgomery=False, check=None, compressed=False, sign="largest"):
        """parallel.ts:97-112: x||y little-endian canonical, 2*fe_bytes per point.  montgomery=True: the coordinates are
        64-bit-limb Montgomery residues v * 2^(8 fe_bytes) mod p (msmz_import_points), converted on the GPU.
        compressed=True: fe_bytes per point, one coordinate (x; y on the twisted Edwards curve) with the sign of the
        other in bit 7 of the last byte -- sign="largest": set iff the canonical value is above (p - 1) / 2,
        sign="parity": iff it is odd; the GPU recovers the other coordinate and the array is an ordinary point array.  A
        record that is no point raises MsmzError (MSMZ_ERR_POINT).
        check="curve" / "subgroup": validate the new set on the GPU (checkPoints); a set that fails is freed and
        ValueError names its first bad point.  None (the default) validates nothing."""
        what = check_arg(check, "pointsFromBytes")
        form = compressed_arg(compressed, sign, montgomery, "pointsFromBytes")
        if what:
            return self._checked(self.pointsFromBytes(data, n, is_inf, montgomery, None, compressed, sign), what, "pointsFromBytes")
        fb = self._c.fe_bytes
        rec = fb if compressed else 2 * fb
        n = len(data) // rec if n is None else n
        if n <= 0 or len(data) < rec * n:
            raise ValueError(f"pointsFromBytes: {len(data)} bytes for {n} points of {rec} bytes")
        if is_inf is not None and len(is_inf) < n:
            raise ValueError(f"pointsFromBytes: {len(is_inf)} infinity flags for {n} points")
        data, flags = bytes(data), None if is_inf is None else bytes(is_inf)
        if montgomery or compressed:
            src = MsmzSrc(C.cast(C.c_char_p(data), C.c_void_p), 0, rec, form | (_native.MSMZ_SRC_MONTGOMERY if montgomery else 0), None,
                          None if flags is None else C.cast(C.c_char_p(flags), C.c_void_p))
            return _resident(self._c, "points", n, "msmz_import_points", C.byref(src), n)
        return _resident(self._c, "points", n, "msmz_upload_points", data, flags, n)

    def scalarsFromBytes(self, data, n=None, width=32, montgomery=False):
        """parallel.ts:114-133: 32 bytes little-endian per scalar.  width: bytes per scalar on the wire (4..32, a multiple
        of 4; only they cross PCIe, the resident scalars are zero-extended); montgomery=True: the records are
        v * 2^256 mod q in 64-bit limbs (width 32).  Either goes through msmz_import_scalars; the defaults are the
        plain upload."""
        width = scalar_width_arg(width, montgomery, "scalarsFromBytes")
        n = len(data) // width if n is None else n
        if n <= 0 or len(data) < width * n:
            raise ValueError(f"scalarsFromBytes: {len(data)} bytes for {n} scalars of {width} bytes")
        data = bytes(data)
        if width != 32 or montgomery:
            src = MsmzSrc(C.cast(C.c_char_p(data), C.c_void_p), 0, width,
                          _native.MSMZ_SRC_MONTGOMERY if montgomery else 0, None, None)
            return _resident(self._c, "scalars", n, "msmz_import_scalars", C.byref(src), n)
        return _resident(self._c, "scalars", n, "msmz_upload_scalars", data, n)

    # -- imports: the data where it is, in the form it has (msmz_import_*, include/msmz.h) ------------
    def _src(self, view):
        flags = (_native.MSMZ_SRC_DEVICE if view["device"] else 0) | (_native.MSMZ_SRC_MONTGOMERY if view["montgomery"] else 0)
        flags |= view.get("form", 0)   # (compressed records and their sign convention)
        stream = None
        if view["device"]:
            if view["stream"]:
                stream = view["stream"]
            else:   # torch's default stream is the null stream, which a pointer cannot name
                flags |= _native.MSMZ_SRC_DEFAULT_STREAM
        return MsmzSrc(view["ptr"], view["stride"], view["width"], flags, stream, view.get("is_inf"))

    def scalarsFromTensor(self, t, montgomery=False):
        """A resident scalar array from a torch tensor, read where it lies (msmz_import_scalars).  `t`: 2-D (n, k) with a
        contiguous last dimension -- width = k * itemsize bytes per scalar, 4..32, little-endian, zero-extended -- or 1-D of
        an 8-byte dtype (64-bit scalars); dimension 0 may be strided (a column view of a wider matrix).  A GPU tensor must
        be on the context's device and is read there, ordered after the work queued on torch's current stream (no copy
        through the host); a CPU tensor goes the host route, `width` bytes per scalar.  montgomery=True: 32-byte records
        v * 2^256 mod q.  A process that uses GPU tensors imports torch BEFORE this package loads libmsmz.so (before
        startThreads / the first curve): torch carries its own HIP runtime, a process drives the GPU through one copy
        only, and the copy loaded first serves both; the other way round torch finds no GPU."""
        view = tensor_view(t, self._c.devices, "scalars", self._c.fe_bytes, montgomery, "scalarsFromTensor")
        return _resident(self._c, "scalars", view["n"], "msmz_import_scalars", C.byref(self._src(view)), view["n"])

    def scalarsInto(self, dst, first, t, montgomery=False):
        """Write the scalars of tensor `t` (as scalarsFromTensor) over entries [first, first + n) of the resident scalar
        array `dst` (msmz_import_scalars_into): a batch assembled vector by vector.  Single-device contexts."""
        if not _is_array(dst, "scalars"):
            raise TypeError("scalarsInto: `dst` is a resident scalar array")
        view = tensor_view(t, self._c.devices, "scalars", self._c.fe_bytes, montgomery, "scalarsInto")
        if not _is_int(first) or first < 0 or first + view["n"] > len(dst):
            raise ValueError(f"scalarsInto: entries [{first!r}, +{view['n']}) of an array of {len(dst)}")
        _check(lib().msmz_import_scalars_into(self._c._ctx, dst.handle, first, C.byref(self._src(view)), view["n"]),
               "msmz_import_scalars_into")
        return dst

    def pointsFromTensor(self, t, montgomery=False, is_inf=None, check=None, compressed=False, sign="largest"):
        """A resident point array from a torch tensor of n rows of 2 * fe_bytes bytes (x || y, little-endian), read where
        it lies (msmz_import_points); montgomery=True: coordinates v * 2^(8 fe_bytes) mod p.  compressed=True: rows of
        fe_bytes bytes, one coordinate and a sign bit, `sign` as in pointsFromBytes.  is_inf: optional 1-D contiguous
        1-byte tensor of n flags on the same device.  check: as pointsFromBytes."""
        what = check_arg(check, "pointsFromTensor")
        form = compressed_arg(compressed, sign, montgomery, "pointsFromTensor")
        if what:
            return self._checked(self.pointsFromTensor(t, montgomery, is_inf, None, compressed, sign), what, "pointsFromTensor")
        view = tensor_view(t, self._c.devices, "points", self._c.fe_bytes, montgomery, "pointsFromTensor", is_inf,
                           compressed=compressed)
        view["form"] = form
        return _resident(self._c, "points", view["n"], "msmz_import_points", C.byref(self._src(view)), view["n"])

    # -- exports: resident data into the caller's memory, in the form it wants (msmz_export_*, include/msmz.h) --------
    def _dst(self, view):
        s = self._src(view)   # (msmz_dst is msmz_src read in the other direction: the same fields and flags)
        return _native.MsmzDst(s.ptr, s.stride, s.width, s.flags, s.stream, s.is_inf)

    def _host_export(self, name, arr, first, N, rec, flags, want_inf):
        """msmz_export_<name> of entries [first, first + N) into fresh host buffers -> (N * rec bytes, N flag bytes or None)"""
        buf = C.create_string_buffer(rec * N)
        inf = C.create_string_buffer(N) if want_inf else None
        dst = _native.MsmzDst(C.addressof(buf), 0, rec, flags, None, C.addressof(inf) if want_inf else None)
        _check(getattr(lib(), name)(self._c._ctx, arr.handle, first, N, C.byref(dst)), name)
        return buf.raw, inf.raw if want_inf else None

    def scalarsToBytes(self, scalars, first=0, N=None, width=32, montgomery=False):
        """Entries [first, first + N) of a resident scalar array as N * width little-endian bytes (msmz_export_scalars, the
        host route): only `width` bytes per scalar cross PCIe, and a scalar that does not fit them raises MsmzError
        (MSMZ_ERR_RANGE).  montgomery=True: 32-byte records v * 2^256 mod q in 64-bit limbs.  The defaults return what
        Scalar.toBigints reads."""
        first, N = export_range_args(scalars, "scalars", first, N, "scalarsToBytes")
        width = scalar_width_arg(width, montgomery, "scalarsToBytes")
        flags = _native.MSMZ_SRC_MONTGOMERY if montgomery else 0
        return self._host_export("msmz_export_scalars", scalars, first, N, width, flags, False)[0]

    def pointsToBytes(self, points, first=0, N=None, montgomery=False):
        """Points [first, first + N) of a resident point array -> (N * 2 * fe_bytes bytes x || y, N flag bytes)
        (msmz_export_points, the host route).  montgomery=True: coordinates v * 2^(8 fe_bytes) mod p in 64-bit limbs,
        what pointsFromBytes(..., montgomery=True, is_inf=flags) reads back.  A point at infinity is an all-zero record
        with flag 1."""
        first, N = export_range_args(points, "points", first, N, "pointsToBytes")
        if not isinstance(montgomery, bool):
            raise TypeError("pointsToBytes: `montgomery` is a bool")
        flags = _native.MSMZ_SRC_MONTGOMERY if montgomery else 0
        return self._host_export("msmz_export_points", points, first, N, 2 * self._c.fe_bytes, flags, True)

    def _new_tensor(self, who, shape):
        import torch   # (only here and in tensor_view: the package imports without torch)
        if len(self._c.devices) != 1:
            raise ValueError(f"{who}: a context of {len(self._c.devices)} devices exports to host memory only; pass a CPU "
                             f"tensor as `out`")
        return torch.empty(shape, dtype=torch.uint8, device=f"cuda:{self._c.devices[0]}")

    def scalarsToTensor(self, scalars, out=None, first=0, N=None, width=32, montgomery=False):
        """Entries [first, first + N) of a resident scalar array into a torch tensor, written where it lies
        (msmz_export_scalars) -> the tensor.  `out`: any tensor scalarsFromTensor reads -- 2-D (n, k) with a contiguous
        last dimension (k * itemsize = the record's bytes, 4..32) and possibly strided rows, or 1-D of an 8-byte dtype --
        on the context's GPU (written there, ordered after the work queued on torch's current stream; nothing passes
        through the host) or on the CPU (the host route: `width` bytes per scalar cross PCIe); N=None: as many entries as
        `out` has rows; bytes between strided rows are not touched.  out=None: a new (N, width) uint8 tensor on the
        context's GPU; `width` names the record of that tensor only, an `out` brings its own.  A scalar that does not
        fit the record raises MsmzError (MSMZ_ERR_RANGE).  montgomery=True: 32-byte records v * 2^256 mod q in 64-bit
        limbs, what scalarsFromTensor(..., montgomery=True) reads.  The call returns when the GPU has written everything:
        any stream may read the tensor.  torch is imported before this package loads its library, as for
        scalarsFromTensor."""
        who = "scalarsToTensor"
        if out is None:
            first, N = export_range_args(scalars, "scalars", first, N, who)
            width = scalar_width_arg(width, montgomery, who)
            out = self._new_tensor(who, (N, width))
        view = export_tensor_view(scalars, "scalars", out, first, N, self._c.devices, self._c.fe_bytes, montgomery, who)
        _check(lib().msmz_export_scalars(self._c._ctx, scalars.handle, first, view["n"], C.byref(self._dst(view))),
               "msmz_export_scalars")
        return out

    def pointsToTensor(self, points, out=None, first=0, N=None, montgomery=False, compressed=False, sign="largest",
                       is_inf=None):
        """Points [first, first + N) of a resident point array into a torch tensor of rows of 2 * fe_bytes bytes (x || y;
        montgomery=True: coordinates v * 2^(8 fe_bytes) mod p) or, compressed=True, of fe_bytes bytes (one coordinate
        and a sign bit, `sign` as in toCompressedBytes), written where the tensor lies (msmz_export_points).  `out`: as
        pointsFromTensor reads it, GPU or CPU, rows possibly strided; None: a new uint8 tensor on the context's GPU.
        is_inf: a contiguous 1-D one-byte tensor on the same device that receives the infinity flags, or True: one is
        made.  -> the tensor, or (tensor, flags) when is_inf is given.  pointsFromTensor(tensor, ..., is_inf=flags) with
        the same form reads the set back."""
        who = "pointsToTensor"
        form = compressed_arg(compressed, sign, montgomery, who)
        if out is None:
            first, N = export_range_args(points, "points", first, N, who)
            out = self._new_tensor(who, (N, self._c.fe_bytes * (1 if compressed else 2)))
        if is_inf is True:
            import torch
            is_inf = torch.empty((int(out.shape[0]),), dtype=torch.uint8, device=out.device)
        elif is_inf is False:
            is_inf = None
        view = export_tensor_view(points, "points", out, first, N, self._c.devices, self._c.fe_bytes, montgomery, who,
                                  is_inf, compressed)
        view["form"] = form
        _check(lib().msmz_export_points(self._c._ctx, points.handle, first, view["n"], C.byref(self._dst(view))),
               "msmz_export_points")
        return out if is_inf is None else (out, is_inf)

    # -- validation (msmz_check_points, include/msmz.h) ---------------------------------------------
    def checkPoints(self, points, N=None, subgroup=True, first=0, verdicts=False):
        """Are points [first, first + N) of a resident point array on the curve and (subgroup=True) in the subgroup of
        prime order?  isOnCurve / isInSubgroup of the reference's curve API over a whole set, on the GPU.  Returns a
        CheckResult: ok, offCurve, offSubgroup, firstBad (an index of the array, None if ok) and, with verdicts=True,
        `verdicts`: N bytes, bit 0 = not on the curve, bit 1 = on the curve but outside the subgroup."""
        first, N, what = check_points_args(points, N, subgroup, first)
        res = MsmzCheckResult()
        buf = C.create_string_buffer(N) if verdicts else None
        _check(lib().msmz_check_points(self._c._ctx, points.handle, first, N, what, C.byref(res), buf), "msmz_check_points")
        bad = None if res.first_bad == _native.NO_INDEX else int(res.first_bad)
        return CheckResult(bad is None, int(res.off_curve), int(res.off_subgroup), bad, buf.raw if verdicts else None)

    # -- per-point multiplication (msmz_points_mul, include/msmz.h) -----------------------------------
    def mulPoints(self, scalars, points, N=None, addend=None, firstPoint=0, firstScalar=0, firstAddend=0, scalarBits=0,
                  subgroup=False):
        """A new resident point array: out[i] = [s_i] points[firstPoint + i] (+ addend[firstAddend + i]), i < N.
        `scalars` is a resident scalar array (s_i = scalars[firstScalar + i]) or a Python int below the group order:
        one scalar for every point.  `addend` may be `points` itself (an IPA fold: mulPoints(u, G, N, addend=G,
        firstPoint=N)).  The result is an ordinary point array: msm, msmBatch, precomputePoints, checkPoints take it.
        scalarBits = b: every scalar of the call is below 2^b, and the chain walks b bits only (0 = no bound; a scalar
        that breaks the bound fails the call).  subgroup=True: the caller vouches that every finite point of the range
        lies in the prime-order subgroup (checkPoints(..., subgroup=True) says so); the Weierstrass curves then run the
        GLV chain, about half as long.  For a point outside the subgroup that row of the result is unspecified."""
        a = mul_points_args(scalars, points, N, addend, firstPoint, firstScalar, firstAddend, self._c.params["order"])
        o = mul_points_opts(scalars, scalarBits, subgroup)
        m = MsmzMul(points.handle, a["firstPoint"], 0 if a["scalar"] is not None else scalars.handle, a["firstScalar"],
                    a["scalar"], 0 if addend is None else addend.handle, a["firstAddend"])
        return _resident(self._c, "points", a["N"], "msmz_points_mul_opts", C.byref(m), a["N"], C.byref(o))

    # -- fixed-base multiplication (msmz_points_fixed_base, include/msmz.h) ---------------------------
    def fixedBaseMul(self, scalars, base=None, N=None, firstScalar=0, scalarBits=0):
        """A new resident point array: out[i] = [scalars[firstScalar + i]] B, i < N, for ONE base B -- an SRS
        [tau^i]G from scalarPowers(tau, N), Pedersen vectors, points with known discrete logs.  `base`: None (the
        curve's generator), an affine point {x, y, isZero} as msm returns it, or (array, index): a point of a resident
        point array.  B need not lie in the subgroup.  The result is what mulPoints leaves for N copies of B, from a
        window table of multiples of B (kept for the next call on the same base) instead of a chain per point.
        scalarBits = b: every scalar of the range is below 2^b (0 = no bound; a scalar that breaks it fails the call)."""
        a = fixed_base_args(scalars, base, N, firstScalar, self._c.params["modulus"], self._c.fe_bytes)
        bits = scalar_bits_arg({"scalarBits": scalarBits}, "fixedBaseMul")
        f = MsmzFixedBase(a["baseHandle"], a["baseIndex"], a["baseBytes"], scalars.handle, a["firstScalar"], bits, 0)
        return _resident(self._c, "points", a["N"], "msmz_points_fixed_base", C.byref(f), a["N"])

    # -- arithmetic mod q over resident scalar arrays (msmz_scalars_*, include/msmz.h) -----------------
    def combineScalars(self, a, x, b=None, y=None, N=None, firstX=0, firstY=0, out=None, firstOut=0, firstA=0, firstB=0):
        """out[firstOut + i] = a_i x[firstX + i] (+ b_i y[firstY + i]) mod the group order, i < N.  `a` and `b` are Python
        ints below the group order (one coefficient for every i) or resident scalar arrays (a_i = a[firstA + i]).
        out=None: a new resident scalar array of N entries; otherwise entries [firstOut, firstOut + N) of `out` are
        overwritten, and `out` may be `x`, `y` or a coefficient array when the range is exactly theirs or apart from it
        (an IPA fold in place: combineScalars(1, v, uinv, v, N, firstY=N, out=v)).  Returns the array written."""
        t = combine_scalars_args(a, x, b, y, N, firstX, firstY, out, firstOut, firstA, firstB, self._c.params["order"])
        terms = [MsmzScalarTerm(v.handle, fv, 0 if c is None else c.handle, fc, k) for v, fv, c, fc, k in t["terms"]]
        return _resident(self._c, "scalars", t["N"], "msmz_scalars_combine", C.byref(terms[0]),
                         C.byref(terms[1]) if len(terms) > 1 else None, t["N"], t["firstOut"], out=out)

    def innerProduct(self, x, y=None, N=None, firstX=0, firstY=0):
        """sum_i x[firstX + i] y[firstY + i] mod the group order (y=None: sum_i x[firstX + i]) as a Python int; x and y
        may be one array and may overlap."""
        t = combine_scalars_args(1, x, None if y is None else 1, y, N, firstX, firstY, None, 0, 0, 0,
                                 self._c.params["order"], "innerProduct")
        buf = C.create_string_buffer(32)
        _check(lib().msmz_scalars_dot(self._c._ctx, x.handle, firstX, 0 if y is None else y.handle, firstY, t["N"], buf),
               "msmz_scalars_dot")
        return int.from_bytes(buf.raw, "little")

    def innerProducts(self, rows, cols, N=None, out=None, firstOut=0):
        """Every inner product of a family of row vectors with a family of column vectors in one call
        (msmz_scalars_dot_many): result[r][c] = sum_i rows[r][i] cols[c][i] mod the group order, i < N, each value what
        innerProduct gives for that pair.  `rows` (1 to 128) and `cols` (1 to 8) are lists of resident scalar arrays or
        (array, first) pairs; vectors may share arrays, overlap and be one range.  N=None: what the shortest vector
        leaves.  out=None: a list of len(rows) lists of ints.  With `out`, a resident scalar array, entries
        [firstOut, firstOut + len(rows) len(cols)) of it receive the values row-major (no other entry is written; the
        range may meet no input range) and `out` comes back -- for combineScalars or evaluateExpression without a
        crossing to the host.  Many multilinear tables at one point: eqTable(point), then innerProducts(tables, [eq])."""
        t = inner_products_args(rows, cols, N, out, firstOut)
        as_vecs = lambda pairs: (_native.MsmzScalarVec * len(pairs))(*[_native.MsmzScalarVec(a.handle, f) for a, f in pairs])
        rv, cv = as_vecs(t["rows"]), as_vecs(t["cols"])
        d = _native.MsmzDotMany(rv, len(t["rows"]), cv, len(t["cols"]), t["N"], 0)
        if out is not None:
            h = C.c_uint64(out.handle)
            _check(lib().msmz_scalars_dot_many(self._c._ctx, C.byref(d), None, firstOut, C.byref(h)), "msmz_scalars_dot_many")
            return out
        nr, nc = len(t["rows"]), len(t["cols"])
        buf = C.create_string_buffer(32 * nr * nc)
        _check(lib().msmz_scalars_dot_many(self._c._ctx, C.byref(d), buf, 0, None), "msmz_scalars_dot_many")
        raw = buf.raw
        return [[int.from_bytes(raw[32 * (r * nc + c):32 * (r * nc + c) + 32], "little") for c in range(nc)] for r in range(nr)]

    def evaluatePolynomials(self, polys, points, N=None):
        """result[r][c] = p_r(z_c) for polynomials in coefficient form: polys[r] a resident scalar array or (array,
        first) pair whose entry i is the coefficient of X^i, i < N, points[c] an int below the group order (1 to 8 of
        them).  One power vector per point (scalarPowers), ONE innerProducts call, and the vectors are freed again.  In
        evaluation form the same call serves: pass the barycentric weight vectors of the points as `cols` of
        innerProducts."""
        q = self._c.params["order"]
        t = inner_products_args(polys, polys[:1] if isinstance(polys, (list, tuple)) else polys, N, None, 0, "evaluatePolynomials")
        if not isinstance(points, (list, tuple)) or not all(_is_int(z) for z in points):
            raise TypeError("evaluatePolynomials: `points` is a list of ints")
        if not 1 <= len(points) <= _native.MSMZ_DOT_MANY_MAX_COLS:
            raise ValueError(f"evaluatePolynomials: {len(points)} points (1 to {_native.MSMZ_DOT_MANY_MAX_COLS})")
        for z in points:
            if not 0 <= z < q:
                raise ValueError(f"evaluatePolynomials: the point {z} is not in [0, group order)")
        powers = []
        try:
            for z in points:
                powers.append(self.scalarPowers(z, t["N"]))
            return self.innerProducts(t["rows"], powers, t["N"])
        finally:
            for a in powers:
                a.free()

    def scalarPowers(self, ratio, N, base=1):
        """A new resident scalar array: entry i = base ratio^i mod the group order (0^0 = 1)."""
        q = self._c.params["order"]
        for name, v in (("ratio", ratio), ("base", base)):
            if not _is_int(v):
                raise TypeError(f"scalarPowers: `{name}` is an int")
            if not 0 <= v < q:
                raise ValueError(f"scalarPowers: {name} = {v} is not in [0, group order)")
        if not _is_int(N) or not 1 <= N < 1 << 32:
            raise ValueError(f"scalarPowers: N = {N!r}")
        return _resident(self._c, "scalars", N, "msmz_scalars_powers", base.to_bytes(32, "little"), ratio.to_bytes(32, "little"), N)

    # -- recurrences and inversion over resident scalar arrays (msmz_scalars_recurrence / _inverse) ---
    def scalarRecurrence(self, a, b, N=None, init=None, reverse=False, exclusive=False, firstA=0, firstB=0, out=None,
                         firstOut=0):
        """y_i = a_i y_(i-1) + b_i mod the group order, i < N, from y_(-1) = init (reverse=True: y_i = a_i y_(i+1) + b_i
        from y_N = init, highest i first).  `a`: a resident scalar array (a_i = a[firstA + i]), a Python int (one
        multiplier for every i) or None (1); `b`: a resident scalar array or None (no addend); not both None.  init=None
        is 0 with an addend and 1 without.  out[firstOut + i] = y_i, or with exclusive=True the value the step at i
        started from.  out=None: a new array of N entries; otherwise `out` may be `a` or `b` when the range is exactly
        theirs or apart from it.  Returns (the array written, the final y as an int)."""
        t = scalar_recurrence_args(a, b, N, init, reverse, exclusive, firstA, firstB, out, firstOut, self._c.params["order"])
        rec = MsmzScalarRec(t["aHandle"], t["firstA"], t["a"], t["bHandle"], t["firstB"], t["init"], t["flags"])
        last = C.create_string_buffer(32)
        arr = _resident(self._c, "scalars", t["N"], "msmz_scalars_recurrence", C.byref(rec), t["N"], t["firstOut"],
                        after=(last,), out=out)
        return arr, int.from_bytes(last.raw, "little")

    def prefixProducts(self, x, N=None, exclusive=False, init=None, reverse=False, first=0, out=None, firstOut=0):
        """Running products of x[first + i]: (array, the full product).  exclusive=True: entry 0 is init (1), entry i the
        product of the i entries before it -- a grand product column Z."""
        return self.scalarRecurrence(x, None, N, init, reverse, exclusive, first, 0, out, firstOut)

    def prefixSums(self, x, N=None, exclusive=False, init=None, reverse=False, first=0, out=None, firstOut=0):
        """Running sums of x[first + i]: (array, the full sum)."""
        return self.scalarRecurrence(None, x, N, init, reverse, exclusive, 0, first, out, firstOut)

    def divideByLinear(self, p, z, N=None, first=0):
        """(p(X) - p(z)) / (X - z) for the polynomial with coefficients p[first + i], i < N (lowest degree first):
        (quotient, p(z)).  The quotient is a new array of N entries whose top entry is 0, so an MSM takes it against the
        same N points as p: a KZG opening proof."""
        if not _is_int(z):
            raise TypeError("divideByLinear: `z` is an int")
        if not _is_array(p, "scalars"):
            raise TypeError("divideByLinear: `p` is a resident scalar array")
        return self.scalarRecurrence(z, p, N, 0, True, True, 0, first)

    def invertScalars(self, x, N=None, first=0, out=None, firstOut=0):
        """out[firstOut + i] = x[first + i]^-1 mod the group order, 0 -> 0: (the array written, the number of zeros).
        out=None: a new array; `out` may be `x` over exactly the same range (in place) or apart from it."""
        t = invert_scalars_args(x, N, first, out, firstOut)
        zeros = C.c_uint64(0)
        arr = _resident(self._c, "scalars", t["N"], "msmz_scalars_inverse", x.handle, t["first"], t["N"], t["firstOut"],
                        after=(C.byref(zeros),), out=out)
        return arr, int(zeros.value)

    # -- number-theoretic transforms over resident scalar arrays (msmz_scalars_ntt) ------------------
    def ntt(self, x, logN, inverse=False, shift=None, root=None, nIn=None, count=1, first=0, out=None, firstOut=0):
        """`count` transforms of length n = 2^logN mod the group order, natural order in and out.  Input vector k is
        x[first + k nIn : first + (k + 1) nIn] continued with zeros (nIn=None: n); output vector k is
        out[firstOut + k n : firstOut + (k + 1) n].  Forward: out_k = sum_i x_i (g w^k)^i; inverse=True:
        x_i = g^-i n^-1 sum_k X_k w^(-i k) (nIn must be n).  `shift` is the coset shift g (an int, not 0; None: 1), `root` a
        primitive n-th root of unity w (None: rootOfUnity(logN)).  out=None: a new array of count n entries; otherwise
        `out` may be `x` over exactly the source range (in place, nIn = n) or apart from it.  Returns the array written."""
        t = ntt_args(x, logN, inverse, shift, root, nIn, count, first, out, firstOut, self._c.params["order"])
        arg = MsmzNtt(x.handle, t["first"], t["logN"], t["flags"], t["nIn"], t["count"], t["root"], t["shift"])
        return _resident(self._c, "scalars", t["count"] << t["logN"], "msmz_scalars_ntt", C.byref(arg), t["firstOut"], out=out)

    def rootOfUnity(self, logN):
        """The default primitive 2^logN-th root of unity of the scalar field (msmz_scalars_root_of_unity) as an int."""
        if not _is_int(logN) or not 0 <= logN < 1 << 32:
            raise ValueError(f"rootOfUnity: logN = {logN!r}")
        buf = C.create_string_buffer(32)
        _check(lib().msmz_scalars_root_of_unity(self._c.params["curve_id"], logN, buf), "msmz_scalars_root_of_unity")
        return int.from_bytes(buf.raw, "little")

    # -- multilinear polynomials over resident scalar arrays (msmz_scalars_eq_table / _mle_*, _sumcheck_round) --
    def eqTable(self, point, scale=1):
        """A new resident scalar array of 2^len(point) entries: entry i = scale eq(point, i) mod the group order,
        eq(r, i) = prod_j (b_j r_j + (1 - b_j)(1 - r_j)) over the bits b_j of i -- variable 0 is the lowest index bit.
        `point` is a list of at most 31 ints below the group order ([] gives the one entry `scale`)."""
        t = eq_table_args(point, scale, self._c.params["order"])
        return _resident(self._c, "scalars", 1 << t["nVars"], "msmz_scalars_eq_table", t["point"], t["nVars"], t["scale"])

    def evaluateMle(self, f, point, first=0):
        """f(point) = sum_i f[first + i] eq(point, i) over 2^len(point) entries, as a Python int; the eq table is not
        made.  The same value as innerProduct(f, eqTable(point))."""
        t = mle_eval_args(f, point, first, self._c.params["order"])
        buf = C.create_string_buffer(32)
        _check(lib().msmz_scalars_mle_eval(self._c._ctx, f.handle, t["first"], t["nVars"], t["point"], buf),
               "msmz_scalars_mle_eval")
        return int.from_bytes(buf.raw, "little")

    def bindMle(self, f, r, nVars=None, count=1, low=False, first=0, out=None, firstOut=0):
        """Binds one variable of `count` tables of 2^nVars entries (table k at f[first + k 2^nVars]) to the int r:
        out_i = f_i + r (f_(i+h) - f_i), h = 2^(nVars-1) (the high variable), or with low=True
        out_i = f_(2i) + r (f_(2i+1) - f_(2i)) (variable 0).  Output table k is out[firstOut + k h : ...].  nVars=None:
        what the entries from `first` make of `count` equal tables.  out=None: a new array of count h entries; `out` may
        be `f` itself only with count=1, low=False and firstOut == first (the low half is overwritten), or over a range
        apart from the whole source.  Returns the array written."""
        t = mle_bind_args(f, r, nVars, count, low, first, out, firstOut, self._c.params["order"])
        b = _native.MsmzMleBind(f.handle, t["first"], t["nVars"], t["count"], t["flags"], t["r"])
        return _resident(self._c, "scalars", t["N"], "msmz_scalars_mle_bind", C.byref(b), t["firstOut"], out=out)

    def sumcheckRound(self, tables, terms, nVars=None, low=False):
        """The round polynomial of a sumcheck over sum_i sum_T c_T prod_(j in T) tables[j][i]: a list of d + 1 ints
        g(0) .. g(d), g(t) = sum_(i < 2^(nVars-1)) sum_T c_T prod_(j in T) ((1 - t) lo_j(i) + t hi_j(i)), where the round
        sums out the high variable ((lo, hi) = entries (i, i + 2^(nVars-1))) or with low=True variable 0 ((2i, 2i + 1)).
        `tables`: 1 to 6 resident scalar arrays or (array, first) pairs; `terms`: 1 to 8 pairs (c, mask), c an int below
        the group order or None (1), bit j of mask making table j a factor, at most 4 factors; d = the most factors of a
        term.  nVars=None: what the first table holds from its `first`.  Bind every table with bindMle(.., low=low) to go
        on to the next round."""
        t = sumcheck_round_args(tables, terms, nVars, low, self._c.params["order"])
        tabs = (_native.MsmzSumcheckTable * len(t["tables"]))(*[_native.MsmzSumcheckTable(a.handle, f) for a, f in t["tables"]])
        trms = (_native.MsmzSumcheckTerm * len(t["terms"]))(*[_native.MsmzSumcheckTerm(c, m) for c, m in t["terms"]])
        s = _native.MsmzSumcheck(tabs, len(t["tables"]), t["nVars"], trms, len(t["terms"]), t["flags"])
        degree = C.c_uint32(0)
        buf = C.create_string_buffer(32 * (_native.MSMZ_SUMCHECK_MAX_DEGREE + 1))
        _check(lib().msmz_scalars_sumcheck_round(self._c._ctx, C.byref(s), C.byref(degree), buf), "msmz_scalars_sumcheck_round")
        return [int.from_bytes(buf.raw[32 * k:32 * k + 32], "little") for k in range(degree.value + 1)]

    def sumcheckStep(self, tables, terms, nVars, r, out=None, low=False):
        """One step of a sumcheck prover in one call (msmz_scalars_sumcheck_step): binds every table of 2^nVars entries
        to the int r, as bindMle(.., low=low) does, and returns (degree, [g(0) .. g(degree)]), the polynomial
        sumcheckRound(.., nVars - 1, low) gives over the bound tables -- the same ints as the two-call route.  `tables`
        and `terms` are sumcheckRound's.  `out`: one resident scalar array or (array, first) pair per table, receiving
        its 2^(nVars-1) bound entries; each apart from every other destination and from every other table, and apart
        from its own table or exactly that table's low half (low=False only).  out=None: every table in place, its low
        half overwritten (low=False only).  nVars=None: what the first table holds.  nVars == 1 is the last step: the
        bound tables have one entry each and (0, [sum_T c_T prod_(j in T) bound_j]) comes back, the final claim."""
        t = sumcheck_step_args(tables, terms, nVars, r, out, low, self._c.params["order"])
        as_tables = lambda pairs: (_native.MsmzSumcheckTable * len(pairs))(*[_native.MsmzSumcheckTable(a.handle, f) for a, f in pairs])
        tabs, outs = as_tables(t["tables"]), None if t["out"] is None else as_tables(t["out"])
        trms = (_native.MsmzSumcheckTerm * len(t["terms"]))(*[_native.MsmzSumcheckTerm(c, m) for c, m in t["terms"]])
        s = _native.MsmzSumcheckStep(tabs, outs, len(t["tables"]), t["nVars"], trms, len(t["terms"]), t["flags"], t["r"])
        degree = C.c_uint32(0)
        buf = C.create_string_buffer(32 * (_native.MSMZ_SUMCHECK_MAX_DEGREE + 1))
        _check(lib().msmz_scalars_sumcheck_step(self._c._ctx, C.byref(s), C.byref(degree), buf), "msmz_scalars_sumcheck_step")
        return degree.value, [int.from_bytes(buf.raw[32 * k:32 * k + 32], "little") for k in range(degree.value + 1)]

    def sumcheckProve(self, tables, terms, nVars, challenge, low=False):
        """The prover's side of a whole sumcheck over sum_i sum_T c_T prod_(j in T) tables[j][i]: one sumcheckRound, then
        one sumcheckStep per variable with r = challenge(values of the round before), an int below the group order --
        the transcript is the caller's.  Returns (polys, challenges, claim): the nVars round polynomials as lists of
        ints, the nVars challenges, and the final claim sum_T c_T prod_(j in T) f_j(r).  A host loop and nothing else.
        The tables are consumed: low=False binds them in place; low=True goes back and forth between each table and
        one scratch array per table, allocated here and freed before returning.  The tables lie apart from each other."""
        t = sumcheck_round_args(tables, terms, nVars, low, self._c.params["order"], "sumcheckProve")
        if not callable(challenge):
            raise TypeError("sumcheckProve: `challenge` is a function of the round's values returning an int")
        cur, n_vars = t["tables"], t["nVars"]
        polys, challenges, claim = [self.sumcheckRound(cur, terms, n_vars, low)], [], None
        spare = []
        try:
            if low:
                spare = [_resident(self._c, "scalars", 1 << (n_vars - 1), "msmz_alloc_scalars", 1 << (n_vars - 1)) for _ in cur]
            other = [(a, 0) for a in spare]
            for v in range(n_vars, 0, -1):
                r = challenge(list(polys[-1]))
                _, values = self.sumcheckStep(cur, terms, v, r, other if low else None, low)
                challenges.append(r)
                if v > 1:
                    polys.append(values)
                else:
                    claim = values[0]
                if low:
                    cur, other = other, cur
        finally:
            for a in spare:
                a.free()
        return polys, challenges, claim

    # -- sparse matrices against resident scalar arrays (msmz_matrix_create / _matrix_mul) -------------
    def sparseMatrix(self, rows, cols, values=None, shape=None, orientations="rows", firstValue=0):
        """A resident sparse matrix of shape = (nRows, nCols) from triples (rows[k], cols[k], values[k]) in any order;
        triples with the same (row, col) add up.  rows / cols: lists of ints, or 1-D buffers of unsigned 32-bit ints
        (array("I"), a numpy uint32 array).  values: a resident scalar array (value k = values[firstValue + k]), a list
        of ints below the group order or of 32-byte little-endian records (uploaded first, freed afterwards), or None:
        every value is 1.  orientations: "rows" builds for matVec(M, x), "cols" for matVec(M, x, transpose=True),
        "both" for either.  The matrix keeps its own copy: `values` may be freed or overwritten afterwards."""
        a = sparse_matrix_args(rows, cols, values, shape, orientations, firstValue, self._c.params["order"])
        vals, mine = values, False
        if a["upload"] is not None:
            vals, mine = self.scalarsFromBytes(a["upload"], a["nnz"]), True
        try:
            s = _native.MsmzSparse(a["row"], a["col"], 0 if vals is None else vals.handle, a["firstValue"], a["nnz"],
                                   a["shape"][0], a["shape"][1], a["flags"])
            h = C.c_uint64(0)
            _check(lib().msmz_matrix_create(self._c._ctx, C.byref(s), C.byref(h)), "msmz_matrix_create")
        finally:
            if mine:
                vals.free()
        return SparseMatrix(self._c, h.value, a["shape"], a["nnz"], orientations)

    def matVec(self, matrix, x, firstX=0, transpose=False, out=None, firstOut=0):
        """out[firstOut + i] = sum over the non-zeros (i, j, v) of v x[firstX + j] mod the group order, i < nRows; with
        transpose=True the sum runs over (j, i, v) and i < nCols.  out=None: a new resident scalar array; otherwise only
        entries [firstOut, firstOut + nRows) of `out` are written, and they may not meet the x range if `out` is `x`
        (x is gathered).  Returns the array written."""
        a = mat_vec_args(matrix, x, firstX, transpose, out, firstOut)
        v = _native.MsmzMatvec(matrix.handle, x.handle, firstX, a["flags"])
        return _resident(self._c, "scalars", a["N"], "msmz_matrix_mul", C.byref(v), firstOut, out=out)

    # -- lookup arguments: the multiplicities of a column in a table (msmz_scalars_lookup) -------------
    def lookupMultiplicities(self, column, table, *, firstColumn=0, N=None, firstTable=0, tableN=None, out=None, firstOut=0,
                             positions=False):
        """(multiplicities, info) for the column f = column[firstColumn : firstColumn + N] and the table t =
        table[firstTable : firstTable + tableN] (N, tableN = None: to the end of the array): a resident scalar array m of
        tableN entries, m[j] = #{i : f[i] == t[j]} if j is the lowest index among the table entries that hold t[j] and 0
        for every later duplicate -- the vector a logUp argument commits to, sum_j m_j / (beta + t_j) = sum_i 1 / (beta +
        f_i).  info = {"missing": entries of f that equal no table entry (not an error), "firstMissing": the lowest such
        index or None, "distinct": the distinct values of t}, and with positions=True "positions": a numpy uint32 array,
        positions[i] = the index of the first table entry equal to f[i], 0xffffffff where there is none.  out=None: a new
        array; otherwise entries [firstOut, firstOut + tableN) of `out`, which may meet neither the table range nor the
        column range of the same array.  Table and column may be one array and may overlap."""
        a = lookup_args(column, table, firstColumn, N, firstTable, tableN, out, firstOut, positions)
        pos = None
        if positions:
            import numpy as np
            pos = np.empty(a["N"], dtype=np.uint32)
        l = _native.MsmzLookup(table.handle, firstTable, a["tableN"], column.handle, firstColumn, a["N"],
                               None if pos is None else pos.ctypes.data_as(C.POINTER(C.c_uint32)), 0)
        res = _native.MsmzLookupResult()
        m = _resident(self._c, "scalars", a["tableN"], "msmz_scalars_lookup", C.byref(l), firstOut, after=(C.byref(res),), out=out)
        info = {"missing": int(res.n_missing), "distinct": int(res.n_distinct),
                "firstMissing": None if res.first_missing == _native.NO_INDEX else int(res.first_missing)}
        if positions:
            info["positions"] = pos
        return m, info

    # -- gate expressions: sums of products of rotated columns (msmz_scalars_expr) ---------------------
    def evaluateExpression(self, columns, terms, N=None, out=None, firstOut=0):
        """out[firstOut + i] = sum_T c_T prod_(f in T) column_f[(i + rot_f) mod N] mod the group order, i < N: the
        constraint expression of a PLONK-ish prover, entry by entry, in one launch.  `columns`: 1 to 16 resident scalar
        arrays or (array, first) pairs, each read as the N entries from its `first`; `terms`: 1 to 32 pairs (c, factors),
        c an int below the group order or None (1), factors a list of at most 8 column indices or (column, rot) pairs
        ([] makes the term the constant c; a factor may repeat: [0] * 5 is a^5).  A rotation is cyclic inside the
        column's N entries and any int32; over an extended coset of size 4 n pass 4 rot.  All terms together may read at
        most 32 distinct (column, rot mod N) pairs.  N=None: every column holds the same number of entries from its
        `first`, and that is N.  out=None: a new array of N entries; otherwise `out` may be a column that is read at
        rotation 0 only, over exactly its range (out = y out + gate is the term (y, [out]) next to the gate's, in
        place), or lie apart from every column the terms read.  Returns the array written."""
        a = expr_args(columns, terms, N, out, firstOut, self._c.params["order"])
        cols = (_native.MsmzExprColumn * len(a["columns"]))(*[_native.MsmzExprColumn(c.handle, f) for c, f in a["columns"]])
        facs = [(_native.MsmzExprFactor * max(1, len(fs)))(*[_native.MsmzExprFactor(c, r) for c, r in fs]) for _, fs in a["terms"]]
        trms = (_native.MsmzExprTerm * len(a["terms"]))(*[_native.MsmzExprTerm(c, fa if fs else None, len(fs), 0)
                                                          for (c, fs), fa in zip(a["terms"], facs)])
        e = _native.MsmzExpr(cols, len(a["columns"]), len(a["terms"]), trms, a["N"], 0)
        return _resident(self._c, "scalars", a["N"], "msmz_scalars_expr", C.byref(e), firstOut, out=out)

    def _checked(self, arr, what, who):
        try:
            res = self.checkPoints(arr, subgroup=bool(what & _native.MSMZ_CHECK_SUBGROUP))
        except Exception:
            arr.free()   # the check itself failed: the new set does not outlive the call either
            raise
        if not res.ok:
            arr.free()
            raise ValueError(f"{who}: point {res.firstBad} is not {'on the curve' if res.offCurve else 'in the subgroup'} "
                             f"(firstBad = {res.firstBad}; {res.offCurve} off the curve, {res.offSubgroup} outside the "
                             f"subgroup)")
        return arr

    def _assemble(self, vecs, N):
        """one resident set of len(vecs) * N scalars from device tensors / resident scalar arrays (msmBatch)"""
        if len(self._c.devices) != 1:
            raise TypeError("msmBatch: a list of resident arrays is not accepted on a multi-device context; pass ONE "
                            "resident array of B * N scalars or a list of host byte arrays")
        B = len(vecs)
        dst = _resident(self._c, "scalars", B * N, "msmz_alloc_scalars", B * N)
        try:
            for k, v in enumerate(vecs):
                if isinstance(v, DeviceArray):
                    if v.kind != "scalars" or len(v) < N or v.curve is not self._c:
                        raise ValueError(f"msmBatch: vector {k} is not a resident array of >= {N} scalars of this curve")
                    # resident -> resident: the scalars travel as 32-byte canonical records through the host
                    buf = C.create_string_buffer(32 * N)
                    _check(lib().msmz_download_scalars(self._c._ctx, v.handle, 0, N, buf), "msmz_download_scalars")
                    src = MsmzSrc(C.cast(buf, C.c_void_p), 0, 32, 0, None, None)
                    _check(lib().msmz_import_scalars_into(self._c._ctx, dst.handle, k * N, C.byref(src), N),
                           "msmz_import_scalars_into")
                else:
                    if len(v) < N:
                        raise ValueError(f"msmBatch: vector {k} holds {len(v)} scalars, fewer than N = {N}")
                    self.scalarsInto(dst, k * N, v[:N])
        except Exception:
            dst.free()
            raise
        return dst

    def pointsFromBigints(self, points):
        """Affine.writeBigints route (scripts/zprize23/submission-bls377.ts:90-93)."""
        fb = self._c.fe_bytes
        data = b"".join(int(p["x"]).to_bytes(fb, "little") + int(p["y"]).to_bytes(fb, "little") for p in points)
        inf = bytes(1 if p.get("isZero") else 0 for p in points)
        return self.pointsFromBytes(data, len(points), inf if any(inf) else None)

    def scalarsFromBigints(self, scalars):
        """Scalar.writeBigint route (submission-bls377.ts:95-102)."""
        return self.scalarsFromBytes(b"".join(int(s).to_bytes(32, "little") for s in scalars), len(scalars))

    # -- precomputed point sets ---------------------------------------------------------------------
    def precomputePoints(self, points, N, options=None, factor=0):
        """Fixed-base precomputation of the first N resident points (msmz_precompute_points): a new DeviceArray of kind
        "precomputed" that msm / msmUnsafe / msmBatch / msmBatchUnsafe accept in place of `points` (same results).
        `factor` = windows sharing one bucket set (0 = all; 1 is refused); options["c"] / options["glv"] fix the window
        size and GLV choice (default: the engine's), options["scalarBits"] the scalar bit bound the copies are built for
        (fewer windows, fewer copies; MSMs over the array then take that bound).  The copies' parameters are in the
        array's `info` dict."""
        options = dict(options or {})
        c, glv, factor = precompute_args(points, N, options, factor)
        # only c, glv and the bit bound reach the library: the MSM-only fields stay 0, whatever `options` holds
        opts = msm_opts({"c": c, "glv": glv, "scalarBits": options.get("scalarBits")}, "precomputePoints", glv, safe=0, buckets=0)
        arr = _resident(self._c, "precomputed", N, "msmz_precompute_points", points.handle, N, C.byref(opts), factor)
        vals = [C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32(), C.c_uint64()]
        _check(lib().msmz_precomputed_info(self._c._ctx, arr.handle, *[C.byref(v) for v in vals]), "msmz_precomputed_info")
        arr.info = dict(zip(("c", "glv", "factor", "K", "records"), (v.value for v in vals)))
        bits = C.c_int32()
        _check(lib().msmz_precomputed_scalar_bits(self._c._ctx, arr.handle, C.byref(bits)), "msmz_precomputed_scalar_bits")
        arr.info["scalarBits"] = bits.value
        return arr

    # -- the MSM --------------------------------------------------------------------------------
    def _msm(self, scalars, points, N, verbose, options, safe, buckets):
        opts = msm_opts(dict(options or {}), "msm", self._c.default_glv, safe, buckets, 1 if verbose else 0)
        out = C.create_string_buffer(2 * self._c.fe_bytes)
        inf = C.c_int()
        log = MsmzLog()
        if N <= 0 or N > len(points):
            raise ValueError(f"msm: N = {N} but the point set holds {len(points)}")
        if N > (len(scalars) if isinstance(scalars, DeviceArray) else len(scalars) // 32):
            raise ValueError(f"msm: N = {N} but fewer scalars were given")
        if isinstance(scalars, DeviceArray):
            st = lib().msmz_msm_resident(self._c._ctx, points.handle, scalars.handle, N, C.byref(opts), out,
                                         C.byref(inf), C.byref(log))
        else:
            st = lib().msmz_msm(self._c._ctx, points.handle, bytes(scalars), N, C.byref(opts), out, C.byref(inf),
                                C.byref(log))
        _check(st, "msmz_msm")
        return {"result": self._c._point(out.raw, 0, inf.value != 0), "log": _format_log(log), "stats": log}

    def msm(self, scalars, points, N, verbose=False, options=None):
        """Safe additions (msm-batched-affine.ts:74-328 with useSafeAdditions = true)."""
        return self._msm(scalars, points, N, verbose, options, 1, 0)

    def msmUnsafe(self, scalars, points, N, verbose=False, options=None):
        """msm-batched-affine.ts:574-586."""
        return self._msm(scalars, points, N, verbose, options, 0, 0)

    # -- batched MSM: many scalar vectors against one resident point set ---------------------------
    def _msm_batch(self, scalarsList, points, N, options, safe):
        options = dict(options or {})
        if N <= 0 or N > len(points):
            raise ValueError(f"msmBatch: N = {N} but the point set holds {len(points)}")
        assembled = None
        if hasattr(scalarsList, "dim") and hasattr(scalarsList, "data_ptr"):
            # a bare tensor could mean B rows of N 64-bit scalars or B * N records of k bytes: the caller says which
            raise TypeError("msmBatch: pass a list of B tensors, or one resident array made with scalarsFromTensor(t), "
                            "not a bare tensor")
        if is_device_list(scalarsList):
            assembled = scalarsList = self._assemble(list(scalarsList), N)
        try:
            return self._msm_batch_run(scalarsList, points, N, options, safe)
        finally:
            if assembled is not None:
                assembled.free()

    def _msm_batch_run(self, scalarsList, points, N, options, safe):
        kind, data, B = batch_scalars(scalarsList, N, options.get("batch"))
        opts = msm_opts(options, "msmBatch", self._c.default_glv, safe)
        if kind == "resident":
            return self._many(B, "msmz_msm_batch", lambda *res: lib().msmz_msm_batch_resident(
                self._c._ctx, points.handle, data.handle, N, B, C.byref(opts), *res))
        return self._many(B, "msmz_msm_batch", lambda *res: lib().msmz_msm_batch(
            self._c._ctx, points.handle, data, N, B, C.byref(opts), *res))

    def _many(self, B, name, call):
        """the tail of msmBatch and msmSegments: `call(out, is_inf, log)` is the library call -> its B results; the log of
        the call is left in `lastBatchLog`"""
        out = C.create_string_buffer(2 * self._c.fe_bytes * B)
        inf = (C.c_int * B)()
        log = MsmzLog()
        _check(call(out, inf, C.byref(log)), name)
        self.lastBatchLog = log
        raw = out.raw
        return [self._c._point(raw, k, inf[k] != 0) for k in range(B)]

    def msmBatch(self, scalarsList, points, N, options=None):
        """B MSMs over the first N points in one device pipeline (msmz_msm_batch): `scalarsList` is ONE resident
        scalar array of >= B * N scalars (vector k = entries [k N, (k + 1) N); B = options["batch"], default
        len // N) or a list of B host arrays in the scalarsFromBytes byte format.  Returns the B results, each in the
        form of msm()["result"]; the log of the call is left in `lastBatchLog`.  Safe additions."""
        return self._msm_batch(scalarsList, points, N, options, 1)

    def msmBatchUnsafe(self, scalarsList, points, N, options=None):
        """msmBatch with unsafe additions (msmUnsafe)."""
        return self._msm_batch(scalarsList, points, N, options, 0)

    # -- segmented MSM: every problem its own range of one point set and one scalar set -------------
    def _msm_segments(self, scalars, points, segments, options, safe):
        options = dict(options or {})
        segs = msm_segments_args(scalars, points, segments)
        B = len(segs)
        table = (MsmzSegment * B)(*[MsmzSegment(p, s, n) for p, s, n in segs])
        opts = msm_opts(options, "msmSegments", self._c.default_glv, safe)
        return self._many(B, "msmz_msm_segments", lambda *res: lib().msmz_msm_segments(
            self._c._ctx, points.handle, scalars.handle, table, B, C.byref(opts), *res))

    def msmSegments(self, scalars, points, segments, options=None):
        """One MSM per segment (msmz_msm_segments): `segments` is a sequence of (firstPoint, firstScalar, N), result k =
        sum_{i < N} scalars[firstScalar + i] * points[firstPoint + i] over ONE resident scalar array and ONE resident
        point array (plain or precomputed).  Segments may overlap or repeat and differ in length; segments of similar
        length share one device pipeline.  An IPA round: msmSegments(a, G, [(n, 0, n), (0, n, n)]) is L and R.  Returns
        the results in the caller's order, in the form of msmBatch; the log is left in `lastBatchLog`.  Safe additions."""
        return self._msm_segments(scalars, points, segments, options, 1)

    def msmSegmentsUnsafe(self, scalars, points, segments, options=None):
        """msmSegments with unsafe additions (msmUnsafe)."""
        return self._msm_segments(scalars, points, segments, options, 0)

    def msmProjective(self, scalars, points, N, options=None):
        """parallel.ts:69-87: no GLV, projective buckets (msm-basic.ts)."""
        options = dict(options or {})
        options["glv"] = 0
        return self._msm(scalars, points, N, True, options, 1, 1)


class CheckResult:
    """What checkPoints found (msmz_check_result)."""

    def __init__(self, ok, offCurve, offSubgroup, firstBad, verdicts=None):
        self.ok, self.offCurve, self.offSubgroup, self.firstBad, self.verdicts = ok, offCurve, offSubgroup, firstBad, verdicts

    def __repr__(self):
        return (f"CheckResult(ok={self.ok}, offCurve={self.offCurve}, offSubgroup={self.offSubgroup}, "
                f"firstBad={self.firstBad})")


def check_points_args(points, N, subgroup, first):
    """Arguments of checkPoints -> (first, N, what), checked before anything reaches the device."""
    if not _is_array(points, "points"):
        raise TypeError("checkPoints: `points` is a resident point array (pointsFromBytes / randomPointsFast); a "
                        "precomputed array is derived data: check the set it was made from")
    if not _is_int(first) or not 0 <= first < len(points):
        raise ValueError(f"checkPoints: first = {first!r} but the point set holds {len(points)}")
    if N is None:
        N = len(points) - first
    if not _is_int(N) or not 1 <= N <= len(points) - first:
        raise ValueError(f"checkPoints: points [{first}, +{N!r}) of a set of {len(points)}")
    what = _native.MSMZ_CHECK_CURVE | (_native.MSMZ_CHECK_SUBGROUP if subgroup else 0)
    return first, N, what


def mul_points_args(scalars, points, N, addend, firstPoint, firstScalar, firstAddend, order):
    """Arguments of mulPoints -> dict(N, firstPoint, firstScalar, firstAddend, scalar), checked before anything reaches
    the device.  scalar: the 32 little-endian bytes of a broadcast scalar, None for a resident scalar array."""
    if not _is_array(points, "points"):
        raise TypeError("mulPoints: `points` is a resident point array (pointsFromBytes / randomPointsFast); a "
                        "precomputed array is derived data")
    if addend is not None and not _is_array(addend, "points"):
        raise TypeError("mulPoints: `addend` is a resident point array or None")
    broadcast = _is_int(scalars)
    if not broadcast and not _is_array(scalars, "scalars"):
        raise TypeError("mulPoints: `scalars` is a resident scalar array or an int (one scalar for every point)")
    if broadcast and not 0 <= scalars < order:
        raise ValueError(f"mulPoints: the scalar {scalars} is not in [0, group order)")
    N = _ranges("mulPoints", [("firstPoint", firstPoint, points), ("firstScalar", firstScalar, None if broadcast else scalars),
                              ("firstAddend", firstAddend, addend)], N, limit=None)
    return {"N": N, "firstPoint": firstPoint, "firstScalar": firstScalar, "firstAddend": firstAddend,
            "scalar": scalars.to_bytes(32, "little") if broadcast else None}


def fixed_base_args(scalars, base, N, firstScalar, field, fe_bytes):
    """Arguments of fixedBaseMul -> dict(N, firstScalar, baseHandle, baseIndex, baseBytes), checked before anything
    reaches the device.  baseBytes: x || y of an affine base, little-endian (all zero for isZero: the point at infinity
    of a Weierstrass curve), None for the generator or a resident base."""
    if not _is_array(scalars, "scalars"):
        raise TypeError("fixedBaseMul: `scalars` is a resident scalar array (scalarsFromBytes, scalarPowers, ...)")
    handle, index, data = 0, 0, None
    if isinstance(base, tuple):
        if len(base) != 2 or not _is_array(base[0], "points"):
            raise TypeError("fixedBaseMul: a resident base is (point array, index); a precomputed array is derived data")
        if not _is_int(base[1]) or not 0 <= base[1] < len(base[0]):
            raise ValueError(f"fixedBaseMul: base index {base[1]!r} of a point array of {len(base[0])}")
        handle, index = base[0].handle, base[1]
    elif isinstance(base, dict):
        if not all(k in base for k in ("x", "y")) or not _is_int(base["x"]) or not _is_int(base["y"]):
            raise TypeError("fixedBaseMul: an affine base is {x, y, isZero} with int coordinates")
        zero = bool(base.get("isZero", False))
        for name in ("x", "y"):
            if not zero and not 0 <= base[name] < field:
                raise ValueError(f"fixedBaseMul: the base's {name} is not in [0, field modulus)")
        data = bytes(2 * fe_bytes) if zero else base["x"].to_bytes(fe_bytes, "little") + base["y"].to_bytes(fe_bytes, "little")
    elif base is not None:
        raise TypeError("fixedBaseMul: `base` is None (the generator), an affine point {x, y, isZero} or (point array, index)")
    N = _ranges("fixedBaseMul", [("firstScalar", firstScalar, scalars)], N, limit=None)
    return {"N": N, "firstScalar": firstScalar, "baseHandle": handle, "baseIndex": index, "baseBytes": data}


def mul_points_opts(scalars, scalarBits, subgroup):
    """scalarBits and subgroup of mulPoints -> msmz_mul_opts, checked before anything reaches the device: the bound as
    scalar_bits_arg checks it, a broadcast scalar against the bound, the vouch a bool."""
    if not isinstance(subgroup, bool):
        raise TypeError(f"mulPoints: subgroup = {subgroup!r} (True: every point lies in the prime-order subgroup)")
    bits = scalar_bits_arg({"scalarBits": scalarBits}, "mulPoints")
    if bits and _is_int(scalars) and scalars >> bits:
        raise ValueError(f"mulPoints: the scalar {scalars} is not below 2^{bits} (scalarBits)")
    o = MsmzMulOpts()
    o.flags = _native.MSMZ_MUL_SUBGROUP if subgroup else 0
    o.scalar_bits = bits
    return o


def msm_segments_args(scalars, points, segments):
    """Arguments of msmSegments -> [(firstPoint, firstScalar, N), ...] as ints, checked before anything reaches the
    device."""
    if not _is_array(points, "points", "precomputed"):
        raise TypeError("msmSegments: `points` is a resident point array (plain or precomputed)")
    if not _is_array(scalars, "scalars"):
        raise TypeError("msmSegments: `scalars` is a resident scalar array (scalarsFromBytes / scalarsFromTensor); "
                        "host scalars are uploaded first")
    if isinstance(segments, (str, bytes, bytearray, DeviceArray)) or not hasattr(segments, "__len__"):
        raise TypeError("msmSegments: `segments` is a sequence of (firstPoint, firstScalar, N)")
    segs = list(segments)
    if not segs:
        raise ValueError("msmSegments: no segments")
    if len(segs) >= 2 ** 32:
        raise ValueError(f"msmSegments: {len(segs)} segments")
    out = []
    for k, seg in enumerate(segs):
        if isinstance(seg, (str, bytes, bytearray)) or not hasattr(seg, "__len__") or len(seg) != 3:
            raise TypeError(f"msmSegments: segment {k} is not (firstPoint, firstScalar, N): {seg!r}")
        firstPoint, firstScalar, N = seg
        for name, v in (("firstPoint", firstPoint), ("firstScalar", firstScalar), ("N", N)):
            if not _is_int(v) or v < 0:
                raise ValueError(f"msmSegments: segment {k}: {name} = {v!r}")
        if N < 1:
            raise ValueError(f"msmSegments: segment {k}: N = {N}")
        if firstPoint + N > len(points):
            raise ValueError(f"msmSegments: segment {k}: points [{firstPoint}, +{N}) of a set of {len(points)}")
        if firstScalar + N > len(scalars):
            raise ValueError(f"msmSegments: segment {k}: scalars [{firstScalar}, +{N}) of a set of {len(scalars)}")
        out.append((firstPoint, firstScalar, N))
    return out


def combine_scalars_args(a, x, b, y, N, firstX, firstY, out, firstOut, firstA, firstB, order, who="combineScalars"):
    """Arguments of combineScalars -> dict(N, firstOut, terms), checked before anything reaches the device.  terms: one
    or two of (array, first, coefficient array or None, its first, 32 little-endian bytes of a broadcast coefficient or
    None: a coefficient array, or the coefficient 1)."""
    def scalars(v):
        return _is_array(v, "scalars")

    if not scalars(x):
        raise TypeError(f"{who}: `x` is a resident scalar array")
    if (b is None) != (y is None):
        raise TypeError(f"{who}: `b` and `y` come together")
    if y is not None and not scalars(y):
        raise TypeError(f"{who}: `y` is a resident scalar array or None")
    if out is not None and not scalars(out):
        raise TypeError(f"{who}: `out` is a resident scalar array or None")
    ranges = [("firstX", firstX, x), ("firstY", firstY, y)]
    coeffs = []
    for name, first_name, c, first in (("a", "firstA", a, firstA), ("b", "firstB", b, firstB)):
        if name == "b" and y is None:
            ranges.append((first_name, first, None))
            continue
        if _is_int(c):
            if not 0 <= c < order:
                raise ValueError(f"{who}: the coefficient {name} = {c} is not in [0, group order)")
            coeffs.append((None, None if c == 1 else c.to_bytes(32, "little")))   # (1: no product at all)
            ranges.append((first_name, first, None))
        elif scalars(c):
            coeffs.append((c, None))
            ranges.append((first_name, first, c))
        else:
            raise TypeError(f"{who}: `{name}` is an int (one coefficient for every entry) or a resident scalar array")
    N = _ranges(who, ranges + [("firstOut", firstOut, out)], N, out)
    terms = [(x, firstX) + (coeffs[0][0], firstA if coeffs[0][0] is not None else 0, coeffs[0][1])]
    if y is not None:
        terms.append((y, firstY) + (coeffs[1][0], firstB if coeffs[1][0] is not None else 0, coeffs[1][1]))
    return {"N": N, "firstOut": firstOut, "terms": terms}


def inner_products_args(rows, cols, N, out, firstOut, who="innerProducts"):
    """Arguments of innerProducts -> dict(rows, cols, N, firstOut), rows and cols as [(array, first)], checked before
    anything reaches the device, in the order of msmz_scalars_dot_many (include/msmz.h): the types, the two counts, N,
    firstOut without an array, every range inside its array, and a destination range that meets no input range."""
    def vectors(vs, name):
        if not isinstance(vs, (list, tuple)):
            raise TypeError(f"{who}: `{name}` is a list of resident scalar arrays or (array, first) pairs")
        pairs = []
        for v in vs:
            arr, first = v if isinstance(v, tuple) and len(v) == 2 else (v, 0)
            if not _is_array(arr, "scalars") or not _is_int(first):
                raise TypeError(f"{who}: a vector of `{name}` is a resident scalar array or an (array, first) pair")
            pairs.append((arr, first))
        return pairs

    rv, cv = vectors(rows, "rows"), vectors(cols, "cols")
    if out is not None and not _is_array(out, "scalars"):
        raise TypeError(f"{who}: `out` is a resident scalar array or None")
    if N is not None and not _is_int(N):
        raise TypeError(f"{who}: `N` is an int or None")
    if not _is_int(firstOut):
        raise TypeError(f"{who}: `firstOut` is an int")
    if not 1 <= len(rv) <= _native.MSMZ_DOT_MANY_MAX_ROWS:
        raise ValueError(f"{who}: {len(rv)} rows (1 to {_native.MSMZ_DOT_MANY_MAX_ROWS})")
    if not 1 <= len(cv) <= _native.MSMZ_DOT_MANY_MAX_COLS:
        raise ValueError(f"{who}: {len(cv)} columns (1 to {_native.MSMZ_DOT_MANY_MAX_COLS})")
    for arr, first in rv + cv:
        if not 0 <= first <= len(arr):
            raise ValueError(f"{who}: first = {first} of an array of {len(arr)}")
    if N is None:
        N = min(len(arr) - first for arr, first in rv + cv)
    if not 1 <= N < 1 << 32:
        raise ValueError(f"{who}: N = {N}")
    if firstOut < 0 or (out is None and firstOut != 0):
        raise ValueError(f"{who}: firstOut = {firstOut}" + ("" if out is not None else " without the array it indexes"))
    for arr, first in rv + cv:
        if N > len(arr) - first:
            raise ValueError(f"{who}: entries [{first}, +{N}) of an array of {len(arr)}")
    if out is not None:
        results = len(rv) * len(cv)
        if firstOut > len(out) or results > len(out) - firstOut:
            raise ValueError(f"{who}: entries [{firstOut}, +{results}) of an array of {len(out)}")
        for arr, first in rv + cv:
            if arr.handle == out.handle and first < firstOut + results and firstOut < first + N:
                raise ValueError(f"{who}: the destination [{firstOut}, +{results}) meets the input range [{first}, +{N}) "
                                 f"of the same array")
    return {"rows": rv, "cols": cv, "N": N, "firstOut": firstOut}


def _ranges(who, ranges, N, out=None, limit=1 << 32):
    """The range checks of every operation over resident arrays: ranges = [(name, first, array or None)] -> N (None: what
    the shortest array leaves).  Every `first` is an index of its array, and 0 without one; 1 <= N < limit (None: no
    bound) fits every array from its `first`.  With `out` the last range is the destination: it may be an input's range
    exactly or apart from it, never overlap it in part."""
    for name, first, arr in ranges:
        if not _is_int(first) or first < 0:
            raise ValueError(f"{who}: {name} = {first!r}")
        if arr is None and first != 0:
            raise ValueError(f"{who}: {name} = {first} without the array it indexes")
        if arr is not None and first >= len(arr):
            raise ValueError(f"{who}: {name} = {first} but the array holds {len(arr)}")
    if N is None:
        N = min(len(arr) - first for _, first, arr in ranges if arr is not None)
    if not _is_int(N) or N < 1 or (limit is not None and N >= limit):
        raise ValueError(f"{who}: N = {N!r}")
    for name, first, arr in ranges:
        if arr is not None and N > len(arr) - first:
            raise ValueError(f"{who}: entries [{first}, +{N}) from {name} of an array of {len(arr)}")
    if out is not None:
        firstOut = ranges[-1][1]
        for name, first, arr in ranges[:-1]:
            if arr is not None and arr.handle == out.handle and first != firstOut and abs(first - firstOut) < N:
                raise ValueError(f"{who}: the destination [{firstOut}, +{N}) overlaps the input range [{first}, +{N}) "
                                 f"({name}) in part; it may be that range exactly or apart from it")
    return N


def scalar_recurrence_args(a, b, N, init, reverse, exclusive, firstA, firstB, out, firstOut, order,
                           who="scalarRecurrence"):
    """Arguments of scalarRecurrence -> dict(N, firstOut, aHandle, firstA, a, bHandle, firstB, init, flags), checked before
    anything reaches the device.  a / init: the 32 little-endian bytes of a broadcast value, or None."""
    def scalars(v):
        return _is_array(v, "scalars")

    broadcast = _is_int(a)
    if a is not None and not broadcast and not scalars(a):
        raise TypeError(f"{who}: `a` is a resident scalar array, an int (one multiplier for every entry) or None (1)")
    if b is not None and not scalars(b):
        raise TypeError(f"{who}: `b` is a resident scalar array or None (no addend)")
    if a is None and b is None:
        raise TypeError(f"{who}: neither a multiplier nor an addend: nothing to do")
    if out is not None and not scalars(out):
        raise TypeError(f"{who}: `out` is a resident scalar array or None")
    if init is not None and not _is_int(init):
        raise TypeError(f"{who}: `init` is an int or None")
    for name, v in (("reverse", reverse), ("exclusive", exclusive)):
        if not isinstance(v, bool):
            raise TypeError(f"{who}: `{name}` is a bool")
    for name, v in (("a", a if broadcast else None), ("init", init)):
        if v is not None and not 0 <= v < order:
            raise ValueError(f"{who}: {name} = {v} is not in [0, group order)")
    ranges = [("firstA", firstA, a if scalars(a) else None), ("firstB", firstB, b), ("firstOut", firstOut, out)]
    if N is None and not scalars(a) and b is None and out is None:
        raise ValueError(f"{who}: N is needed when no array gives the length")
    N = _ranges(who, ranges, N, out)
    return {"N": N, "firstOut": firstOut, "aHandle": a.handle if scalars(a) else 0, "firstA": firstA,
            "a": a.to_bytes(32, "little") if broadcast else None, "bHandle": 0 if b is None else b.handle,
            "firstB": firstB, "init": None if init is None else init.to_bytes(32, "little"),
            "flags": (_native.MSMZ_REC_REVERSE if reverse else 0) | (_native.MSMZ_REC_EXCLUSIVE if exclusive else 0)}


def invert_scalars_args(x, N, first, out, firstOut, who="invertScalars"):
    """Arguments of invertScalars -> dict(N, first, firstOut), checked before anything reaches the device."""
    if not _is_array(x, "scalars"):
        raise TypeError(f"{who}: `x` is a resident scalar array")
    if out is not None and not _is_array(out, "scalars"):
        raise TypeError(f"{who}: `out` is a resident scalar array or None")
    N = _ranges(who, [("first", first, x), ("firstOut", firstOut, out)], N, out)
    return {"N": N, "first": first, "firstOut": firstOut}


def ntt_args(x, logN, inverse, shift, root, nIn, count, first, out, firstOut, order, who="ntt"):
    """Arguments of ntt -> dict(logN, flags, nIn, count, first, firstOut, root, shift), checked before anything reaches
    the device.  root / shift: the 32 little-endian bytes, or None.  Whether `root` is a primitive root of unity, and
    whether the field has transforms of this length at all, is the library's to say."""
    if not _is_array(x, "scalars"):
        raise TypeError(f"{who}: `x` is a resident scalar array")
    if out is not None and not _is_array(out, "scalars"):
        raise TypeError(f"{who}: `out` is a resident scalar array or None")
    if not isinstance(inverse, bool):
        raise TypeError(f"{who}: `inverse` is a bool")
    for name, v in (("shift", shift), ("root", root)):
        if v is not None and not _is_int(v):
            raise TypeError(f"{who}: `{name}` is an int or None")
        if v is not None and not 0 <= v < order:
            raise ValueError(f"{who}: {name} = {v} is not in [0, group order)")
    if shift == 0:
        raise ValueError(f"{who}: the coset shift is not 0")
    if not _is_int(logN) or not 0 <= logN < 32:
        raise ValueError(f"{who}: logN = {logN!r} (0..31)")
    n = 1 << logN
    if not _is_int(count) or count < 1 or count * n >= 1 << 32:
        raise ValueError(f"{who}: count = {count!r} transforms of {n} entries (1 <= count, count * n < 2^32)")
    if nIn is None:
        nIn = n
    if not _is_int(nIn) or not 1 <= nIn <= n:
        raise ValueError(f"{who}: nIn = {nIn!r} (1..{n})")
    if inverse and nIn != n:
        raise ValueError(f"{who}: an inverse transform reads whole vectors (nIn = {nIn}, n = {n})")
    for name, v, arr in (("first", first, x), ("firstOut", firstOut, out)):
        if not _is_int(v) or v < 0:
            raise ValueError(f"{who}: {name} = {v!r}")
        if arr is None and v != 0:
            raise ValueError(f"{who}: {name} = {v} without the array it indexes")
    if count * nIn > len(x) - first:
        raise ValueError(f"{who}: entries [{first}, +{count * nIn}) of an array of {len(x)}")
    if out is not None:
        if count * n > len(out) - firstOut:
            raise ValueError(f"{who}: entries [{firstOut}, +{count * n}) of an array of {len(out)}")
        same = first == firstOut and nIn == n
        apart = first + count * nIn <= firstOut or firstOut + count * n <= first
        if out.handle == x.handle and not same and not apart:
            raise ValueError(f"{who}: the destination [{firstOut}, +{count * n}) overlaps the source [{first}, "
                             f"+{count * nIn}) in part; it may be that range exactly (nIn = n) or apart from it")
    return {"logN": logN, "flags": (_native.MSMZ_NTT_INVERSE if inverse else 0) | (_native.MSMZ_NTT_COSET if shift is not None else 0),
            "nIn": nIn, "count": count, "first": first, "firstOut": firstOut,
            "root": None if root is None else root.to_bytes(32, "little"),
            "shift": None if shift is None else shift.to_bytes(32, "little")}


MLE_MAX_VARS = 31   # a resident array has fewer than 2^32 entries


def _mle_point(point, order, who):
    """a point of a multilinear polynomial -> (its variables, its 32-byte values in a row)"""
    if not isinstance(point, (list, tuple)) or not all(_is_int(r) for r in point):
        raise TypeError(f"{who}: `point` is a list of ints, one per variable")
    if len(point) > MLE_MAX_VARS:
        raise ValueError(f"{who}: {len(point)} variables (at most {MLE_MAX_VARS})")
    for j, r in enumerate(point):
        if not 0 <= r < order:
            raise ValueError(f"{who}: point[{j}] = {r} is not in [0, group order)")
    return len(point), b"".join(r.to_bytes(32, "little") for r in point)


def _mle_first(name, first, arr, who):
    if not _is_int(first) or first < 0:
        raise ValueError(f"{who}: {name} = {first!r}")
    if arr is None and first != 0:
        raise ValueError(f"{who}: {name} = {first} without the array it indexes")


def eq_table_args(point, scale, order, who="eqTable"):
    """Arguments of eqTable -> dict(nVars, point, scale), checked before anything reaches the device.  scale: its 32
    little-endian bytes, or None for 1."""
    n_vars, raw = _mle_point(point, order, who)
    if not _is_int(scale):
        raise TypeError(f"{who}: `scale` is an int")
    if not 0 <= scale < order:
        raise ValueError(f"{who}: scale = {scale} is not in [0, group order)")
    return {"nVars": n_vars, "point": raw, "scale": None if scale == 1 else scale.to_bytes(32, "little")}


def mle_eval_args(f, point, first, order, who="evaluateMle"):
    """Arguments of evaluateMle -> dict(nVars, point, first), checked before anything reaches the device."""
    if not _is_array(f, "scalars"):
        raise TypeError(f"{who}: `f` is a resident scalar array")
    n_vars, raw = _mle_point(point, order, who)
    _mle_first("first", first, f, who)
    if (1 << n_vars) > len(f) - first:
        raise ValueError(f"{who}: entries [{first}, +{1 << n_vars}) of an array of {len(f)}")
    return {"nVars": n_vars, "point": raw, "first": first}


def _mle_vars(n_vars, have, who, what):
    """nVars of bindMle / sumcheckRound, 1 .. 31; None: `have` entries must be a power of two, at least 2"""
    if n_vars is None:
        if have < 2 or have & (have - 1):
            raise ValueError(f"{who}: nVars is needed: {what} {have} entries, not a power of two >= 2")
        return have.bit_length() - 1
    if not _is_int(n_vars) or not 1 <= n_vars <= MLE_MAX_VARS:
        raise ValueError(f"{who}: nVars = {n_vars!r} (1..{MLE_MAX_VARS})")
    return n_vars


def mle_bind_args(f, r, nVars, count, low, first, out, firstOut, order, who="bindMle"):
    """Arguments of bindMle -> dict(nVars, count, flags, first, firstOut, r, N), checked before anything reaches the
    device.  N: the entries written, count 2^(nVars-1); r: its 32 little-endian bytes."""
    if not _is_array(f, "scalars"):
        raise TypeError(f"{who}: `f` is a resident scalar array")
    if out is not None and not _is_array(out, "scalars"):
        raise TypeError(f"{who}: `out` is a resident scalar array or None")
    if not _is_int(r):
        raise TypeError(f"{who}: `r` is an int")
    if not isinstance(low, bool):
        raise TypeError(f"{who}: `low` is a bool")
    if not 0 <= r < order:
        raise ValueError(f"{who}: r = {r} is not in [0, group order)")
    if not _is_int(count) or count < 1:
        raise ValueError(f"{who}: count = {count!r}")
    _mle_first("first", first, f, who)
    _mle_first("firstOut", firstOut, out, who)
    have = len(f) - first
    if nVars is None and (have < 0 or have % count):
        raise ValueError(f"{who}: nVars is needed: {have} entries are not {count} equal tables")
    nVars = _mle_vars(nVars, have // count if nVars is None else 0, who, "a table would hold")
    n, h = 1 << nVars, 1 << (nVars - 1)
    if count * n >= 1 << 32:
        raise ValueError(f"{who}: count = {count} tables of {n} entries (count * 2^nVars < 2^32)")
    if count * n > have:
        raise ValueError(f"{who}: entries [{first}, +{count * n}) of an array of {len(f)}")
    if out is not None:
        if count * h > len(out) - firstOut:
            raise ValueError(f"{who}: entries [{firstOut}, +{count * h}) of an array of {len(out)}")
        in_place = count == 1 and not low and firstOut == first
        apart = firstOut + count * h <= first or first + count * n <= firstOut
        if out.handle == f.handle and not in_place and not apart:
            raise ValueError(f"{who}: the destination [{firstOut}, +{count * h}) overlaps the source [{first}, +{count * n}); "
                             "it may be the low half of ONE table bound in its high variable, or apart from the source")
    return {"nVars": nVars, "count": count, "flags": _native.MSMZ_MLE_LOW if low else 0, "first": first,
            "firstOut": firstOut, "r": r.to_bytes(32, "little"), "N": count * h}


def sumcheck_round_args(tables, terms, nVars, low, order, who="sumcheckRound"):
    """Arguments of sumcheckRound -> dict(tables, nVars, terms, flags, degree), checked before anything reaches the
    device.  tables: [(array, first)]; terms: [(32 little-endian bytes or None, mask)]."""
    if not isinstance(tables, (list, tuple)) or not isinstance(terms, (list, tuple)):
        raise TypeError(f"{who}: `tables` and `terms` are lists")
    if not isinstance(low, bool):
        raise TypeError(f"{who}: `low` is a bool")
    tabs = []
    for t in tables:
        arr, first = t if isinstance(t, tuple) and len(t) == 2 else (t, 0)
        if not _is_array(arr, "scalars"):
            raise TypeError(f"{who}: a table is a resident scalar array or an (array, first) pair")
        _mle_first("first", first, arr, who)
        tabs.append((arr, first))
    if not 1 <= len(tabs) <= _native.MSMZ_SUMCHECK_MAX_TABLES:
        raise ValueError(f"{who}: {len(tabs)} tables (1..{_native.MSMZ_SUMCHECK_MAX_TABLES})")
    if not 1 <= len(terms) <= _native.MSMZ_SUMCHECK_MAX_TERMS:
        raise ValueError(f"{who}: {len(terms)} terms (1..{_native.MSMZ_SUMCHECK_MAX_TERMS})")
    out, degree = [], 0
    for t in terms:
        if not isinstance(t, (list, tuple)) or len(t) != 2:
            raise TypeError(f"{who}: a term is a pair (coefficient, mask)")
        c, mask = t
        if c is not None and not _is_int(c):
            raise TypeError(f"{who}: a coefficient is an int or None (1)")
        if not _is_int(mask):
            raise TypeError(f"{who}: a mask is an int, bit j for table j")
        if c is not None and not 0 <= c < order:
            raise ValueError(f"{who}: the coefficient {c} is not in [0, group order)")
        factors = bin(mask).count("1") if mask > 0 else 0
        if mask <= 0 or mask >> len(tabs) or factors > _native.MSMZ_SUMCHECK_MAX_DEGREE:
            raise ValueError(f"{who}: mask = {mask:#b}: 1..{_native.MSMZ_SUMCHECK_MAX_DEGREE} of the {len(tabs)} tables")
        degree = max(degree, factors)
        out.append((None if c is None else c.to_bytes(32, "little"), mask))
    nVars = _mle_vars(nVars, len(tabs[0][0]) - tabs[0][1], who, "the first table holds")
    for arr, first in tabs:
        if (1 << nVars) > len(arr) - first:
            raise ValueError(f"{who}: entries [{first}, +{1 << nVars}) of an array of {len(arr)}")
    return {"tables": tabs, "nVars": nVars, "terms": out, "flags": _native.MSMZ_MLE_LOW if low else 0, "degree": degree}


def sumcheck_step_args(tables, terms, nVars, r, out, low, order, who="sumcheckStep"):
    """Arguments of sumcheckStep -> dict(tables, out, nVars, terms, flags, degree, r), checked before anything reaches the
    device: those of sumcheckRound, then r, then the destinations and the overlap rules of include/msmz.h.  out:
    [(array, first)] or None (every table in place); degree: that of the polynomial returned (0 when nVars == 1)."""
    t = sumcheck_round_args(tables, terms, nVars, low, order, who)
    if not _is_int(r):
        raise TypeError(f"{who}: `r` is an int")
    if out is not None and not isinstance(out, (list, tuple)):
        raise TypeError(f"{who}: `out` is a list with one destination per table, or None")
    outs = []
    for o in out or ():
        arr, first = o if isinstance(o, tuple) and len(o) == 2 else (o, 0)
        if not _is_array(arr, "scalars"):
            raise TypeError(f"{who}: a destination is a resident scalar array or an (array, first) pair")
        _mle_first("first", first, arr, who)
        outs.append((arr, first))
    if not 0 <= r < order:
        raise ValueError(f"{who}: r = {r} is not in [0, group order)")
    tabs, n, h = t["tables"], 1 << t["nVars"], 1 << (t["nVars"] - 1)
    if out is not None and len(outs) != len(tabs):
        raise ValueError(f"{who}: {len(outs)} destinations for {len(tabs)} tables")
    dst = tabs if out is None else outs
    for arr, first in outs:
        if h > len(arr) - first:
            raise ValueError(f"{who}: entries [{first}, +{h}) of an array of {len(arr)}")
    meet = lambda a, fa, na, b, fb, nb: a.handle == b.handle and fa < fb + nb and fb < fa + na
    for j, (d, df) in enumerate(dst):
        for k in range(j):
            if meet(d, df, h, dst[k][0], dst[k][1], h):
                raise ValueError(f"{who}: the destinations of tables {k} and {j} overlap")
        for k, (s, sf) in enumerate(tabs):
            if not meet(d, df, h, s, sf, n):
                continue
            if k != j:
                raise ValueError(f"{who}: the destination of table {j} overlaps table {k}")
            if low or df != sf:
                raise ValueError(f"{who}: the destination of table {j} overlaps its table; it may be the table's low half "
                                 f"[{sf}, +{h}) with low=False, or apart from it")
    return {**t, "out": None if out is None else outs, "r": r.to_bytes(32, "little"),
            "degree": t["degree"] if t["nVars"] > 1 else 0}


def _index_array(name, v, bound, who):
    """row / column indices -> a ctypes array of uint32, every entry checked against `bound`"""
    import array
    if isinstance(v, (list, tuple)):
        if not all(_is_int(i) for i in v):
            raise TypeError(f"{who}: `{name}` is a list of ints or a buffer of unsigned 32-bit ints")
        for k, i in enumerate(v):
            if not 0 <= i < bound:
                raise ValueError(f"{who}: {name}[{k}] = {i} is not in [0, {bound})")
        buf = array.array("I", v)
    else:
        try:
            m = memoryview(v)
        except TypeError:
            raise TypeError(f"{who}: `{name}` is a list of ints or a buffer of unsigned 32-bit ints") from None
        if m.ndim != 1 or m.itemsize != 4 or m.format not in ("I", "L", "=I", "<I"):
            raise TypeError(f"{who}: `{name}` is a list of ints or a 1-D buffer of unsigned 32-bit ints")
        buf = array.array("I", m.tobytes())
        if len(buf) and max(buf) >= bound:
            k = next(k for k, i in enumerate(buf) if i >= bound)
            raise ValueError(f"{who}: {name}[{k}] = {buf[k]} is not in [0, {bound})")
    assert buf.itemsize == 4
    return (C.c_uint32 * len(buf)).from_buffer(buf) if len(buf) else (C.c_uint32 * 1)()


_ORIENTATIONS = {"rows": _native.MSMZ_MAT_ROWS, "cols": _native.MSMZ_MAT_COLS,
                 "both": _native.MSMZ_MAT_ROWS | _native.MSMZ_MAT_COLS}


def sparse_matrix_args(rows, cols, values, shape, orientations, firstValue, order, who="sparseMatrix"):
    """Arguments of sparseMatrix -> dict(row, col, nnz, shape, flags, firstValue, upload), checked before anything
    reaches the device.  row / col: ctypes arrays of uint32; upload: the 32-byte records of a host value list, or None
    (`values` is a resident array or absent)."""
    if not (isinstance(shape, (list, tuple)) and len(shape) == 2 and all(_is_int(d) for d in shape)):
        raise TypeError(f"{who}: `shape` is a pair of ints (nRows, nCols)")
    if orientations not in _ORIENTATIONS:
        raise ValueError(f"{who}: orientations = {orientations!r} (\"rows\", \"cols\" or \"both\")")
    n_rows, n_cols = shape
    for name, d in (("nRows", n_rows), ("nCols", n_cols)):
        if not 1 <= d < 1 << 32:
            raise ValueError(f"{who}: {name} = {d}")
    row = _index_array("rows", rows, n_rows, who)
    col = _index_array("cols", cols, n_cols, who)
    nnz = len(rows)
    if len(cols) != nnz:
        raise ValueError(f"{who}: {nnz} rows but {len(cols)} cols")
    if not 1 <= nnz < 1 << 32:
        raise ValueError(f"{who}: N = {nnz!r}")
    upload = None
    _mle_first("firstValue", firstValue, values if _is_array(values, "scalars") else None, who)
    if _is_array(values, "scalars"):
        if nnz > len(values) - firstValue:
            raise ValueError(f"{who}: entries [{firstValue}, +{nnz}) from firstValue of an array of {len(values)}")
    elif isinstance(values, (list, tuple)):
        if len(values) != nnz:
            raise ValueError(f"{who}: {nnz} rows but {len(values)} values")
        recs = []
        for k, v in enumerate(values):
            if _is_int(v):
                if not 0 <= v < order:
                    raise ValueError(f"{who}: values[{k}] = {v} is not in [0, group order)")
                recs.append(v.to_bytes(32, "little"))
            elif isinstance(v, (bytes, bytearray)) and len(v) == 32:
                if int.from_bytes(v, "little") >= order:
                    raise ValueError(f"{who}: values[{k}] is not in [0, group order)")
                recs.append(bytes(v))
            else:
                raise TypeError(f"{who}: a value is an int or 32 little-endian bytes")
        upload = b"".join(recs)
    elif values is not None:
        raise TypeError(f"{who}: `values` is a resident scalar array, a list of ints or of 32-byte records, or None")
    return {"row": row, "col": col, "nnz": nnz, "shape": (n_rows, n_cols), "flags": _ORIENTATIONS[orientations],
            "firstValue": firstValue, "upload": upload}


def mat_vec_args(matrix, x, firstX, transpose, out, firstOut, who="matVec"):
    """Arguments of matVec -> dict(N, flags), checked before anything reaches the device.  N: the entries written."""
    if not isinstance(matrix, SparseMatrix):
        raise TypeError(f"{who}: `matrix` is a sparse matrix (sparseMatrix)")
    if not _is_array(x, "scalars"):
        raise TypeError(f"{who}: `x` is a resident scalar array")
    if out is not None and not _is_array(out, "scalars"):
        raise TypeError(f"{who}: `out` is a resident scalar array or None")
    if not isinstance(transpose, bool):
        raise TypeError(f"{who}: `transpose` is a bool")
    if matrix.handle is None:
        raise ValueError(f"{who}: the matrix was freed")
    need = "cols" if transpose else "rows"
    if matrix.orientations not in (need, "both"):
        raise ValueError(f"{who}: transpose={transpose} needs a matrix built with orientations=\"{need}\" or \"both\", "
                         f"this one has \"{matrix.orientations}\"")
    n_out, n_in = matrix.shape if not transpose else matrix.shape[::-1]
    _mle_first("firstX", firstX, x, who)
    _mle_first("firstOut", firstOut, out, who)
    if n_in > len(x) - firstX:
        raise ValueError(f"{who}: entries [{firstX}, +{n_in}) from firstX of an array of {len(x)}")
    if out is not None:
        if n_out > len(out) - firstOut:
            raise ValueError(f"{who}: entries [{firstOut}, +{n_out}) from firstOut of an array of {len(out)}")
        if out.handle == x.handle and firstOut < firstX + n_in and firstX < firstOut + n_out:
            raise ValueError(f"{who}: the destination [{firstOut}, +{n_out}) overlaps the input range [{firstX}, +{n_in}) "
                             "(firstX); x is gathered, so the two may not meet at all")
    return {"N": n_out, "flags": _native.MSMZ_MATVEC_TRANSPOSE if transpose else 0}


def lookup_args(column, table, firstColumn, N, firstTable, tableN, out, firstOut, positions, who="lookupMultiplicities"):
    """Arguments of lookupMultiplicities -> dict(N, tableN), checked before anything reaches the device.  N: the column
    entries looked up; tableN: the table entries, which is also the entries written."""
    if not _is_array(column, "scalars"):
        raise TypeError(f"{who}: `column` is a resident scalar array")
    if not _is_array(table, "scalars"):
        raise TypeError(f"{who}: `table` is a resident scalar array")
    if out is not None and not _is_array(out, "scalars"):
        raise TypeError(f"{who}: `out` is a resident scalar array or None")
    if not isinstance(positions, bool):
        raise TypeError(f"{who}: `positions` is a bool")
    _mle_first("firstColumn", firstColumn, column, who)
    _mle_first("firstTable", firstTable, table, who)
    _mle_first("firstOut", firstOut, out, who)
    sizes = {}
    for name, n, first, arr, limit in (("N", N, firstColumn, column, (1 << 32) - 1), ("tableN", tableN, firstTable, table, 1 << 30)):
        if n is None:
            n = len(arr) - first
        if not _is_int(n) or not 1 <= n <= limit:
            raise ValueError(f"{who}: {name} = {n!r}")
        if n > len(arr) - first:
            raise ValueError(f"{who}: entries [{first}, +{n}) of an array of {len(arr)} ({name})")
        sizes[name] = n
    if out is not None:
        n_out = sizes["tableN"]
        if n_out > len(out) - firstOut:
            raise ValueError(f"{who}: entries [{firstOut}, +{n_out}) from firstOut of an array of {len(out)}")
        for name, arr, first, n in (("table", table, firstTable, sizes["tableN"]), ("column", column, firstColumn, sizes["N"])):
            if out.handle == arr.handle and firstOut < first + n and first < firstOut + n_out:
                raise ValueError(f"{who}: the destination [{firstOut}, +{n_out}) overlaps the {name} range [{first}, +{n}); "
                                 "both inputs are gathered, so it may meet neither at all")
    return sizes


def expr_args(columns, terms, N, out, firstOut, order, who="evaluateExpression"):
    """Arguments of evaluateExpression -> dict(columns, terms, N), checked before anything reaches the device.  columns:
    [(array, first)]; terms: [(32 little-endian bytes or None, [(column, rot)])]."""
    if not isinstance(columns, (list, tuple)) or not isinstance(terms, (list, tuple)):
        raise TypeError(f"{who}: `columns` and `terms` are lists")
    if out is not None and not _is_array(out, "scalars"):
        raise TypeError(f"{who}: `out` is a resident scalar array or None")
    cols = []
    for c in columns:
        arr, first = c if isinstance(c, tuple) and len(c) == 2 else (c, 0)
        if not _is_array(arr, "scalars"):
            raise TypeError(f"{who}: a column is a resident scalar array or an (array, first) pair")
        cols.append((arr, first))
    if not 1 <= len(cols) <= _native.MSMZ_EXPR_MAX_COLUMNS:
        raise ValueError(f"{who}: {len(cols)} columns (1..{_native.MSMZ_EXPR_MAX_COLUMNS})")
    if not 1 <= len(terms) <= _native.MSMZ_EXPR_MAX_TERMS:
        raise ValueError(f"{who}: {len(terms)} terms (1..{_native.MSMZ_EXPR_MAX_TERMS})")
    parsed = []
    for t in terms:
        if not isinstance(t, (list, tuple)) or len(t) != 2 or not isinstance(t[1], (list, tuple)):
            raise TypeError(f"{who}: a term is a pair (coefficient, [factors])")
        c, factors = t
        if c is not None and not _is_int(c):
            raise TypeError(f"{who}: a coefficient is an int or None (1)")
        if c is not None and not 0 <= c < order:
            raise ValueError(f"{who}: the coefficient {c} is not in [0, group order)")
        fs = []
        for f in factors:
            col, rot = f if isinstance(f, tuple) and len(f) == 2 else (f, 0)
            if not _is_int(col) or not _is_int(rot):
                raise TypeError(f"{who}: a factor is a column index or a pair (column, rot) of ints")
            if not 0 <= col < len(cols):
                raise ValueError(f"{who}: a factor names column {col} of {len(cols)}")
            if not -(1 << 31) <= rot < 1 << 31:
                raise ValueError(f"{who}: rot = {rot} is no int32")
            fs.append((col, rot))
        if len(fs) > _native.MSMZ_EXPR_MAX_DEGREE:
            raise ValueError(f"{who}: a term of {len(fs)} factors (0..{_native.MSMZ_EXPR_MAX_DEGREE})")
        parsed.append((None if c is None else c.to_bytes(32, "little"), fs))
    ranges = [(f"the first of column {k}", first, arr) for k, (arr, first) in enumerate(cols)]
    if N is None:
        for name, first, arr in ranges:   # (so that the lengths below are those of valid ranges)
            _mle_first(name, first, arr, who)
        lengths = {len(arr) - first for arr, first in cols}
        if len(lengths) != 1:
            raise ValueError(f"{who}: N is needed when the columns hold different numbers of entries: {sorted(lengths)}")
        N = lengths.pop()
    N = _ranges(who, ranges + [("firstOut", firstOut, out)], N, limit=1 << 32)
    operands = {(col, rot % N) for _, fs in parsed for col, rot in fs}
    if len(operands) > _native.MSMZ_EXPR_MAX_OPERANDS:
        raise ValueError(f"{who}: the terms read {len(operands)} distinct (column, rot mod N) pairs "
                         f"(at most {_native.MSMZ_EXPR_MAX_OPERANDS})")
    if out is not None:
        for k, (arr, first) in enumerate(cols):
            rots = {rot for col, rot in operands if col == k}
            if arr.handle != out.handle or not rots:
                continue
            if rots == {0}:
                if first != firstOut and abs(first - firstOut) < N:
                    raise ValueError(f"{who}: the destination [{firstOut}, +{N}) overlaps the input range [{first}, +{N}) "
                                     f"(column {k}) in part; it may be that range exactly or apart from it")
            elif abs(first - firstOut) < N:
                raise ValueError(f"{who}: the destination [{firstOut}, +{N}) overlaps the input range [{first}, +{N}) "
                                 f"(column {k}); the column is read rotated, so the two may not meet at all")
    return {"columns": cols, "terms": parsed, "N": N}


def check_arg(check, who):
    """check= of pointsFromBytes / pointsFromTensor -> the `what` bits of msmz_check_points (0: no validation)"""
    if check is None:
        return 0
    if check == "curve":
        return _native.MSMZ_CHECK_CURVE
    if check == "subgroup":
        return _native.MSMZ_CHECK_CURVE | _native.MSMZ_CHECK_SUBGROUP
    raise ValueError(f'{who}: check = {check!r} (None, "curve" or "subgroup")')


def precompute_args(points, N, options, factor):
    """Arguments of precomputePoints -> (c, glv, factor), checked before anything reaches the device."""
    if not _is_array(points, "points"):
        raise TypeError("precomputePoints: `points` is a resident point array (pointsFromBytes / randomPointsFast)")
    if not _is_int(N) or not 1 <= N <= len(points):
        raise ValueError(f"precomputePoints: N = {N!r} but the point set holds {len(points)}")
    if not _is_int(factor) or factor < 0 or factor == 1 or factor >= 2 ** 32:
        raise ValueError(f"precomputePoints: factor = {factor!r} (0 = all windows, or 2, 3, ...)")
    c = int(options.get("c") or 0)
    glv = int(options.get("glv", -1))
    if not 0 <= c <= 24:
        raise ValueError(f"precomputePoints: c = {c} (0 = the engine's choice, or 2..24)")
    if glv not in (-1, 0, 1):
        raise ValueError(f"precomputePoints: glv = {glv} (-1, 0 or 1)")
    scalar_bits_arg(options, "precomputePoints")
    return c, glv, factor


def msm_opts(options, who, glv, safe, buckets=None, timing=0):
    """`options` of an MSM call -> msmz_opts.  glv, safe: what holds without options["glv"] / ["useSafeAdditions"];
    buckets: None takes options["buckets"]; reserved[0] = reduceAffine (1: batched-affine first reduction level,
    reduceBucketsAffine), reserved[1] = scalarBits (every scalar is below 2^scalarBits; 0: no bound)."""
    opts = MsmzOpts()
    opts.c = int(options.get("c") or 0)
    opts.glv = int(options.get("glv", glv))
    opts.safe = int(options.get("useSafeAdditions", safe))
    opts.buckets = int(options.get("buckets", 0)) if buckets is None else buckets
    opts.timing = timing
    opts.reserved[0] = int(options.get("reduceAffine", 0))
    opts.reserved[1] = scalar_bits_arg(options, who)
    return opts


def scalar_bits_arg(options, who):
    """options["scalarBits"] -> msmz_opts.reserved[1]: "every scalar of this call is below 2^scalarBits".  0 / absent = no
    bound; a value of at least the scalar field's bit length means the same; the window count follows the bound, and a
    scalar that breaks it fails the call (MSMZ_ERR_RANGE).  Checked before anything reaches the device."""
    bits = options.get("scalarBits")
    if bits is None:
        return 0
    if not _is_int(bits) or not 0 <= bits <= 256:
        raise ValueError(f"{who}: scalarBits = {bits!r} (0 = no bound, or 1..256)")
    return bits


def scalar_width_arg(width, montgomery, who):
    """bytes per imported scalar record: 4..32, a multiple of 4; Montgomery records are 32 bytes"""
    if not _is_int(width) or not 4 <= width <= 32 or width % 4:
        raise ValueError(f"{who}: width = {width!r} (4..32 bytes, a multiple of 4)")
    if montgomery and width != 32:
        raise ValueError(f"{who}: Montgomery scalars are 32-byte records, not {width}")
    return width


def is_device_list(scalarsList):
    """msmBatch: a list whose vectors are all GPU tensors or resident scalar arrays (assembled with scalarsInto)?"""
    if isinstance(scalarsList, (DeviceArray, bytes, bytearray, memoryview, str)) or not hasattr(scalarsList, "__len__"):
        return False
    if hasattr(scalarsList, "dim"):   # a bare tensor is not a list of vectors (msmBatch refuses it)
        return False
    vecs = list(scalarsList)
    on_gpu = [getattr(getattr(v, "device", None), "type", None) == "cuda" for v in vecs]
    return bool(vecs) and any(on_gpu) and all(g or isinstance(v, DeviceArray) for g, v in zip(on_gpu, vecs))


def sign_arg(sign, who):
    """the sign convention of compressed records -> 0 ("largest") or MSMZ_SRC_SIGN_PARITY ("parity")"""
    if sign == "largest" and isinstance(sign, str):
        return 0
    if sign == "parity" and isinstance(sign, str):
        return _native.MSMZ_SRC_SIGN_PARITY
    raise ValueError(f"{who}: sign is 'largest' or 'parity', got {sign!r}")


def compressed_arg(compressed, sign, montgomery, who):
    """compressed= / sign= of pointsFromBytes and pointsFromTensor -> the msmz_src form flags (0: x || y records)"""
    if not isinstance(compressed, bool):
        raise TypeError(f"{who}: compressed is True or False, got {type(compressed).__name__}")
    flag = sign_arg(sign, who)
    if not compressed:
        if flag:
            raise ValueError(f"{who}: sign='parity' describes compressed records (compressed=True)")
        return 0
    if montgomery:
        raise ValueError(f"{who}: compressed records are canonical, not Montgomery residues")
    return _native.MSMZ_SRC_COMPRESSED | flag


def compressed_range_args(arr, first, count, who):
    """points [first, first + count) of a resident point array, count=None: to its end -> (first, count)"""
    if not _is_array(arr, "points"):
        raise TypeError(f"{who}: expected a resident point array")
    if not _is_int(first) or first < 0 or first >= len(arr):
        raise ValueError(f"{who}: first = {first!r} of an array of {len(arr)}")
    count = len(arr) - first if count is None else count
    if not _is_int(count) or count <= 0 or first + count > len(arr):
        raise ValueError(f"{who}: points [{first}, +{count!r}) of an array of {len(arr)}")
    return first, count


def compress_point(params, point, sign="largest"):
    """{x, y, isZero} -> (one compressed record of fe_bytes bytes, isZero), as msmz_download_points_compressed writes it:
    the wire coordinate (x; y on the twisted Edwards curve) little-endian, the sign of the other in bit 7 of the last
    byte; infinity is the all-zero record.  Pure Python, for MSM results."""
    parity = sign_arg(sign, "compressPoint") != 0
    p, fb = params["modulus"], params["fe_bytes"]
    if point.get("isZero") and params["kind"] == "weierstrass":
        return bytes(fb), True
    x, y = point["x"], point["y"]
    if not (_is_int(x) and _is_int(y) and 0 <= x < p and 0 <= y < p):
        raise ValueError("compressPoint: coordinates are ints in [0, p)")
    wire, other = (x, y) if params["kind"] == "weierstrass" else (y, x)
    bit = (other & 1) if parity else int(other > (p - 1) // 2)
    return (wire | (bit << (8 * fb - 1))).to_bytes(fb, "little"), False


def tensor_view(t, devices, kind, fe_bytes, montgomery, who, is_inf=None, compressed=False):
    """The arguments of an import from a tensor, checked before anything reaches the device.  `t` needs the tensor
    attributes used here (dim, shape, stride, element_size, device, data_ptr), so a fake will do; torch is imported only
    to ask a GPU tensor's current stream.  -> dict(ptr, n, width, stride (bytes), device, stream, montgomery[, is_inf])."""
    for a in ("dim", "shape", "stride", "element_size", "device", "data_ptr"):
        if not hasattr(t, a):
            raise TypeError(f"{who}: expected a torch.Tensor, got {type(t).__name__}")
    item = int(t.element_size())
    if t.dim() == 2:
        n, k = int(t.shape[0]), int(t.shape[1])
        if k > 1 and t.stride(1) != 1:
            raise ValueError(f"{who}: the last dimension must be contiguous (stride {t.stride(1)})")
        width = k * item
    elif t.dim() == 1 and kind == "scalars":
        if item != 8:
            raise ValueError(f"{who}: a 1-D tensor holds 64-bit scalars (an 8-byte dtype), not {item}-byte elements")
        n, width = int(t.shape[0]), 8
    else:
        raise ValueError(f"{who}: expected a 2-D tensor (n, k)" + (" or a 1-D tensor of an 8-byte dtype" if kind == "scalars" else ""))
    if n <= 0:
        raise ValueError(f"{who}: an empty tensor")
    if kind == "scalars":
        scalar_width_arg(width, montgomery, who)
    elif width != (fe_bytes if compressed else 2 * fe_bytes):
        raise ValueError(f"{who}: rows of {width} bytes, a point is {fe_bytes if compressed else 2 * fe_bytes}")
    stride = int(t.stride(0)) * item if n > 1 else width
    if stride < width or stride % 4 or stride >= 1 << 24:
        raise ValueError(f"{who}: rows {stride} bytes apart (a multiple of 4, at least the width {width}, below 2^24)")
    ptr = int(t.data_ptr())
    if ptr == 0 or ptr % 4:
        raise ValueError(f"{who}: the data must be 4-byte aligned")
    on_gpu = t.device.type == "cuda"
    if t.device.type not in ("cuda", "cpu"):
        raise ValueError(f"{who}: tensor on {t.device}")
    if on_gpu and (t.device.index or 0) not in devices:
        raise ValueError(f"{who}: the tensor is on {t.device}, the context drives GPU(s) {devices}")
    view = {"ptr": ptr, "n": n, "width": width, "stride": stride, "device": on_gpu, "stream": 0,
            "montgomery": bool(montgomery)}
    if is_inf is not None:
        if kind != "points":
            raise ValueError(f"{who}: infinity flags belong to points")
        if (is_inf.dim() != 1 or int(is_inf.shape[0]) < n or is_inf.element_size() != 1 or
                (n > 1 and is_inf.stride(0) != 1) or is_inf.device != t.device):
            raise ValueError(f"{who}: is_inf is a contiguous 1-D tensor of {n} one-byte flags on {t.device}")
        view["is_inf"] = int(is_inf.data_ptr())
    if on_gpu:
        import torch
        view["stream"] = int(torch.cuda.current_stream(t.device).cuda_stream)
    return view


def export_range_args(arr, kind, first, N, who):
    """Entries [first, first + N) of a resident array of `kind` ("scalars" / "points"), N=None: to its end -> (first, N),
    through the range checks every operation over resident arrays shares (_ranges)."""
    if not _is_array(arr, kind):
        raise TypeError(f"{who}: `{kind}` is a resident {kind[:-1]} array")
    return first, _ranges(who, [("first", first, arr)], N, limit=1 << 32 if kind == "scalars" else None)


def export_tensor_view(arr, kind, out, first, N, devices, fe_bytes, montgomery, who, is_inf=None, compressed=False):
    """The arguments of an export into the tensor `out`, checked before anything reaches the device: `out` as tensor_view
    accepts it, the range as export_range_args (N=None: as many entries as `out` has rows), and `out` has a row for every
    entry.  -> the dict of tensor_view with n = N."""
    if not _is_array(arr, kind):
        raise TypeError(f"{who}: `{kind}` is a resident {kind[:-1]} array")
    view = tensor_view(out, devices, kind, fe_bytes, montgomery, who, is_inf, compressed=compressed)
    first, N = export_range_args(arr, kind, first, view["n"] if N is None else N, who)
    if N > view["n"]:
        raise ValueError(f"{who}: {N} entries into a tensor of {view['n']} rows")
    view["n"] = N
    return view


def batch_scalars(scalarsList, N, batch=None):
    """The scalar argument of msmBatch -> ("resident", array, B) or ("host", concatenated bytes, B).  The C ABI takes one
    contiguous scalar set, so a list of separate resident arrays is refused."""
    if N <= 0:
        raise ValueError(f"msmBatch: N = {N}")
    if isinstance(scalarsList, DeviceArray):
        if scalarsList.kind != "scalars":
            raise ValueError("msmBatch: the resident array holds points, not scalars")
        B = len(scalarsList) // N if batch is None else int(batch)
        if B <= 0 or B * N > len(scalarsList):
            raise ValueError(f"msmBatch: {B} vectors of N = {N} scalars need {max(B, 1) * N}, the resident array "
                             f"holds {len(scalarsList)}")
        return "resident", scalarsList, B
    if isinstance(scalarsList, (bytes, bytearray, memoryview, str)) or not hasattr(scalarsList, "__len__"):
        raise TypeError("msmBatch: scalarsList is one resident scalar array or a list of host byte arrays")
    vecs = list(scalarsList)
    if not vecs:
        raise ValueError("msmBatch: no scalar vectors")
    if any(isinstance(v, DeviceArray) for v in vecs):
        raise TypeError("msmBatch: a list of resident arrays is not accepted; pass ONE resident array of B * N "
                        "scalars or a list of host byte arrays")
    vecs = [bytes(v) for v in vecs]
    lens = {len(v) for v in vecs}
    if len(lens) != 1:
        raise ValueError(f"msmBatch: scalar vectors of unequal length {sorted(lens)}")
    if lens.pop() < 32 * N:
        raise ValueError(f"msmBatch: a vector of {len(vecs[0])} bytes holds fewer than N = {N} scalars")
    if batch is not None and int(batch) != len(vecs):
        raise ValueError(f"msmBatch: batch = {batch} but {len(vecs)} vectors were given")
    return "host", b"".join(v[:32 * N] for v in vecs), len(vecs)


def _format_log(log):
    """Same shape as the reference's deferred log lines (msm-common.ts:192-230)."""
    lines = [[{"n_entries": int(log.n_entries), "K": log.K, "c": log.c}]]
    for i, name in enumerate(_native.STAGE_NAMES):
        lines.append([f"{name}... {log.stage_ms[i]:.3f}ms"])
    for r in range(log.rounds):
        if log.batch_add_ms[r] > 0:
            lines.append([f"batch add round {r}: {log.batch_add_ms[r]:.3f}ms"])
    return lines


class _Curve:
    def __init__(self, params, kind):
        if params["kind"] != kind:
            raise ValueError(f"{params['label']} is not a {kind} curve")
        if _state["devices"] is None:
            startThreads()
        self.params = params
        self.kind = kind
        self.fe_bytes = params["fe_bytes"]
        self.default_glv = -1 if kind == "weierstrass" else 0   # -1: GLV below 2^21 points (include/msmz.h)
        ctx = C.c_void_p()
        devs = _state["devices"]
        self.devices = list(devs)
        _check(lib().msmz_create(C.byref(ctx), params["curve_id"], (C.c_int * len(devs))(*devs), len(devs)), "msmz_create")
        self._ctx = ctx
        self.Scalar = _Scalar(self)
        self.Affine = _Affine(self)
        self.Parallel = _Parallel(self)

    def close(self):
        if self._ctx is not None:
            lib().msmz_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def pointAdd(self, a, b):
        """Host-side group addition of two affine results (combining per-GPU partial sums)."""
        fb = self.fe_bytes
        enc = lambda p: int(p["x"]).to_bytes(fb, "little") + int(p["y"]).to_bytes(fb, "little")
        za, zb = bool(a.get("isZero")), bool(b.get("isZero"))
        out = C.create_string_buffer(2 * fb)
        inf = C.c_int()
        _check(lib().msmz_point_add(self.params["curve_id"], None if za else enc(a), int(za), None if zb else enc(b),
                                    int(zb), out, C.byref(inf)), "msmz_point_add")
        return self._point(out.raw, 0, inf.value != 0)

    def _point(self, raw, k, is_zero, zero_rule=True):
        """record k of `raw` (x || y, little-endian) and its infinity flag -> {"x", "y", "isZero"}.  zero_rule: the zero of
        a Weierstrass curve reads (0, 1) (bigint/projective-weierstrass.ts:210 toAffine of zero); a downloaded input set
        keeps the bytes it holds."""
        fb = self.fe_bytes
        x = int.from_bytes(raw[2 * fb * k:2 * fb * k + fb], "little")
        y = int.from_bytes(raw[2 * fb * k + fb:2 * fb * (k + 1)], "little")
        if is_zero and zero_rule and self.kind == "weierstrass":
            x, y = 0, 1
        return {"x": x, "y": y, "isZero": is_zero}


class Weierstrass:
    """`Weierstraß.create(params)` (parallel.ts:33-34, 40-177)."""

    @staticmethod
    def create(params):
        return _Curve(params, "weierstrass")


class TwistedEdwards:
    """`TwistedEdwards.create(params)` (parallel.ts:36-37, 179-289)."""

    @staticmethod
    def create(params):
        return _Curve(params, "twisted-edwards")

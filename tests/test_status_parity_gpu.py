"""Statuses of the resident-set entry points and their precedence, through the C ABI: one bad or boundary call per case
with the status it must return, on a single-engine context and on a two-engine context (both engines on device 0), for
BLS12-377 and ed-on-BLS12-377.  Every bad call is refused on the host before a launch; after it the context still works
(an untouched set downloads its original bytes) and no handle was registered (the next id handed out is the expected
one).  Every valid boundary call (equal starts in place, a distance of exactly n, first = len - n) also has its result
compared with Python integers mod q, or with the points it must reproduce."""
import ctypes as C

import pytest

from msm_zprize_amd import _native as N
from oracle import params as P

pytestmark = pytest.mark.gpu

OK, ARG, UNS, RANGE = 0, 1, 4, 6
CURVE_IDS = {"bls12-377": 0, "ed-on-bls12-377": 3}
LABELS = list(CURVE_IDS)
TOP = (1 << 64) - 1
BIG = (1 << 16) + 8   # two engines: both hold a share
UNKNOWN = 987654


def le(v):
    return int(v).to_bytes(32, "little")


class Ctx:
    """one context, its sets, and a Python model of every scalar set's contents"""

    def __init__(self, label, engines):
        self.L = N.lib()
        self.label, self.G = label, engines
        self.q = P.CURVES[label]["order"]
        self.weier = label != "ed-on-bls12-377"
        ctx = C.c_void_p()
        devs = (C.c_int * engines)(*([0] * engines))
        assert self.L.msmz_create(C.byref(ctx), CURVE_IDS[label], devs, engines) == OK
        self.ctx = ctx
        self.rec = 2 * self.L.msmz_ctx_fe_bytes(ctx)
        self.next_id = 1
        self.model = {}
        q = self.q
        self.keep = self.upload([q - 1 - i for i in range(8)])   # never written
        self.a = self.upload([3 + 5 * i for i in range(8)])
        self.b = self.upload([q - 2 - 7 * i for i in range(8)])
        self.d = self.upload([11 * (i + 1) for i in range(8)])   # destination of the in-place calls
        self.pts = self.random_points(8, 5)
        self.pts2 = self.random_points(8, 6)
        self.pre = 0
        if self.weier:
            st, h = self.precompute(self.pts, 8)
            assert st == OK
            self.pre = self.made(h)
        if engines > 1:
            self.big = self.upload([(i * i + 1) % q for i in range(BIG)])
            self.bigd = self.upload([(7 * i + 2) % q for i in range(BIG)])

    def close(self):
        self.L.msmz_destroy(self.ctx)

    def made(self, h):
        assert h == self.next_id, (h, self.next_id)
        self.next_id += 1
        return h

    def upload(self, values):
        h = C.c_uint64(0)
        assert self.L.msmz_upload_scalars(self.ctx, b"".join(le(v) for v in values), len(values), C.byref(h)) == OK
        self.model[h.value] = list(values)
        return self.made(h.value)

    def random_points(self, n, seed):
        h = C.c_uint64(0)
        assert self.L.msmz_random_points(self.ctx, n, seed, C.byref(h)) == OK
        return self.made(h.value)

    def precompute(self, ph, n):
        o = N.MsmzOpts()
        o.glv, o.c = 0, 7
        h = C.c_uint64(0)
        return self.L.msmz_precompute_points(self.ctx, ph, n, C.byref(o), 2, C.byref(h)), h.value

    def scalars(self, h, first, count):
        buf = C.create_string_buffer(32 * max(count, 1))
        st = self.L.msmz_download_scalars(self.ctx, h, first, count, buf)
        raw = buf.raw
        return st, [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(count)]

    def points(self, h, first, count):
        buf = C.create_string_buffer(self.rec * max(count, 1))
        inf = C.create_string_buffer(max(count, 1))
        return self.L.msmz_download_points(self.ctx, h, first, count, buf, inf), buf.raw[:self.rec * count]

    def intact(self):
        """after a refused call: the untouched set reads back, and the next handle id is the one expected"""
        st, got = self.scalars(self.keep, 0, 8)
        assert st == OK and got == self.model[self.keep]
        h = C.c_uint64(0)
        assert self.L.msmz_random_scalars(self.ctx, 1, 1, C.byref(h)) == OK
        assert self.L.msmz_free(self.ctx, self.made(h.value)) == OK

    def agrees(self, h):
        st, got = self.scalars(h, 0, len(self.model[h]))
        assert st == OK and got == self.model[h]

    # ---- the entry points: (status, ...) with *out_handle as the call left it
    def combine(self, x, y, n, first_out=0, out=0):
        """x, y: (handle, first, coeff_handle, coeff_first, coeff int or None)"""
        t = [N.MsmzScalarTerm(v[0], v[1], v[2], v[3], None if v[4] is None else le(v[4])) if v else None for v in (x, y)]
        h = C.c_uint64(out)
        st = self.L.msmz_scalars_combine(self.ctx, C.byref(t[0]), C.byref(t[1]) if t[1] else None, n, first_out, C.byref(h))
        return st, h.value

    def dot(self, xh, fx, yh, fy, n):
        out = C.create_string_buffer(b"\xaa" * 32, 32)
        st = self.L.msmz_scalars_dot(self.ctx, xh, fx, yh, fy, n, out)
        return st, int.from_bytes(out.raw, "little")

    def powers(self, base, ratio, n):
        h = C.c_uint64(0)
        st = self.L.msmz_scalars_powers(self.ctx, None if base is None else le(base), None if ratio is None else le(ratio),
                                        n, C.byref(h))
        return st, h.value

    def recur(self, n, a_handle=0, a_first=0, a=None, b_handle=0, b_first=0, init=None, flags=0, first_out=0, out=0):
        r = N.MsmzScalarRec(a_handle, a_first, None if a is None else le(a), b_handle, b_first,
                            None if init is None else le(init), flags)
        h = C.c_uint64(out)
        last = C.create_string_buffer(b"\xaa" * 32, 32)
        st = self.L.msmz_scalars_recurrence(self.ctx, C.byref(r), n, first_out, C.byref(h), last)
        return st, h.value, int.from_bytes(last.raw, "little")

    def inverse(self, h, first, n, first_out=0, out=0):
        oh = C.c_uint64(out)
        zeros = C.c_uint64(1 << 40)
        st = self.L.msmz_scalars_inverse(self.ctx, h, first, n, first_out, C.byref(oh), C.byref(zeros))
        return st, oh.value, zeros.value

    def mul(self, n, ph, fp=0, sh=0, fs=0, scalar=None, qh=0, fq=0):
        m = N.MsmzMul(ph, fp, sh, fs, None if scalar is None else le(scalar), qh, fq)
        h = C.c_uint64(0)
        st = self.L.msmz_points_mul(self.ctx, C.byref(m), n, C.byref(h))
        return st, h.value

    def check(self, ph, first, count, what=N.MSMZ_CHECK_CURVE):
        res = N.MsmzCheckResult(77, 77, 77)
        st = self.L.msmz_check_points(self.ctx, ph, first, count, what, C.byref(res), None)
        return st, (res.off_curve, res.off_subgroup, res.first_bad)

    def into(self, h, first, values, n):
        data = C.create_string_buffer(b"".join(le(v) for v in values), 32 * len(values))
        src = N.MsmzSrc(C.cast(data, C.c_void_p), 0, 32, 0, None, None)
        return self.L.msmz_import_scalars_into(self.ctx, h, first, C.byref(src), n)

    def segments(self, ph, sh, segs):
        arr = (N.MsmzSegment * len(segs))(*[N.MsmzSegment(*s) for s in segs])
        out = C.create_string_buffer(self.rec * len(segs))
        inf = (C.c_int * len(segs))()
        st = self.L.msmz_msm_segments(self.ctx, ph, sh, arr, len(segs), None, out, inf, None)
        return st, out.raw, list(inf)

    def resident_msm(self, ph, sh, n, batch=1):
        out = C.create_string_buffer(self.rec * batch)
        inf = (C.c_int * batch)()
        return self.L.msmz_msm_batch_resident(self.ctx, ph, sh, n, batch, None, out, inf, None)


@pytest.fixture(scope="module")
def contexts():
    cache = {}

    def get(label, engines):
        if (label, engines) not in cache:
            cache[(label, engines)] = Ctx(label, engines)
        return cache[(label, engines)]

    yield get
    for c in cache.values():
        c.close()


def term(h, first=0, ch=0, cfirst=0, coeff=None):
    return (h, first, ch, cfirst, coeff)


# ------------------------------------------------------------------------------------------------ refused calls
# (id, call(c) -> status or a tuple starting with it, expected status, Weierstrass only)
REFUSED_ONE = [
    # scalars_combine: handles and ranges (ARG) before a broadcast coefficient >= q (RANGE)
    ("combine-unknown", lambda c: c.combine(term(UNKNOWN), None, 8), ARG, False),
    ("combine-points-as-x", lambda c: c.combine(term(c.pts), None, 8), ARG, False),
    ("combine-n0", lambda c: c.combine(term(c.a), None, 0), ARG, False),
    ("combine-n-2^32", lambda c: c.combine(term(c.a), None, 1 << 32), ARG, False),
    ("combine-beyond", lambda c: c.combine(term(c.a, 1), None, 8), ARG, False),
    ("combine-first-len-n1", lambda c: c.combine(term(c.a, 8), None, 1), ARG, False),
    ("combine-first-len+1", lambda c: c.combine(term(c.a, 9), None, 1), ARG, False),
    ("combine-wrap", lambda c: c.combine(term(c.a, TOP), None, 2), ARG, False),
    ("combine-coeff-set-beyond", lambda c: c.combine(term(c.a, 0, c.b, 6), None, 3), ARG, False),
    ("combine-coeff-set-points", lambda c: c.combine(term(c.a, 0, c.pts, 0), None, 3), ARG, False),
    ("combine-beyond-and-coeff-q", lambda c: c.combine(term(c.a, 6, 0, 0, c.q), None, 3), ARG, False),
    ("combine-y-beyond-x-coeff-q", lambda c: c.combine(term(c.a, 0, 0, 0, c.q), term(c.b, 7), 2), ARG, False),
    ("combine-dest-beyond-coeff-q", lambda c: c.combine(term(c.a, 0, 0, 0, c.q), None, 3, 6, c.d), ARG, False),
    ("combine-coeff-q", lambda c: c.combine(term(c.a, 0, 0, 0, c.q), None, 3), RANGE, False),
    ("combine-y-coeff-top", lambda c: c.combine(term(c.a), term(c.b, 0, 0, 0, (1 << 256) - 1), 3), RANGE, False),
    ("combine-fresh-first-out", lambda c: c.combine(term(c.a), None, 3, 1, 0), ARG, False),
    ("combine-dest-unknown", lambda c: c.combine(term(c.a), None, 3, 0, UNKNOWN), ARG, False),
    ("combine-dest-points", lambda c: c.combine(term(c.a), None, 3, 0, c.pts), ARG, False),
    ("combine-dest-beyond", lambda c: c.combine(term(c.a), None, 3, 6, c.d), ARG, False),
    # scalars_dot
    ("dot-first-y-without-y", lambda c: c.dot(c.a, 0, 0, 1, 4), ARG, False),
    ("dot-x-unknown", lambda c: c.dot(UNKNOWN, 0, 0, 0, 4), ARG, False),
    ("dot-y-points", lambda c: c.dot(c.a, 0, c.pts, 0, 4), ARG, False),
    ("dot-n0", lambda c: c.dot(c.a, 0, c.b, 0, 0), ARG, False),
    ("dot-n-2^32", lambda c: c.dot(c.a, 0, c.b, 0, 1 << 32), ARG, False),
    ("dot-x-beyond", lambda c: c.dot(c.a, 5, c.b, 0, 4), ARG, False),
    ("dot-y-beyond", lambda c: c.dot(c.a, 0, c.b, 8, 1), ARG, False),
    ("dot-wrap", lambda c: c.dot(c.a, TOP, c.b, 0, 2), ARG, False),
    # scalars_powers: ARG first
    ("powers-no-ratio", lambda c: c.powers(1, None, 4), ARG, False),
    ("powers-n0-ratio-q", lambda c: c.powers(1, c.q, 0), ARG, False),
    ("powers-n-2^32-base-q", lambda c: c.powers(c.q, 2, 1 << 32), ARG, False),
    ("powers-ratio-q", lambda c: c.powers(None, c.q, 4), RANGE, False),
    ("powers-base-q", lambda c: c.powers(c.q, 2, 4), RANGE, False),
    # scalars_recurrence: ARG before RANGE
    ("rec-flags", lambda c: c.recur(4, a_handle=c.a, flags=4), ARG, False),
    ("rec-nothing", lambda c: c.recur(4), ARG, False),
    ("rec-n0", lambda c: c.recur(0, a_handle=c.a), ARG, False),
    ("rec-n-2^32", lambda c: c.recur(1 << 32, a_handle=c.a), ARG, False),
    # scalars_inverse
    ("inv-unknown", lambda c: c.inverse(UNKNOWN, 0, 4), ARG, False),
    ("inv-points", lambda c: c.inverse(c.pts, 0, 4), ARG, False),
    ("inv-n0", lambda c: c.inverse(c.a, 0, 0), ARG, False),
    ("inv-beyond", lambda c: c.inverse(c.a, 5, 4), ARG, False),
    ("inv-wrap", lambda c: c.inverse(c.a, TOP, 2), ARG, False),
    ("inv-fresh-first-out", lambda c: c.inverse(c.a, 0, 4, 1, 0), ARG, False),
    ("inv-dest-unknown", lambda c: c.inverse(c.a, 0, 4, 0, UNKNOWN), ARG, False),
    ("inv-dest-beyond", lambda c: c.inverse(c.a, 0, 4, 5, c.d), ARG, False),
    ("inv-overlap-1", lambda c: c.inverse(c.d, 0, 3, 1, c.d), ARG, False),
    ("inv-overlap-n-1", lambda c: c.inverse(c.d, 2, 3, 0, c.d), ARG, False),
    # points_mul: unknown / wrong kind, then a precomputed set, then the ranges, then the broadcast scalar
    ("mul-p-unknown", lambda c: c.mul(3, UNKNOWN, scalar=1), ARG, False),
    ("mul-p-scalars", lambda c: c.mul(3, c.a, scalar=1), ARG, False),
    ("mul-q-unknown", lambda c: c.mul(3, c.pts, scalar=1, qh=UNKNOWN), ARG, False),
    ("mul-s-points", lambda c: c.mul(3, c.pts, sh=c.pts2), ARG, False),
    ("mul-no-scalar", lambda c: c.mul(3, c.pts), ARG, False),
    ("mul-n0", lambda c: c.mul(0, c.pts, scalar=1), ARG, False),
    ("mul-pre-p-unknown-q", lambda c: c.mul(3, c.pre, scalar=1, qh=UNKNOWN), ARG, True),
    ("mul-pre-p", lambda c: c.mul(3, c.pre, scalar=1), UNS, True),
    ("mul-pre-q", lambda c: c.mul(3, c.pts, scalar=1, qh=c.pre), UNS, True),
    ("mul-pre-p-beyond", lambda c: c.mul(3, c.pre, 7, scalar=1), UNS, True),
    ("mul-pre-q-s-beyond-scalar", lambda c: c.mul(3, c.pts, 6, sh=c.a, fs=6, qh=c.pre), UNS, True),
    ("mul-pre-p-scalar-q", lambda c: c.mul(3, c.pre, scalar=c.q), UNS, True),
    ("mul-p-beyond", lambda c: c.mul(3, c.pts, 6, scalar=1), ARG, False),
    ("mul-q-beyond", lambda c: c.mul(3, c.pts, 0, scalar=1, qh=c.pts2, fq=8), ARG, False),
    ("mul-s-beyond", lambda c: c.mul(3, c.pts, 0, sh=c.a, fs=6), ARG, False),
    ("mul-wrap", lambda c: c.mul(2, c.pts, TOP, scalar=1), ARG, False),
    ("mul-beyond-scalar-q", lambda c: c.mul(3, c.pts, 6, scalar=c.q), ARG, False),
    ("mul-scalar-q", lambda c: c.mul(3, c.pts, 0, scalar=c.q), RANGE, False),
    # check_points: what / count, kind, a precomputed set, the range
    ("check-what-0", lambda c: c.check(c.pts, 0, 3, 0), ARG, False),
    ("check-what-4", lambda c: c.check(c.pts, 0, 3, 4), ARG, False),
    ("check-count-0", lambda c: c.check(c.pts, 0, 0), ARG, False),
    ("check-unknown", lambda c: c.check(UNKNOWN, 0, 3), ARG, False),
    ("check-scalars", lambda c: c.check(c.a, 0, 3), ARG, False),
    ("check-pre-what-0", lambda c: c.check(c.pre, 0, 3, 0), ARG, True),
    ("check-pre", lambda c: c.check(c.pre, 0, 3), UNS, True),
    ("check-pre-beyond", lambda c: c.check(c.pre, 7, 3), UNS, True),
    ("check-beyond", lambda c: c.check(c.pts, 6, 3), ARG, False),
    ("check-first-len", lambda c: c.check(c.pts, 8, 1), ARG, False),
    ("check-wrap", lambda c: c.check(c.pts, TOP, 2), ARG, False),
    # downloads and free
    ("download-scalars-beyond", lambda c: c.scalars(c.a, 6, 3), ARG, False),
    ("download-scalars-first-len+1", lambda c: c.scalars(c.a, 9, 0), ARG, False),
    ("download-scalars-wrap", lambda c: c.scalars(c.a, TOP, 2), ARG, False),
    ("download-scalars-points", lambda c: c.scalars(c.pts, 0, 1), ARG, False),
    ("download-points-scalars", lambda c: c.points(c.a, 0, 1), ARG, False),
    ("download-points-wrap", lambda c: c.points(c.pts, TOP, 2), ARG, False),
    ("free-unknown", lambda c: c.L.msmz_free(c.ctx, UNKNOWN), ARG, False),
    # MSMs over resident sets
    ("msm-points-unknown", lambda c: c.resident_msm(UNKNOWN, c.a, 8), ARG, False),
    ("msm-n-above", lambda c: c.resident_msm(c.pts, c.a, 9), ARG, False),
    ("msm-scalars-points", lambda c: c.resident_msm(c.pts, c.pts2, 8), ARG, False),
    ("msm-batch-above", lambda c: c.resident_msm(c.pts, c.a, 8, 2), ARG, False),
]

SINGLE_ONLY = [
    ("combine-overlap-1", lambda c: c.combine(term(c.d, 0), None, 3, 1, c.d), ARG, False),
    ("combine-overlap-n-1", lambda c: c.combine(term(c.d, 0), None, 3, 2, c.d), ARG, False),
    ("combine-overlap-behind", lambda c: c.combine(term(c.d, 4), None, 3, 2, c.d), ARG, False),
    ("combine-coeff-set-overlap", lambda c: c.combine(term(c.a, 0, c.d, 1), None, 3, 0, c.d), ARG, False),
    ("combine-y-overlap", lambda c: c.combine(term(c.a), term(c.d, 3), 4, 0, c.d), ARG, False),
    ("rec-fresh-first-out", lambda c: c.recur(4, a_handle=c.a, first_out=1), ARG, False),
    ("rec-a-unknown", lambda c: c.recur(4, a_handle=UNKNOWN), ARG, False),
    ("rec-b-points", lambda c: c.recur(4, b_handle=c.pts), ARG, False),
    ("rec-a-beyond-init-q", lambda c: c.recur(4, a_handle=c.a, a_first=5, init=c.q), ARG, False),
    ("rec-b-beyond-a-q", lambda c: c.recur(4, a=c.q, b_handle=c.b, b_first=5), ARG, False),
    ("rec-wrap", lambda c: c.recur(2, b_handle=c.b, b_first=TOP), ARG, False),
    ("rec-dest-beyond-a-q", lambda c: c.recur(4, a=c.q, b_handle=c.b, first_out=5, out=c.d), ARG, False),
    ("rec-dest-unknown", lambda c: c.recur(4, b_handle=c.b, out=UNKNOWN), ARG, False),
    ("rec-a-q", lambda c: c.recur(4, a=c.q, b_handle=c.b), RANGE, False),
    ("rec-init-q", lambda c: c.recur(4, a_handle=c.a, init=c.q), RANGE, False),
    ("rec-overlap-1", lambda c: c.recur(3, b_handle=c.d, b_first=0, first_out=1, out=c.d), ARG, False),
    ("rec-overlap-n-1", lambda c: c.recur(3, a_handle=c.d, a_first=4, first_out=2, out=c.d), ARG, False),
    ("download-points-beyond-images", lambda c: c.points(c.pts, 0, 17 if c.weier else 9), ARG, False),
    ("into-unknown", lambda c: c.into(UNKNOWN, 0, [1, 2], 2), ARG, False),
    ("into-points", lambda c: c.into(c.pts, 0, [1, 2], 2), ARG, False),
    ("into-n0", lambda c: c.into(c.d, 0, [1, 2], 0), ARG, False),
    ("into-beyond", lambda c: c.into(c.d, 7, [1, 2], 2), ARG, False),
    ("into-wrap", lambda c: c.into(c.d, TOP, [1, 2], 2), ARG, False),
    ("segments-points-unknown", lambda c: c.segments(UNKNOWN, c.a, [(0, 0, 3)]), ARG, False),
    ("segments-scalars-points", lambda c: c.segments(c.pts, c.pts2, [(0, 0, 3)]), ARG, False),
    ("segments-n0", lambda c: c.segments(c.pts, c.a, [(0, 0, 3), (0, 0, 0)]), ARG, False),
    ("segments-points-beyond", lambda c: c.segments(c.pts, c.a, [(0, 0, 3), (6, 0, 3)]), ARG, False),
    ("segments-scalars-beyond", lambda c: c.segments(c.pts, c.a, [(0, 8, 1)]), ARG, False),
    ("segments-wrap", lambda c: c.segments(c.pts, c.a, [(TOP, 0, 2)]), ARG, False),
    ("precompute-unknown", lambda c: c.precompute(UNKNOWN, 8)[0], ARG, True),
    ("precompute-n-above", lambda c: c.precompute(c.pts, 9)[0], ARG, True),
    ("precompute-twice", lambda c: c.precompute(c.pre, 8)[0], ARG, True),
]

# a two-engine context: a range beyond the set is ARG even when it is also shifted; a valid shifted range is UNSUPPORTED
MULTI_ONLY = [
    ("multi-combine-shifted", lambda c: c.combine(term(c.a, 1), None, 3), UNS, False),
    ("multi-combine-beyond-and-shifted", lambda c: c.combine(term(c.a, 1), None, 8), ARG, False),
    ("multi-combine-coeff-set-shifted", lambda c: c.combine(term(c.a, 0, c.b, 2), None, 3), UNS, False),
    ("multi-combine-first-out", lambda c: c.combine(term(c.a), None, 3, 2, c.d), UNS, False),
    ("multi-combine-dest-longer", lambda c: c.combine(term(c.a), None, 4, 0, c.d), UNS, False),
    ("multi-combine-dest-longer-big", lambda c: c.combine(term(c.big), None, 1 << 16, 0, c.bigd), UNS, False),
    ("multi-combine-overlap-shifted", lambda c: c.combine(term(c.d, 0), None, 3, 1, c.d), UNS, False),
    ("multi-combine-shifted-coeff-q", lambda c: c.combine(term(c.a, 1, 0, 0, c.q), None, 3), UNS, False),
    ("multi-dot-shifted", lambda c: c.dot(c.a, 1, c.b, 0, 3), UNS, False),
    ("multi-dot-y-shifted", lambda c: c.dot(c.big, 0, c.bigd, 8, 1 << 16), UNS, False),
    ("multi-dot-beyond-and-shifted", lambda c: c.dot(c.a, 1, c.b, 0, 8), ARG, False),
    ("multi-inv-shifted", lambda c: c.inverse(c.a, 4, 4), UNS, False),
    ("multi-inv-first-out", lambda c: c.inverse(c.a, 0, 4, 4, c.d), UNS, False),
    ("multi-inv-dest-longer", lambda c: c.inverse(c.a, 0, 4, 0, c.d), UNS, False),
    ("multi-inv-distance-n", lambda c: c.inverse(c.d, 0, 4, 4, c.d), UNS, False),
    ("multi-inv-beyond-and-shifted", lambda c: c.inverse(c.a, 5, 4), ARG, False),
    ("multi-rec-valid", lambda c: c.recur(8, b_handle=c.b), UNS, False),
    ("multi-rec-unknown-handles", lambda c: c.recur(8, a_handle=UNKNOWN, b_handle=UNKNOWN, b_first=TOP, out=UNKNOWN), UNS, False),
    ("multi-rec-a-q", lambda c: c.recur(8, a=c.q, b_handle=c.b), UNS, False),
    ("multi-rec-flags-unknown", lambda c: c.recur(8, a_handle=UNKNOWN, flags=8), ARG, False),
    ("multi-rec-nothing", lambda c: c.recur(8), ARG, False),
    ("multi-rec-n0", lambda c: c.recur(0, b_handle=c.b), ARG, False),
    ("multi-into-valid", lambda c: c.into(c.d, 0, [1, 2], 2), UNS, False),
    ("multi-into-unknown-beyond", lambda c: c.into(UNKNOWN, TOP, [1, 2], 2), UNS, False),
    ("multi-segments-valid", lambda c: c.segments(c.pts, c.a, [(0, 0, 3)]), UNS, False),
    ("multi-segments-unknown-beyond", lambda c: c.segments(UNKNOWN, c.pts, [(TOP, 9, 0)]), UNS, False),
    ("multi-mul-shifted", lambda c: c.mul(3, c.pts, 5, scalar=1), UNS, False),
    ("multi-mul-s-shifted", lambda c: c.mul(3, c.pts, 0, sh=c.a, fs=5), UNS, False),
    ("multi-mul-beyond-and-shifted", lambda c: c.mul(3, c.pts, 6, scalar=1), ARG, False),
    ("multi-mul-pre-shifted", lambda c: c.mul(3, c.pre, 5, scalar=1), UNS, True),
    ("multi-mul-shifted-scalar-q", lambda c: c.mul(3, c.pts, 5, scalar=c.q), UNS, False),
    ("multi-alloc", lambda c: c.L.msmz_alloc_scalars(c.ctx, 8, C.byref(C.c_uint64())), UNS, False),
]


def _cases(table):
    """(label, case) for both curves; the cases about a precomputed set for the Weierstrass curve only"""
    return [pytest.param(label, t, id=f"{label}-{t[0]}") for label in LABELS for t in table
            if not (t[3] and label == "ed-on-bls12-377")]


def _refused(c, call, want):
    before = {h: c.scalars(h, 0, 8)[1] for h in (c.a, c.b, c.d)}
    got = call(c)
    st = got if isinstance(got, int) else got[0]
    assert st == want, got
    c.intact()
    assert {h: c.scalars(h, 0, 8)[1] for h in before} == before


@pytest.mark.parametrize("label,case", _cases(REFUSED_ONE + SINGLE_ONLY))
def test_refused_single_engine(contexts, label, case):
    _refused(contexts(label, 1), case[1], case[2])


@pytest.mark.parametrize("label,case", _cases(REFUSED_ONE + MULTI_ONLY))
def test_refused_two_engines(contexts, label, case):
    _refused(contexts(label, 2), case[1], case[2])


@pytest.mark.parametrize("engines", [1, 2])
@pytest.mark.parametrize("label", LABELS)
def test_refused_calls_leave_out_handle(contexts, label, engines):
    """a refused call leaves *out_handle as it was: 0 for a fresh output, the caller's handle for an in-place one"""
    c = contexts(label, engines)
    assert c.combine(term(c.a, 7), None, 3) == (ARG, 0)
    assert c.combine(term(c.a, 0, 0, 0, c.q), None, 8, 0, c.d) == (RANGE, c.d)
    assert c.combine(term(c.a), None, 3, 7, c.d) == (ARG, c.d)
    assert c.inverse(c.a, 7, 3)[:2] == (ARG, 0)
    assert c.inverse(c.a, 0, 3, 7, c.d)[:2] == (ARG, c.d)
    assert c.recur(3, b_handle=c.b, b_first=7)[:2] == (ARG if engines == 1 else UNS, 0)
    assert c.recur(3, b_handle=c.b, first_out=7, out=c.d)[:2] == (ARG if engines == 1 else UNS, c.d)
    assert c.mul(3, c.pts, 7, scalar=1) == (ARG, 0)
    assert c.powers(1, c.q, 3) == (RANGE, 0)
    c.intact()
    c.agrees(c.d)


# ------------------------------------------------------------------------------------------------ valid boundaries
def _lin(q, xs, k=1, ys=None, m=1):
    return [(k * x + (m * y if ys is not None else 0)) % q for x, y in zip(xs, ys if ys is not None else xs)]


@pytest.mark.parametrize("label", LABELS)
def test_valid_boundaries_single_engine(contexts, label):
    """first = len - n, equal starts in place, and a distance of exactly n (both orders), with the results"""
    c = contexts(label, 1)
    q, A, B = c.q, c.model[c.a], c.model[c.b]
    # combine: fresh from the last three records; first = len with n = 0 is refused (n = 0), a download of it is not
    st, h = c.combine(term(c.a, 5, 0, 0, 3), term(c.b, 5, c.a, 5), 3)
    assert st == OK
    c.model[c.made(h)] = [(3 * x + x * y) % q for x, y in zip(A[5:], B[5:])]
    c.agrees(h)
    assert c.scalars(c.a, 8, 0) == (OK, [])
    # in place, equal starts; then source and destination exactly n apart, in both orders
    D = c.model[c.d]
    assert c.combine(term(c.d, 2, 0, 0, 5), None, 3, 2, c.d) == (OK, c.d)
    D[2:5] = _lin(q, D[2:5], 5)
    c.agrees(c.d)
    assert c.combine(term(c.d, 0), term(c.d, 6, 0, 0, q - 1), 2, 2, c.d) == (OK, c.d)   # distances 2 = n and 4
    D[2:4] = [(x - y) % q for x, y in zip(D[0:2], D[6:8])]
    c.agrees(c.d)
    assert c.combine(term(c.d, 5), None, 3, 2, c.d) == (OK, c.d)                        # the source behind, n apart
    D[2:5] = D[5:8]
    c.agrees(c.d)
    assert c.combine(term(c.a, 0, c.d, 5), None, 3, 5, c.d) == (OK, c.d)                # the coefficient set in place
    D[5:8] = [x * y % q for x, y in zip(A[0:3], D[5:8])]
    c.agrees(c.d)
    # dot over the last records
    assert c.dot(c.a, 4, c.b, 4, 4) == (OK, sum(x * y for x, y in zip(A[4:], B[4:])) % q)
    assert c.dot(c.a, 7, 0, 0, 1) == (OK, A[7])
    # recurrence (prefix sums of b): fresh from first = len - n; in place at equal starts; n apart
    sums = lambda v: [sum(v[:i + 1]) % q for i in range(len(v))]
    st, h, last = c.recur(3, b_handle=c.b, b_first=5)
    assert (st, last) == (OK, sums(B[5:])[-1])
    c.model[c.made(h)] = sums(B[5:])
    c.agrees(h)
    st, h, last = c.recur(4, b_handle=c.d, b_first=4, first_out=4, out=c.d)
    D[4:8] = sums(D[4:8])
    assert (st, h, last) == (OK, c.d, D[7])
    c.agrees(c.d)
    st, h, last = c.recur(4, a=2, b_handle=c.d, b_first=4, init=1, first_out=0, out=c.d)   # y_i = 2 y_(i-1) + b_i
    y, out = 1, []
    for b in D[4:8]:
        y = (2 * y + b) % q
        out.append(y)
    D[0:4] = out
    assert (st, h, last) == (OK, c.d, out[-1])
    c.agrees(c.d)
    # inverse: first = len - n fresh; in place at equal starts; n apart
    inv = lambda v: [pow(x, -1, q) if x else 0 for x in v]
    st, h, zeros = c.inverse(c.a, 5, 3)
    assert (st, zeros) == (OK, 0)
    c.model[c.made(h)] = inv(A[5:])
    c.agrees(h)
    assert c.inverse(c.d, 0, 4, 0, c.d) == (OK, c.d, D[0:4].count(0))
    D[0:4] = inv(D[0:4])
    c.agrees(c.d)
    assert c.inverse(c.d, 4, 4, 0, c.d) == (OK, c.d, D[4:8].count(0))
    D[0:4] = inv(D[4:8])
    c.agrees(c.d)
    # import into the last records
    assert c.into(c.d, 6, [q - 1, 9], 2) == OK
    D[6:8] = [q - 1, 9]
    c.agrees(c.d)
    # points: [1] P over the last three records reproduces them; the check accepts them; a segment over them = their sum
    # and [s_i] P_i + Q_i = ([s_i] P_i) + Q_i, all three ranges at first = len - n
    want = c.points(c.pts, 5, 3)
    st, h = c.mul(3, c.pts, 5, scalar=1)
    assert st == OK and c.points(c.made(h), 0, 3) == want and want[0] == OK
    assert c.check(c.pts, 5, 3, 3) == (OK, (0, 0, TOP))
    st, prod = c.mul(3, c.pts, 5, sh=c.a, fs=5)
    assert st == OK
    recs = c.points(c.made(prod), 0, 3)[1]
    st, both = c.mul(3, c.pts, 5, sh=c.a, fs=5, qh=c.pts2, fq=5)
    assert st == OK
    sums = c.points(c.made(both), 0, 3)[1]
    addend = c.points(c.pts2, 5, 3)[1]
    rec = lambda raw, k: raw[k * c.rec:(k + 1) * c.rec]

    def add(p1, p2):
        out, inf = C.create_string_buffer(c.rec), C.c_int(0)
        assert c.L.msmz_point_add(CURVE_IDS[label], p1, 0, p2, 0, out, C.byref(inf)) == OK and inf.value == 0
        return out.raw

    assert [add(rec(recs, k), rec(addend, k)) for k in range(3)] == [rec(sums, k) for k in range(3)]
    st, out, inf = c.segments(c.pts, c.a, [(5, 5, 3)])
    assert (st, out, inf) == (OK, add(add(rec(recs, 0), rec(recs, 1)), rec(recs, 2)), [0])
    c.intact()


@pytest.mark.parametrize("which", ["small", "big"])
@pytest.mark.parametrize("label", LABELS)
def test_valid_in_place_two_engines(contexts, label, which):
    """whole sets from 0 are the calls a two-engine context takes: in place at equal starts, and the results, with one
    engine holding everything (8 records) and with both holding a share"""
    c = contexts(label, 2)
    q = c.q
    src, dst = (c.a, c.d) if which == "small" else (c.big, c.bigd)
    X, D = c.model[src], c.model[dst]
    n = len(X)
    assert c.combine(term(src, 0, 0, 0, 3), term(dst, 0, src, 0), n, 0, dst) == (OK, dst)
    D[:] = [(3 * x + x * d) % q for x, d in zip(X, D)]
    c.agrees(dst)
    assert c.dot(src, 0, dst, 0, n) == (OK, sum(x * d for x, d in zip(X, D)) % q)
    assert c.inverse(dst, 0, n, 0, dst) == (OK, dst, D.count(0))
    st, got = c.scalars(dst, 0, n)   # (the inverse mod q is unique: x * y = 1 pins y, and costs no Python inversion)
    assert st == OK and all(x * y % q == 1 if x else y == 0 for x, y in zip(D, got))
    D[:] = got
    c.intact()


@pytest.mark.parametrize("label", LABELS)
def test_valid_fresh_two_engines(contexts, label):
    """a prefix of a longer set into a fresh one, powers over both shares, [1] P, a shifted check and a shifted download"""
    c = contexts(label, 2)
    q = c.q
    st, h = c.combine(term(c.big, 0, 0, 0, 2), None, 1 << 16)
    assert st == OK
    c.model[c.made(h)] = [2 * x % q for x in c.model[c.big][:1 << 16]]
    c.agrees(h)
    st, h = c.powers(5, 3, BIG)
    assert st == OK
    pw, v = [], 5
    for _ in range(BIG):
        pw.append(v)
        v = v * 3 % q
    c.model[c.made(h)] = pw
    c.agrees(h)
    want = c.points(c.pts, 0, 8)
    st, h = c.mul(8, c.pts, 0, scalar=1)
    assert st == OK and c.points(c.made(h), 0, 8) == want
    assert c.check(c.pts, 5, 3, 3) == (OK, (0, 0, TOP))   # (a shifted range is fine here: every engine checks its share)
    assert c.scalars(c.big, BIG - 3, 3) == (OK, c.model[c.big][-3:])
    c.intact()

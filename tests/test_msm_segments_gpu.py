"""Segmented MSM (msmz_msm_segments): every problem its own range of one resident point set and one resident scalar set.
Every result is compared bit-exactly, per segment, against the C oracle on the sliced bigints (computed once per
(curve, scalar set, segment) and shared), and where noted against msm / msmBatch of the existing API.  The counters of
msmz_test_passes prove which path ran: one batched pipeline per sub-batch of a length class, or the range loop.

Sizes: a sort tile is 2048 half-scalars (2048 scalars, 1024 with GLV), so the class {2048, 2049, 3000, 4095} has tiles
wholly past a segment's end, a ragged last tile, and more than one workgroup per problem, on either tile size."""
import ctypes as C
import random
from contextlib import contextmanager

import pytest

from oracle import c_oracle
from oracle import params as P

pytestmark = pytest.mark.gpu

WEIER = ["bls12-377", "pallas", "bls12-381"]
MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
NP, NS = 6000, 6200   # points / scalars of the shared sets
# one length class, unaligned non-zero offsets, the last two ending exactly at the end of the point / scalar set
CLASS = [(1500, 700, 2048), (37, 3, 2049), (2999, 3100, 3000), (1905, 2105, 4095)]


@pytest.fixture(scope="module")
def mod():
    import msm_zprize_amd as m
    m.startThreads()
    return m


def _create(mod, label):
    params = mod.curves.BY_LABEL[label]
    return (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)


def _enc(scalars):
    return b"".join(int(s).to_bytes(32, "little") for s in scalars)


def _pt(label, p):
    """a result as (x, y, infinity flag); twisted Edwards results carry no flag: the identity is (0, 1)"""
    return (p["x"], p["y"], bool(p.get("isZero", False)) and label in WEIER)


class Data:
    """per curve: NP points, NS scalars below q and NS scalars below 2^64, resident and as bigints; the oracle's results"""

    def __init__(self, mod, label):
        self.label, self.curve = label, _create(mod, label)
        self.q = P.CURVES[label]["order"]
        rng = random.Random(sorted(P.CURVES).index(label) + 31)
        self.pts = self.curve.Parallel.randomPointsFast(NP, 4242)
        self.big = self.curve.Affine.toBigints(self.pts)
        self.s = {"full": [rng.randrange(self.q) for _ in range(NS)], "u64": [rng.randrange(1 << 64) for _ in range(NS)]}
        self.sc = {k: self.curve.Parallel.scalarsFromBytes(_enc(v), NS) for k, v in self.s.items()}
        self._want = {}

    def want(self, seg, which="full"):
        key = (which, tuple(seg))
        if key not in self._want:
            fp, fs, n = seg
            self._want[key] = _pt(self.label, c_oracle.msm(P.CURVES[self.label], self.s[which][fs:fs + n], self.big[fp:fp + n]))
        return self._want[key]


@pytest.fixture(scope="module")
def data(mod):
    cache = {}

    def get(label):
        if label not in cache:
            cache[label] = Data(mod, label)
        return cache[label]

    yield get
    for d in cache.values():
        d.curve.close()


def passes(curve):
    """(range passes, batched pipelines) the context ran so far"""
    from msm_zprize_amd._native import lib
    rp, sb = C.c_uint64(), C.c_uint64()
    assert lib().msmz_test_passes(curve._ctx, C.byref(rp), C.byref(sb)) == 0
    return rp.value, sb.value


@contextmanager
def limits(curve, pass_entries=0, batch_entries=0):
    from msm_zprize_amd._native import lib
    assert lib().msmz_test_set_limits(curve._ctx, pass_entries, batch_entries) == 0
    try:
        yield
    finally:
        assert lib().msmz_test_set_limits(curve._ctx, 0, 0) == 0


def _opts(glv=-1, safe=1, c=0, buckets=0, bits=0, reduce_affine=0):
    from msm_zprize_amd._native import MsmzOpts
    o = MsmzOpts()
    o.c, o.glv, o.safe, o.buckets = c, glv, safe, buckets
    o.reserved[0], o.reserved[1] = reduce_affine, bits
    return o


def raw_segments(curve, ph, sh, segs, opts, log=None):
    """msmz_msm_segments through the C ABI -> (status, result bytes, infinity flags)"""
    from msm_zprize_amd._native import MsmzSegment, lib
    fb = curve.fe_bytes
    table = (MsmzSegment * max(len(segs), 1))(*[MsmzSegment(*s) for s in segs])
    out = C.create_string_buffer(2 * fb * max(len(segs), 1))
    inf = (C.c_int * max(len(segs), 1))()
    st = lib().msmz_msm_segments(curve._ctx, ph, sh, table, len(segs), C.byref(opts) if opts is not None else None, out, inf,
                                 None if log is None else C.byref(log))
    return st, out.raw, list(inf)


def _points(label, curve, raw, infs):
    fb = curve.fe_bytes
    return [(int.from_bytes(raw[2 * fb * k:2 * fb * k + fb], "little") if not (infs[k] and label in WEIER) else 0,
             int.from_bytes(raw[2 * fb * k + fb:2 * fb * (k + 1)], "little") if not (infs[k] and label in WEIER) else 1,
             bool(infs[k]) and label in WEIER) for k in range(len(infs))]


def _via_python(d, segs, options, safe=True, which="full", points=None):
    f = d.curve.Parallel.msmSegments if safe else d.curve.Parallel.msmSegmentsUnsafe
    return [_pt(d.label, r) for r in f(d.sc[which], points or d.pts, segs, options)]


# ------------------------------------------------------------------------------------------------ one class, one pipeline
# (label, glv, safe, c, segments): the whole class at the planner's window size -- small inputs: the generic sort kernels --
# and its two shortest members (2048 and 2049 entries: one tile wholly past the shorter one's end, on either tile size)
# at the window sizes the sort kernels are specialized for, which only a forced c reaches at these lengths
ONE_CLASS = [(label, glv, safe, 0, CLASS) for safe in (1, 0) for glv in (0, 1) for label in WEIER] + \
            [("bls12-377", 0, 1, 16, CLASS[:2]), ("bls12-377", 0, 1, 17, CLASS[:2]), ("bls12-377", 1, 1, 16, CLASS[:2])]


@pytest.mark.parametrize("label,glv,safe,c,segs", ONE_CLASS,
                         ids=[f"{l}-{g}-{s}" + (f"-c{c}" if c else "") for l, g, s, c, _ in ONE_CLASS])
def test_one_class_is_one_pipeline(data, label, glv, safe, c, segs):
    """lengths {2048, 2049, 3000, 4095} at unaligned offsets: trailing empty tiles, a ragged last tile, GLV images read
    at first_p behind a set larger than any segment"""
    d = data(label)
    r0, s0 = passes(d.curve)
    got = _via_python(d, segs, {"glv": glv, "c": c} if c else {"glv": glv}, bool(safe))
    assert passes(d.curve) == (r0, s0 + 1)
    assert not c or d.curve.Parallel.lastBatchLog.c == c
    for k, seg in enumerate(segs):
        assert got[k] == d.want(seg), (k, seg)


@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("label", WEIER)
def test_mixed_classes_overlaps_and_repeats(data, label, glv):
    """lengths {1, 5, 257, 300, 4095}: classes of 2, 3, 3 and 1 members; overlapping and repeated segments; caller order"""
    d = data(label)
    segs = [(0, 0, 1), (10, 20, 5), (100, 50, 257), (120, 60, 300), (1000, 2000, 4095), (10, 20, 5), (5999, 6199, 1),
            (200, 50, 257), (4, 7, 5)]
    r0, s0 = passes(d.curve)
    got = _via_python(d, segs, {"glv": glv})
    assert passes(d.curve) == (r0 + 1, s0 + 3)   # the class of one runs alone
    for k, seg in enumerate(segs):
        assert got[k] == d.want(seg), (k, seg)
    assert got[1] == got[5]


# ------------------------------------------------------------------------------------------------ equivalences
@pytest.mark.parametrize("label,glv", [(l, g) for l in WEIER for g in (-1, 0, 1)] + [("ed-on-bls12-377", 0)])
def test_equals_msm_resident_and_batch_resident(data, label, glv):
    """{0, 0, n} returns the bytes and status of msmz_msm_resident, B segments {0, k n, n} those of msmz_msm_batch_resident"""
    from msm_zprize_amd._native import lib
    d = data(label)
    curve, fb = d.curve, d.curve.fe_bytes
    o = _opts(glv=glv)
    for n in (300, 4095):
        out = C.create_string_buffer(2 * fb)
        inf = C.c_int()
        st = lib().msmz_msm_resident(curve._ctx, d.pts.handle, d.sc["full"].handle, n, C.byref(o), out, C.byref(inf), None)
        assert st == 0
        assert raw_segments(curve, d.pts.handle, d.sc["full"].handle, [(0, 0, n)], o) == (0, out.raw, [inf.value])
        assert _points(label, curve, out.raw, [inf.value])[0] == d.want((0, 0, n))
    n, B = 257, 3
    out = C.create_string_buffer(2 * fb * B)
    inf = (C.c_int * B)()
    r0, s0 = passes(curve)
    st = lib().msmz_msm_batch_resident(curve._ctx, d.pts.handle, d.sc["full"].handle, n, B, C.byref(o), out, inf, None)
    assert st == 0
    r1, s1 = passes(curve)
    got = raw_segments(curve, d.pts.handle, d.sc["full"].handle, [(0, k * n, n) for k in range(B)], o)
    assert got == (0, out.raw, list(inf))
    assert passes(curve) == (r1 + (r1 - r0), s1 + (s1 - s0))   # ... and runs as the batch ran
    assert _points(label, curve, got[1], got[2]) == [d.want((0, k * n, n)) for k in range(B)]


def test_ipa_round(data):
    """L = <a_lo, G_hi> and R = <a_hi, G_lo> in one call over the halves of one set, the generators folded with mulPoints
    (G'_i = G_lo,i + [u] G_hi,i), then an MSM over the folded set: <b, G'> = <b, G_lo> + <u b, G_hi>"""
    label = "bls12-377"
    d = data(label)
    n, h = 4096, 2048
    got = _via_python(d, [(h, 0, h), (0, h, h)], None, safe=False)
    assert got == [d.want((h, 0, h)), d.want((0, h, h))]
    u = 0x1234567890abcdef1234567890abcdef % d.q
    folded = d.curve.Parallel.mulPoints(u, d.pts, h, addend=d.pts, firstPoint=h)
    try:
        b = d.s["full"][4096:4096 + h]
        want = _pt(label, c_oracle.msm(P.CURVES[label], b + [(u * x) % d.q for x in b], d.big[:n]))
        res = d.curve.Parallel.msmSegmentsUnsafe(d.sc["full"], folded, [(0, 4096, h)])
        assert _pt(label, res[0]) == want
        assert _pt(label, d.curve.Parallel.msmUnsafe(d.sc["full"], folded, 5)["result"]) == \
            _pt(label, d.curve.Parallel.msmSegmentsUnsafe(d.sc["full"], folded, [(0, 0, 5)])[0])
    finally:
        folded.free()


# ------------------------------------------------------------------------------------------------ safe additions
@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("label", WEIER)
def test_safe_additions_inside_and_across_segments(data, label, glv):
    """equal and opposite points with equal scalars inside one segment (the same bucket in every window), and an equal pair
    straddling the boundary of two segments (it must NOT meet: each half belongs to its own problem)"""
    d = data(label)
    m = P.CURVES[label]["modulus"]
    big = [dict(p) for p in d.big[:300]]
    big[110] = dict(big[100])                                                      # equal, inside A
    big[111] = {"x": big[101]["x"], "y": (m - big[101]["y"]) % m, "isZero": False}   # opposite, inside A
    big[150] = dict(big[149])                                                      # equal, A's last and B's first
    A, B = (90, 40, 60), (150, 100, 60)            # point i of A has scalar i - 50, of B scalar i - 50
    s = list(d.s["full"][:300])
    s[110 - 50], s[111 - 50], s[150 - 50] = s[100 - 50], s[101 - 50], s[149 - 50]
    pts = d.curve.Parallel.pointsFromBigints(big)
    sc = d.curve.Parallel.scalarsFromBytes(_enc(s), 300)
    try:
        r0, s0 = passes(d.curve)
        got = [_pt(label, r) for r in d.curve.Parallel.msmSegments(sc, pts, [A, B, A], {"glv": glv})]
        assert passes(d.curve) == (r0, s0 + 1)
        want = [_pt(label, c_oracle.msm(P.CURVES[label], s[fs:fs + n], big[fp:fp + n])) for fp, fs, n in (A, B)]
        assert got == [want[0], want[1], want[0]]
    finally:
        pts.free()
        sc.free()


# ------------------------------------------------------------------------------------------------ options
@pytest.mark.parametrize("glv", [-1, 0])
@pytest.mark.parametrize("label", WEIER)
def test_scalar_bits_64(data, label, glv):
    """a 64-bit bound on the first class: few windows, the top one folded or spread by the entry index h * n_max + idx"""
    d = data(label)
    r0, s0 = passes(d.curve)
    got = _via_python(d, CLASS, {"glv": glv, "scalarBits": 64}, which="u64")
    assert passes(d.curve) == (r0, s0 + 1)
    log = d.curve.Parallel.lastBatchLog
    assert log.K == -(-65 // log.c)               # the windows of a 64-bit scalar, not of the field
    assert got == [d.want(seg, "u64") for seg in CLASS]
    # the bound is checked inside the segments only
    st, _, _ = raw_segments(d.curve, d.pts.handle, d.sc["full"].handle, CLASS, _opts(glv=glv, bits=64))
    assert st == MSMZ_ERR_RANGE


@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_precomputed_handle(data, label, glv):
    """factor 0 (every window in one bucket set): copies and GLV images are reached at first_p != 0; identical to the
    plain handle"""
    d = data(label)
    pre = d.curve.Parallel.precomputePoints(d.pts, NP, {"glv": glv}, 0)
    try:
        o = _opts(glv=glv)
        plain = raw_segments(d.curve, d.pts.handle, d.sc["full"].handle, CLASS, o)
        r0, s0 = passes(d.curve)
        got = raw_segments(d.curve, pre.handle, d.sc["full"].handle, CLASS, _opts(glv=-1))
        assert passes(d.curve) == (r0, s0 + 1)
        assert got == plain and got[0] == 0
        assert _points(label, d.curve, got[1], got[2]) == [d.want(seg) for seg in CLASS]
        one = raw_segments(d.curve, pre.handle, d.sc["full"].handle, [CLASS[2]], None)   # ... and through the range loop
        assert one[0] == 0 and _points(label, d.curve, one[1], one[2]) == [d.want(CLASS[2])]
        # options that contradict the handle, and the combinations no MSM over a precomputed handle supports
        assert raw_segments(d.curve, pre.handle, d.sc["full"].handle, CLASS, _opts(glv=1 - glv))[0] == MSMZ_ERR_ARG
        assert raw_segments(d.curve, pre.handle, d.sc["full"].handle, CLASS, _opts(c=pre.info["c"] + 1))[0] == MSMZ_ERR_ARG
        assert raw_segments(d.curve, pre.handle, d.sc["full"].handle, CLASS, _opts(buckets=1))[0] == MSMZ_ERR_UNSUPPORTED
        assert raw_segments(d.curve, pre.handle, d.sc["full"].handle, CLASS, _opts(reduce_affine=1))[0] == MSMZ_ERR_UNSUPPORTED
    finally:
        pre.free()
    half = d.curve.Parallel.precomputePoints(d.pts, 3000, {"glv": glv}, 0)
    try:   # first_p + n beyond the n the handle was built for
        assert raw_segments(d.curve, half.handle, d.sc["full"].handle, [(2000, 0, 1001)], None)[0] == MSMZ_ERR_ARG
        ok = raw_segments(d.curve, half.handle, d.sc["full"].handle, [(2000, 0, 1000), (1000, 5, 1999)], None)
        assert ok[0] == 0 and _points(label, d.curve, ok[1], ok[2]) == [d.want((2000, 0, 1000)), d.want((1000, 5, 1999))]
    finally:
        half.free()


@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_range_check_covers_the_segments_only(data, label, glv):
    """a resident scalar >= q (planted with msmz_import_scalars_into, which converts before it reports): segments that
    avoid it succeed, a segment whose LAST entry it is fails the call, the next call succeeds; and with the bad scalar at
    first_s + n_k, one past a segment that ends on a tile boundary inside a class sized for a longer one, the call succeeds
    (a guard on n_max would read it)"""
    from msm_zprize_amd._native import MsmzSrc, lib
    from msm_zprize_amd.parallel import DeviceArray
    d = data(label)
    BAD = 5000
    h = C.c_uint64()
    assert lib().msmz_alloc_scalars(d.curve._ctx, NS, C.byref(h)) == 0
    sc = DeviceArray(d.curve, h.value, NS, "scalars")
    try:
        good = _enc(d.s["full"])
        src = MsmzSrc(C.cast(C.c_char_p(good), C.c_void_p), 0, 32, 0, None, None)
        assert lib().msmz_import_scalars_into(d.curve._ctx, sc.handle, 0, C.byref(src), NS) == 0
        raw = _enc([d.q])
        src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
        assert lib().msmz_import_scalars_into(d.curve._ctx, sc.handle, BAD, C.byref(src), 1) == MSMZ_ERR_RANGE
        assert d.curve.Scalar.toBigints(sc, BAD, 1) == [d.q]   # resident all the same
        o = _opts(glv=glv)
        # one past the end: n_k = 2048 is whole tiles on either tile size, the class is sized for 4095
        clear = [(0, BAD - 2048, 2048), (1905, 100, 4095), (7, BAD + 1, 1199)]
        got = raw_segments(d.curve, d.pts.handle, sc.handle, clear, o)
        assert got[0] == 0 and _points(label, d.curve, got[1], got[2]) == [d.want(s) for s in clear]
        for hit in ([(0, BAD - 2047, 2048), (1905, 100, 4095)], [(0, BAD - 299, 300)], [(0, 0, 5), (3, BAD, 1)]):
            assert raw_segments(d.curve, d.pts.handle, sc.handle, hit, o)[0] == MSMZ_ERR_RANGE, hit
            got = raw_segments(d.curve, d.pts.handle, sc.handle, clear[:2], o)
            assert got[0] == 0 and _points(label, d.curve, got[1], got[2]) == [d.want(s) for s in clear[:2]]
    finally:
        sc.free()


# ------------------------------------------------------------------------------------------------ the loop path
@pytest.mark.parametrize("label,options", [("ed-on-bls12-377", {}), ("pallas", {"buckets": 1, "glv": 0}),
                                           ("pallas", {"reduceAffine": 1, "glv": 1})])
def test_loop_path(data, label, options):
    """twisted Edwards, projective buckets and reserved[0] = 1 run segment by segment, pointers advanced to each"""
    d = data(label)
    segs = [(3, 7, 300), (300, 0, 257), (3, 7, 300)]
    r0, s0 = passes(d.curve)
    got = _via_python(d, segs, options)
    assert passes(d.curve) == (r0 + 3, s0)
    assert got == [d.want(s) for s in segs]


@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_lowered_limits(data, label):
    """a class split into several sub-batches, and segments longer than a pass: the results do not change"""
    d = data(label)
    options = {"glv": 0, "c": 10}
    want = [d.want(seg) for seg in CLASS]
    assert _via_python(d, CLASS, options) == want
    K = d.curve.Parallel.lastBatchLog.K
    with limits(d.curve, 0, 2 * K * 4095):       # entries per problem = K * n_max: two problems per sub-batch
        r0, s0 = passes(d.curve)
        assert _via_python(d, CLASS, options) == want
        assert passes(d.curve) == (r0, s0 + 2)
    with limits(d.curve, 1000, 0):               # n_max beyond a pass: every segment in ceil(n / 1000) range passes
        r0, s0 = passes(d.curve)
        assert _via_python(d, CLASS, options) == want
        assert passes(d.curve) == (r0 + 3 + 3 + 3 + 5, s0)


# ------------------------------------------------------------------------------------------------ errors
def test_argument_errors(data):
    from msm_zprize_amd._native import MsmzSegment, lib
    d = data("pallas")
    curve, ph, sh = d.curve, d.pts.handle, d.sc["full"].handle
    o = _opts()
    fb = curve.fe_bytes
    table = (MsmzSegment * 1)(MsmzSegment(0, 0, 5))
    out = C.create_string_buffer(2 * fb)
    inf = (C.c_int * 1)()
    f = lib().msmz_msm_segments
    r0 = passes(curve)
    assert f(curve._ctx, ph, sh, None, 1, C.byref(o), out, inf, None) == MSMZ_ERR_ARG
    assert f(curve._ctx, ph, sh, table, 1, C.byref(o), None, inf, None) == MSMZ_ERR_ARG
    assert f(curve._ctx, ph, sh, table, 1, C.byref(o), out, None, None) == MSMZ_ERR_ARG
    assert f(curve._ctx, ph, sh, table, 0, C.byref(o), out, inf, None) == MSMZ_ERR_ARG
    assert f(None, ph, sh, table, 1, C.byref(o), out, inf, None) == MSMZ_ERR_ARG
    bad = [
        (ph, sh, [(0, 0, 0)]), (ph, sh, [(0, 0, 5), (0, 0, 0)]),                   # an empty segment
        (ph + 1000, sh, [(0, 0, 5)]), (ph, sh + 1000, [(0, 0, 5)]), (0, sh, [(0, 0, 5)]),   # unknown handles
        (sh, sh, [(0, 0, 5)]), (ph, ph, [(0, 0, 5)]), (sh, ph, [(0, 0, 5)]),       # wrong kinds
        (ph, sh, [(NP, 0, 1)]), (ph, sh, [(NP - 4, 0, 5)]), (ph, sh, [(0, 0, NP + 1)]),   # beyond the points
        (ph, sh, [(0, NS, 1)]), (ph, sh, [(0, NS - 4, 5)]),                         # beyond the scalars
        (ph, sh, [((1 << 64) - 1, 0, 2)]), (ph, sh, [(0, (1 << 64) - 1, 2)]), (ph, sh, [(2, 0, (1 << 64) - 1)]),   # wrap-around
        (ph, sh, [(0, 0, 5), (NP + 1, 0, 1)]),
    ]
    for p, s, segs in bad:
        assert raw_segments(curve, p, s, segs, o)[0] == MSMZ_ERR_ARG, (p, s, segs)
    assert raw_segments(curve, ph, sh, [(0, 0, 5)], _opts(bits=257))[0] == MSMZ_ERR_ARG
    assert raw_segments(curve, ph, sh, [(0, 0, 5)], _opts(bits=-1))[0] == MSMZ_ERR_ARG
    assert passes(curve) == r0                                                      # nothing ran
    got = raw_segments(curve, ph, sh, [(NP - 5, NS - 5, 5)], None)                   # a null opts, the sets' very ends
    assert got[0] == 0 and _points("pallas", curve, got[1], got[2]) == [d.want((NP - 5, NS - 5, 5))]


def test_multi_device_context_is_unsupported(mod):
    """sets are dealt to the devices in blocks: a range is not a prefix of a device's share"""
    mod.startThreads(devices=[0, 0])
    try:
        curve = _create(mod, "pallas")
    finally:
        mod.startThreads()
    try:
        pts = curve.Parallel.randomPointsFast(100, 1)
        sc = curve.Parallel.randomScalars(100, 2)
        assert raw_segments(curve, pts.handle, sc.handle, [(0, 0, 50)], _opts())[0] == MSMZ_ERR_UNSUPPORTED
        with pytest.raises(Exception):
            curve.Parallel.msmSegments(sc, pts, [(0, 0, 50)])
    finally:
        curve.close()


def test_log_is_the_whole_call(data):
    """totals over every pipeline of the call, merged as a batch's"""
    from msm_zprize_amd._native import MsmzLog
    d = data("bls12-377")
    o = _opts(glv=0)
    whole, a, b = MsmzLog(), MsmzLog(), MsmzLog()
    segs = CLASS + [(0, 0, 300), (5, 5, 257)]
    assert raw_segments(d.curve, d.pts.handle, d.sc["full"].handle, segs, o, whole)[0] == 0
    assert raw_segments(d.curve, d.pts.handle, d.sc["full"].handle, CLASS, o, a)[0] == 0
    assert raw_segments(d.curve, d.pts.handle, d.sc["full"].handle, segs[4:], o, b)[0] == 0
    assert whole.n_entries == a.n_entries + b.n_entries and whole.n_pairs == a.n_pairs + b.n_pairs
    assert whole.max_bucket == max(a.max_bucket, b.max_bucket) and whole.rounds == max(a.rounds, b.rounds)
    assert whole.stage_ms[7] > 0

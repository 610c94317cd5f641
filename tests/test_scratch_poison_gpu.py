"""No result may depend on what scratch memory held before the call ("Scratch is undefined at the start of
every call").

Every stage of the engine works in grow-only device scratch that is never cleared between calls, and a new result
handle is handed to its kernel as the allocator left it.  msmz_test_poison (include/msmz_test.h) fills every scratch
buffer of a context over its whole capacity with one byte and arms the context, so that every later allocation --
scratch that grows, every new handle -- is filled too.  Each workload here runs once as it is and then again under the
patterns 0x00 (what a fresh process normally sees), 0xa5 and 0x5a: every poisoned run must equal the first one byte for
byte -- points, downloaded sets, the log's n_entries / n_pairs / max_bucket -- and the first one must equal the
Python-integer or oracle answer of the util modules.  The patterns are a loop inside each test, 0x00 first, so that the
reference of a workload is computed once.

One fresh context per curve for this module: capacities stay small and a fill costs microseconds.  Sizes come from the
geometry hooks: the smallest at which a kernel has more than one tile and a partial last one, and the smallest at which
a one-workgroup fold loops.  Those largest sizes (the looping folds, the three-pass transform) run on BLS12-377 only: the
loops are the same template code for every scalar field, and every field runs the one-tile-plus-one sizes.

Not reachable from here: MSMZ_NO_BUCKET_SUMS is read when a context is created, from the environment; the long-bucket
inputs below run msmBasic at c = 2 too, where a bucket holds several chunk accumulators and k_bucket_sums runs (engine.h:
more than 1.5 accumulators per bucket); the path without it is what the larger windows take."""
import ctypes as C
import random
from contextlib import contextmanager

import pytest

import check_points_util as U
import compressed_util as Z
import fixed_base_util as FB
import matrix_util as MX
import mle_util as ML
import ntt_util as NT
import points_mul_util as M
import scalar_ops_util as S
import scalar_scan_util as SC
from oracle import c_oracle
from oracle import params as P
from test_limits_gpu import _variants

pytestmark = pytest.mark.gpu

WEIER = ["bls12-377", "pallas", "bls12-381"]
ALL = WEIER + ["ed-on-bls12-377"]
BIG = "bls12-377"   # the curve of the largest sizes
PATTERNS = (0x00, 0xa5, 0x5a)
MSMZ_ERR_ARG, MSMZ_ERR_RANGE = 1, 6
UNTOUCHED = 0x5151515151515151


@pytest.fixture(scope="module")
def mod():
    import msm_zprize_amd as m
    m.startThreads()
    return m


def _create(mod, label):
    params = mod.curves.BY_LABEL[label]
    return (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)


@pytest.fixture(scope="module")
def curves(mod):
    """this module's own context of every curve"""
    cache = {}

    def get(label):
        if label not in cache:
            mod.startThreads()
            cache[label] = _create(mod, label)
        return cache[label]

    yield get
    for c in cache.values():
        c.close()


@contextmanager
def fresh(mod, label, devices=None):
    """a context of its own: for what needs first allocations, a large geometry, or two engines"""
    mod.startThreads(devices=devices) if devices else mod.startThreads()
    curve = _create(mod, label)
    mod.startThreads()
    try:
        yield curve
    finally:
        curve.close()


def _lib():
    from msm_zprize_amd._native import lib
    return lib()


def poison(curve, pattern):
    """msmz_test_poison -> (buffers filled, bytes written)"""
    nb, by = C.c_uint64(UNTOUCHED), C.c_uint64(UNTOUCHED)
    assert _lib().msmz_test_poison(curve._ctx, pattern, C.byref(nb), C.byref(by)) == 0, pattern
    assert nb.value != UNTOUCHED and by.value != UNTOUCHED
    return nb.value, by.value


def scratch(curve, engine=0):
    """msmz_test_scratch -> (buffers, bytes) that a fill would write on one engine of the context; fills nothing"""
    nb, by = C.c_uint64(UNTOUCHED), C.c_uint64(UNTOUCHED)
    assert _lib().msmz_test_scratch(curve._ctx, engine, C.byref(nb), C.byref(by)) == 0, engine
    return nb.value, by.value


def under_poison(curve, run, want=None, what=""):
    """run() as it is, then under every pattern: all equal, and equal to `want` if given -> the first result"""
    base = run()
    if want is not None:
        assert base == want, (what, "unpoisoned")
    for pat in PATTERNS:
        poison(curve, pat)
        got = run()
        assert got == base, (what, hex(pat))
    return base


def _enc(scalars):
    return b"".join(int(s).to_bytes(32, "little") for s in scalars)


def _pt(label, p):
    return (p["x"], p["y"], bool(p.get("isZero", False)) and label in WEIER)


def _oracle(label, scalars, points):
    return _pt(label, c_oracle.msm(P.CURVES[label], scalars, points))


def _msm(curve, label, fn, scalars, pts, n, opts):
    """one MSM -> (point, n_entries, n_pairs, max_bucket)"""
    if fn == "msmProjective":
        r = curve.Parallel.msmProjective(scalars, pts, n, dict(opts))
    else:
        r = getattr(curve.Parallel, fn)(scalars, pts, n, False, dict(opts))
    s = r["stats"]
    return _pt(label, r["result"]), int(s.n_entries), int(s.n_pairs), int(s.max_bucket)


def _msm_checked(curve, label, fn, scalars, pts, n, opts, want, what):
    got = under_poison(curve, lambda: _msm(curve, label, fn, scalars, pts, n, opts), None, what)
    assert got[0] == want, what
    assert got[1] > 0 and got[3] > 0, what
    return got


def _scalars_of(curve, arr, first=0, n=None):
    return curve.Scalar.toBigints(arr, first, n)


def _raw_scalars(curve, arr):
    buf = C.create_string_buffer(32 * arr.n)
    assert _lib().msmz_download_scalars(curve._ctx, arr.handle, 0, arr.n, buf) == 0
    return buf.raw


def _raw_points(curve, arr, n=None):
    """records and flags of a point set as msmz_download_points gives them"""
    n = arr.n if n is None else n
    buf, inf = C.create_string_buffer(2 * curve.fe_bytes * n), C.create_string_buffer(n)
    assert _lib().msmz_download_points(curve._ctx, arr.handle, 0, n, buf, inf) == 0
    return buf.raw, inf.raw


def _plant(curve, arr, index, value):
    """make `value` (>= q) entry `index` of a resident set, as tests/test_scalar_ops_gpu.py does: msmz_import_scalars_into
    converts before it reports, so after its MSMZ_ERR_RANGE the refused value is what the handle holds"""
    from msm_zprize_amd._native import MsmzSrc
    raw = S.encode([value])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, arr.handle, index, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert curve.Scalar.toBigints(arr, index, 1) == [value]


def _geometry(name, n):
    vals = [C.c_uint32(0) for _ in range(n)]
    getattr(_lib(), name)(*[C.byref(v) for v in vals])
    assert all(v.value for v in vals), name
    return [v.value for v in vals]


# ================================================================================================ MSM
N_SET, N_SMALL = 2500, 257


class MsmData:
    """One curve's inputs: N_SET device-generated points, N_SET scalars with the group order's neighbours at the edges
    of the small prefix, as host bytes and resident, and the oracle's MSMs of both sizes, computed once."""

    def __init__(self, curve, label):
        self.label, self.q = label, P.CURVES[label]["order"]
        par = curve.Parallel
        self.pts = par.randomPointsFast(N_SET, 4321)
        self.big = curve.Affine.toBigints(self.pts)
        rng = random.Random("poison" + label)
        self.s = [rng.randrange(self.q) for _ in range(N_SET)]
        self.s[0], self.s[N_SMALL - 1], self.s[N_SMALL], self.s[N_SET - 1] = self.q - 1, self.q - 2, 1, self.q - 1
        self.host = _enc(self.s)
        self.res = par.scalarsFromBytes(self.host, N_SET)
        self.want = {n: _oracle(label, self.s[:n], self.big[:n]) for n in (N_SMALL, N_SET)}


@pytest.fixture(scope="module")
def msm_data(curves):
    cache = {}

    def get(label):
        if label not in cache:
            cache[label] = MsmData(curves(label), label)
        return cache[label]

    return get


@pytest.mark.parametrize("label", ALL)
def test_msm_every_variant(curves, msm_data, label):
    """every variant of test_limits_gpu._variants at n = 257 and n = 2500, resident and host scalars"""
    curve, d = curves(label), msm_data(label)
    for n in (N_SMALL, N_SET):
        for name, fn, opts, _ in _variants(label):
            for kind, sc in (("resident", d.res), ("host", d.host)):
                _msm_checked(curve, label, fn, sc, d.pts, n, opts, d.want[n], (name, n, kind))


def test_msm_sort_paths(mod, msm_data, curves):
    """c = 22 takes the fallback sort (digits materialized, cleared histogram and cursors), c = 19 the two-level sort
    with more bins than threads, as test_window_sizes_that_take_the_fallback_sort; a context of its own, because these
    geometries allocate hundreds of megabytes that every later fill would have to write"""
    label = "bls12-377"
    d = msm_data(label)
    with fresh(mod, label) as curve:
        pts = curve.Parallel.randomPointsFast(N_SET, 4321)   # (the same points: point i depends on the seed and i only)
        for glv, c in ((0, 22), (1, 22), (0, 19), (1, 19)):
            for sc in (d.host, curve.Parallel.scalarsFromBytes(d.host, N_SET)):
                _msm_checked(curve, label, "msmUnsafe", sc, pts, N_SET, {"glv": glv, "c": c}, d.want[N_SET], (glv, c))
        _msm_checked(curve, label, "msmProjective", d.host, pts, N_SET, {"c": 22}, d.want[N_SET], "projective c=22")


@pytest.mark.parametrize("label", ["bls12-377", "pallas", "ed-on-bls12-377"])
def test_msm_long_buckets(curves, label):
    """the repeated-scalar inputs of test_long_buckets, n = 700: the tree rounds run many rounds and stop short of the
    longest bucket, msmBasic leaves several chunk accumulators per bucket (k_bucket_sums runs)"""
    curve = curves(label)
    q = P.CURVES[label]["order"]
    rng = random.Random(77)
    n = 700
    pts = curve.Parallel.randomPointsFast(n, 4242)
    points = curve.Affine.toBigints(pts)
    s1, s2 = rng.randrange(q), rng.randrange(q)
    for k, scalars in enumerate(([s1] * n, [s1 if i % 3 else s2 for i in range(n)],
                                 [s1 if i < 500 else rng.randrange(q) for i in range(n)])):
        want = _oracle(label, scalars, points)
        sc = curve.Parallel.scalarsFromBigints(scalars)
        if label in WEIER:
            for glv in (0, 1):
                for cc in (0, 4, 9):
                    _msm_checked(curve, label, "msmUnsafe", sc, pts, n, {"glv": glv, "c": cc}, want, (k, glv, cc))
                _msm_checked(curve, label, "msm", sc, pts, n, {"glv": glv}, want, (k, glv, "safe"))
                _msm_checked(curve, label, "msmUnsafe", sc, pts, n, {"glv": glv, "reduceAffine": 1}, want, (k, glv, "f2"))
            for cc in (0, 2):   # (c = 2: ~9 chunk accumulators per bucket, so k_bucket_sums runs)
                _msm_checked(curve, label, "msmProjective", sc, pts, n, {"c": cc}, want, (k, "projective", cc))
        else:
            for cc in (0, 6, 2):
                _msm_checked(curve, label, "msm", sc, pts, n, {"c": cc}, want, (k, cc))
        sc.free()
    pts.free()


@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_shrinking_geometry(mod, label):
    """no hook at first: n = 4096 at c = 16, then n = 65 at c = 5, then a batch of three, then n = 1 -- the small calls
    run with the large call's records, not a constant, behind their extents.  Then the same sequence with a poison
    between the calls."""
    q = P.CURVES[label]["order"]
    with fresh(mod, label) as curve:
        par = curve.Parallel
        pts = par.randomPointsFast(4096, 99)
        big = curve.Affine.toBigints(pts)
        rng = random.Random("shrink" + label)
        s = [rng.randrange(q) for _ in range(4096)]
        sc = par.scalarsFromBytes(_enc(s), 4096)
        want = {n: _oracle(label, s[:n], big[:n]) for n in (4096, 65, 1)}
        want_batch = [_oracle(label, s[k * N_SMALL:(k + 1) * N_SMALL], big[:N_SMALL]) for k in range(3)]

        def sequence(between):
            for glv in (0, 1):
                for fn in ("msmUnsafe", "msm"):
                    assert _msm(curve, label, fn, sc, pts, 4096, {"glv": glv, "c": 16})[0] == want[4096], (glv, fn)
                    between()
                    assert _msm(curve, label, fn, sc, pts, 65, {"glv": glv, "c": 5})[0] == want[65], (glv, fn)
                    between()
                    got = [_pt(label, r) for r in par.msmBatchUnsafe(sc, pts, N_SMALL, {"glv": glv, "batch": 3})]
                    assert got == want_batch, (glv, fn)
                    between()
                    assert _msm(curve, label, fn, sc, pts, 1, {"glv": glv})[0] == want[1], (glv, fn)
                    between()
            assert _msm(curve, label, "msmProjective", sc, pts, 4096, {"c": 12})[0] == want[4096]
            between()
            assert _msm(curve, label, "msmProjective", sc, pts, 65, {"c": 5})[0] == want[65]

        sequence(lambda: None)
        for pat in PATTERNS:
            sequence(lambda: poison(curve, pat))


@pytest.mark.parametrize("label", WEIER)
def test_batch_segments_precomputed_short(curves, msm_data, label):
    curve, d = curves(label), msm_data(label)
    par, n, big = curve.Parallel, N_SMALL, msm_data(label).big
    L = _lib()
    # ---- msm_batch_resident: B = 3 vectors of 257 (entries [k n, (k + 1) n) of the resident set)
    want = [_oracle(label, d.s[k * n:(k + 1) * n], big[:n]) for k in range(3)]
    for glv in (0, 1):
        for f in (par.msmBatch, par.msmBatchUnsafe):
            def run():
                res = [_pt(label, r) for r in f(d.res, d.pts, n, {"glv": glv, "batch": 3})]
                log = par.lastBatchLog
                return res, int(log.n_entries), int(log.n_pairs), int(log.max_bucket)
            assert under_poison(curve, run, None, ("batch", glv))[0] == want, glv
    # ---- msm_segments: three segments of unequal length, the first two overlapping in points and scalars
    segs = [(0, 0, 257), (100, 50, 200), (150, 300, 31)]
    want = [_oracle(label, d.s[fs:fs + m], big[fp:fp + m]) for fp, fs, m in segs]
    for glv in (0, 1):
        run = lambda: [_pt(label, r) for r in par.msmSegmentsUnsafe(d.res, d.pts, segs, {"glv": glv})]
        under_poison(curve, run, want, ("segments", glv))
    # ---- a precomputed set of factor 2: poisoned before precompute_points AND before the MSM over the set
    want = d.want[n]
    for glv in (0, 1):
        for pat in (None,) + PATTERNS:
            if pat is not None:
                poison(curve, pat)
            pre = par.precomputePoints(d.pts, n, {"glv": glv, "c": 8}, 2)
            if pat is not None:
                poison(curve, pat)
            for fn in ("msm", "msmUnsafe"):
                assert _msm(curve, label, fn, d.res, pre, n, {})[0] == want, ("precomputed", glv, pat, fn)
            pre.free()
    # ---- scalar_bits = 64
    rng = random.Random("short" + label)
    short = [rng.randrange(1 << 64) for _ in range(n)]
    short[0], short[n - 1] = (1 << 64) - 1, 1 << 63
    want = _oracle(label, short, big[:n])
    for glv in (0, 1):
        for sc in (_enc(short), par.scalarsFromBytes(_enc(short), n)):
            _msm_checked(curve, label, "msm", sc, d.pts, n, {"glv": glv, "scalarBits": 64}, want, ("scalarBits", glv))
    # ---- a pass size that splits n = 2500 raggedly: the second pass runs on the first pass's leftovers
    assert L.msmz_test_set_limits(curve._ctx, 1000, 0) == 0
    try:
        for glv in (0, 1):
            for fn in ("msmUnsafe", "msm", "msmProjective"):
                if fn == "msmProjective" and glv:
                    continue
                opts = {} if fn == "msmProjective" else {"glv": glv}
                under_poison(curve, lambda: _msm(curve, label, fn, d.res, d.pts, N_SET, opts)[0], d.want[N_SET],
                             ("passes", glv, fn))
    finally:
        assert L.msmz_test_set_limits(curve._ctx, 0, 0) == 0
    # ---- the lowered GLV bound: the redone MSM runs on the failed attempt's scratch
    before = L.msmz_test_retries(curve._ctx)
    assert L.msmz_test_set_glv_bits(curve._ctx, 100) == 0
    try:
        for fn in ("msmUnsafe", "msm"):
            _msm_checked(curve, label, fn, d.res, d.pts, n, {"glv": 1, "c": 8}, d.want[n], ("glv redo", fn))
    finally:
        assert L.msmz_test_set_glv_bits(curve._ctx, 0) == 0
    assert L.msmz_test_retries(curve._ctx) >= before + 2 * (1 + len(PATTERNS))


# ================================================================================================ scalar sets
def _upload(curve, vals):
    return curve.Parallel.scalarsFromBytes(S.encode(vals), len(vals))


def _device_vectors(curve, n, seed):
    """two device-made sets of n scalars and their values (for the sizes at which an upload would be slow)"""
    x, y = curve.Parallel.randomScalars(n, seed), curve.Parallel.randomScalars(n, seed + 1)
    return x, y, S.decode(_raw_scalars(curve, x)), S.decode(_raw_scalars(curve, y))


@pytest.mark.parametrize("label", ALL)
def test_scalars_dot_recurrence_inverse(curves, label):
    """one tile + 1 of the dot product and of every recurrence mode, 3 C + 7 inversions with zeros on both sides of a
    chunk edge, and powers / combine into a NEW handle, whose memory the armed allocator fills"""
    curve, q, par = curves(label), S.order(label), curves(label).Parallel
    dot_tile, _ = _geometry("msmz_test_scalar_dot_geometry", 2)
    rec_tile, _, inv_chunk = _geometry("msmz_test_scalar_scan_geometry", 3)
    # ---- dot
    n = dot_tile + 1
    xs, ys = S.build_vectors(label, n, 31)
    x, y = _upload(curve, xs), _upload(curve, ys)
    under_poison(curve, lambda: par.innerProduct(x, y), sum(a * b for a, b in zip(xs, ys)) % q, "dot")
    under_poison(curve, lambda: par.innerProduct(x), sum(xs) % q, "sum")
    # ---- combine and powers into new handles
    a, b = random.Random(label).randrange(q), q - 1

    def combine():
        out = par.combineScalars(a, x, b, y)
        raw = _raw_scalars(curve, out)
        out.free()
        return raw
    under_poison(curve, combine, S.encode([(a * u + b * v) % q for u, v in zip(xs, ys)]), "combine")

    def powers():
        out = par.scalarPowers(a, n, b)
        raw = _raw_scalars(curve, out)
        out.free()
        return raw
    want, v = [], b
    for _ in range(n):
        want.append(v)
        v = v * a % q
    under_poison(curve, powers, S.encode(want), "powers")
    x.free(); y.free()
    # ---- recurrence: the modes of test_edge_sizes_every_mode at T + 1
    n = rec_tile + 1
    xs, ys = S.build_vectors(label, n, 32)
    x, y = _upload(curve, xs), _upload(curve, ys)
    k = random.Random(n).randrange(2, q)
    for mode, mult, addend in SC.MODES:
        av = None if mult is None else (k if mult == "broadcast" else xs)
        aa = None if mult is None else (k if mult == "broadcast" else x)
        for reverse in (False, True):
            for exclusive in (False, True):
                def run():
                    out, last = par.scalarRecurrence(aa, y if addend else None, n, None, reverse, exclusive)
                    raw = _raw_scalars(curve, out)
                    out.free()
                    return raw, last
                vals, last = SC.recurrence(q, n, av, ys if addend else None, None, reverse, exclusive)
                under_poison(curve, run, (S.encode(vals), last), (mode, reverse, exclusive))
    x.free(); y.free()
    # ---- inverse: zeros at both sides of the first and second chunk edge, at the ends
    n = 3 * inv_chunk + 7
    xs, _ = S.build_vectors(label, n, 33)
    xs = [v or 1 for v in xs]
    for i in (0, inv_chunk - 1, inv_chunk, 2 * inv_chunk - 1, 2 * inv_chunk, 2 * inv_chunk + 1, n - 1):
        xs[i] = 0
    x = _upload(curve, xs)

    def invert():
        out, zeros = par.invertScalars(x)
        raw = _raw_scalars(curve, out)
        out.free()
        return raw, zeros
    inv, zeros = SC.inverse(q, xs)
    under_poison(curve, invert, (S.encode(inv), zeros), "inverse")
    x.free()


def test_scalars_dot_second_level_loops(curves):
    """the smallest size at which the one workgroup of k_scalars_dot_fold loops over the tile sums that the first launch
    left: tile x pass + 1"""
    label = BIG
    curve, q, par = curves(label), S.order(label), curves(label).Parallel
    dot_tile, dot_pass = _geometry("msmz_test_scalar_dot_geometry", 2)
    n = dot_tile * dot_pass + 1
    x, y, xs, ys = _device_vectors(curve, n, 41)
    under_poison(curve, lambda: par.innerProduct(x, y), sum(a * b for a, b in zip(xs, ys)) % q, "dot")
    x.free(); y.free()


@pytest.fixture(scope="module")
def rec_big(curves):
    """two device-made sets of tile x pass + 1 scalars on the context of BIG and their values, for every mode below"""
    rec_tile, rec_pass, _ = _geometry("msmz_test_scalar_scan_geometry", 3)
    return _device_vectors(curves(BIG), rec_tile * rec_pass + 1, 43)


@pytest.mark.parametrize("mode", [m[0] for m in SC.MODES])
def test_scalars_recurrence_second_level_loops(curves, rec_big, mode):
    """every mode of test_edge_sizes_every_mode, forward and reverse, inclusive and exclusive, at the smallest size at
    which the one workgroup of k_scalars_rec_carry loops over the tile aggregates: tile x pass + 1.  One case per mode,
    one after another on one context: a mode that carries only part of an aggregate runs on what the mode before it left
    in sscan_, and on the pattern"""
    label = BIG
    curve, q, par = curves(label), S.order(label), curves(label).Parallel
    x, y, xs, ys = rec_big
    n = len(xs)
    k = random.Random(n).randrange(2, q)
    _, mult, addend = SC.MODE[mode]
    av = None if mult is None else (k if mult == "broadcast" else xs)
    aa = None if mult is None else (k if mult == "broadcast" else x)
    for reverse in (False, True):
        for exclusive in (False, True):
            def run():
                out, last = par.scalarRecurrence(aa, y if addend else None, n, None, reverse, exclusive)
                raw = _raw_scalars(curve, out)
                out.free()
                return raw, last
            vals, last = SC.recurrence(q, n, av, ys if addend else None, None, reverse, exclusive)
            under_poison(curve, run, (S.encode(vals), last), (mode, reverse, exclusive))


def _ntt_case(curve, label, log_n, big):
    """forward with a coset, count = 2 and n_in < n; inverse with a coset back to the inputs; plain forward in place"""
    q, par = S.order(label), curve.Parallel
    n = 1 << log_n
    n_in = n - 3 if n > 4 else n
    w, g = NT.root(label, log_n), 7
    v0 = NT.inputs(label, n_in, 50 + log_n)
    k = q - 2
    v1 = [k * v % q for v in v0]   # (the second vector a multiple of the first: its transform is the same multiple)
    x = _upload(curve, v0 + v1)
    t0 = NT.transform(q, v0, n, w, False, g)
    want = S.encode(t0 + [k * v % q for v in t0])

    def forward():
        out = par.ntt(x, log_n, shift=g, nIn=n_in, count=2)
        raw = _raw_scalars(curve, out)
        out.free()
        return raw
    under_poison(curve, forward, want, ("forward", log_n))
    f = par.ntt(x, log_n, shift=g, nIn=n_in, count=2)
    back = S.encode(v0 + [0] * (n - n_in) + v1 + [0] * (n - n_in))

    def inverse():
        out = par.ntt(f, log_n, inverse=True, shift=g, count=2)
        raw = _raw_scalars(curve, out)
        out.free()
        return raw
    under_poison(curve, inverse, back, ("inverse", log_n))
    if not big:
        full = NT.inputs(label, n, 60 + log_n)
        plain = S.encode(NT.transform(q, full, n, w))

        def in_place():
            y = _upload(curve, full)
            par.ntt(y, log_n, out=y)
            raw = _raw_scalars(curve, y)
            y.free()
            return raw
        under_poison(curve, in_place, plain, ("in place", log_n))
    x.free(); f.free()


# (the scalar field of ed-on-bls12-377 has two-adicity 1: no transform of more than two entries, tests/test_ntt_gpu.py)
@pytest.mark.parametrize("label", [l for l in ALL if NT.two_adicity(l) >= 17])
def test_scalars_ntt_one_and_two_passes(curves, label):
    """the one-pass limit and the smallest two-pass size"""
    L = _lib()
    one = NT.pass_log(L)
    assert len(NT.plan(L, NT.curve_id(label), one)[1]) == 1 and len(NT.plan(L, NT.curve_id(label), one + 1)[1]) == 2
    for log_n in (one, one + 1):
        _ntt_case(curves(label), label, log_n, False)


def test_scalars_ntt_three_passes(curves):
    """log_n = 17 is the smallest plan of three passes (ntt_plan.h): both scratch copies are in use"""
    L = _lib()
    assert len(NT.plan(L, NT.curve_id(BIG), 16)[1]) == 2 and len(NT.plan(L, NT.curve_id(BIG), 17)[1]) == 3
    _ntt_case(curves(BIG), BIG, 17, True)


def _round_two_tables(fs, gs, c, q, low):
    """ML.round_poly for the ONE term c f g, as three inner products: g(t) = c sum (lo_f + t d_f)(lo_g + t d_g) at t = 0,
    1, 2.  For tables too long for the general loop; _mle_case holds it against ML.round_poly where both can run."""
    pf, pg = ML.pairs(fs, low), ML.pairs(gs, low)
    a = sum(x[0] * y[0] for x, y in zip(pf, pg))
    b = sum(x[0] * (y[1] - y[0]) + (x[1] - x[0]) * y[0] for x, y in zip(pf, pg))
    d = sum((x[1] - x[0]) * (y[1] - y[0]) for x, y in zip(pf, pg))
    return [c * (a + t * b + t * t * d) % q for t in range(3)]


def _mle_big(curve, label, v_eval, v_round):
    """what has a second level: mle_eval over 2^v_eval entries, one sumcheck round of c f g over 2^v_round"""
    q, par = S.order(label), curve.Parallel
    rng = random.Random(f"mle big {label}")
    f, g = par.randomScalars(1 << v_round, 75), par.randomScalars(1 << v_round, 76)
    fs, gs = S.decode(_raw_scalars(curve, f)), S.decode(_raw_scalars(curve, g))
    point = [rng.randrange(q) for _ in range(v_eval)]
    want = sum(a * b for a, b in zip(fs, ML.eq(point, q))) % q
    under_poison(curve, lambda: par.evaluateMle(f, point), want, ("eval", v_eval))
    c = rng.randrange(1, q)
    under_poison(curve, lambda: par.sumcheckRound([f, g], [(c, 3)], nVars=v_round), _round_two_tables(fs, gs, c, q, False),
                 ("sumcheck", v_round))
    f.free(); g.free()


def _mle_case(curve, label, v):
    q, par = S.order(label), curve.Parallel
    rng = random.Random(f"mle{label}{v}")
    n = 1 << v
    point = [rng.randrange(q) for _ in range(v)]
    scale = rng.randrange(1, q)
    table = ML.eq(point, q, scale)

    def eq_table():
        out = par.eqTable(point, scale)
        raw = _raw_scalars(curve, out)
        out.free()
        return raw
    under_poison(curve, eq_table, S.encode(table), ("eq", v))
    f, g = par.randomScalars(n, 70 + v), par.randomScalars(n, 71 + v)
    fs, gs = S.decode(_raw_scalars(curve, f)), S.decode(_raw_scalars(curve, g))
    eq1 = ML.eq(point, q)
    under_poison(curve, lambda: par.evaluateMle(f, point), sum(a * b for a, b in zip(fs, eq1)) % q, ("eval", v))
    r = rng.randrange(q)
    for low in (False, True):
        def bind():
            out = par.bindMle(f, r, low=low)
            raw = _raw_scalars(curve, out)
            out.free()
            return raw
        under_poison(curve, bind, S.encode(ML.bind(fs, r, q, low)), ("bind", v, low))
        terms = [(rng.randrange(q), 3), (None, 1), (q - 1, 2)]
        under_poison(curve, lambda: par.sumcheckRound([f, g], terms, low=low), ML.round_poly([fs, gs], terms, q, low),
                     ("sumcheck", v, low))
        assert _round_two_tables(fs, gs, terms[0][0], q, low) == ML.round_poly([fs, gs], terms[:1], q, low)
    # in place: the low half of a copy is overwritten
    want = S.encode(ML.bind(fs, r, q))

    def bind_in_place():
        y = par.combineScalars(1, f)
        par.bindMle(y, r, out=y)
        raw = _raw_scalars(curve, y)[:32 * (n // 2)]
        y.free()
        return raw
    under_poison(curve, bind_in_place, want, ("bind in place", v))
    f.free(); g.free()


def _first_power_above(x):
    v = 0
    while (1 << v) <= x:
        v += 1
    return v


@pytest.mark.parametrize("label", ALL)
def test_mle_more_than_one_tile(curves, label):
    """tables of the smallest 2^v that is more than one tile of every kernel (a table cannot be one tile + 1 long)"""
    run, eval_tile, round_tile = _geometry("msmz_test_mle_geometry", 3)
    _mle_case(curves(label), label, _first_power_above(max(eval_tile, 2 * round_tile, 256 * run)))


def test_mle_second_level_loops(curves):
    """... and the smallest tables whose tiles are more than one pass of k_scalars_dot_fold: mle_eval, and a sumcheck
    round, whose tiles are tiles of pair indices.  (eq_table and mle_bind have no second level.)"""
    _, eval_tile, round_tile = _geometry("msmz_test_mle_geometry", 3)
    _, dot_pass = _geometry("msmz_test_scalar_dot_geometry", 2)
    _mle_big(curves(BIG), BIG, _first_power_above(eval_tile * dot_pass), _first_power_above(2 * round_tile * dot_pass))


def _matrix_case(curve, label, nnz, structures):
    """structures: {name: (rows in sorted order, n_rows)}.  Every run creates the matrix anew, so matrix_create runs
    under every pattern too: its forms are new device buffers, its values are packed through stage_.  The triples go in
    as unsigned 32-bit buffers and a resident value set, so that the host side of a large matrix costs nothing."""
    import array
    q, par = S.order(label), curve.Parallel
    rng = random.Random(f"matrix{label}{nnz}")
    for name, (rows, n_rows) in structures.items():
        n_cols = 300
        cols = MX.columns(nnz, n_cols, rng)
        vals = MX.values_for(nnz, q, rng)
        srows, scols, svals = MX.shuffled(rows, cols, vals, rng)
        arows, acols, va = array.array("I", srows), array.array("I", scols), _upload(curve, svals)
        xs, xt = MX.x_for(n_cols, q, rng), MX.x_for(n_rows, q, rng)
        x, xtr = _upload(curve, xs), _upload(curve, xt)
        want = S.encode(MX.matvec(rows, cols, vals, xs, n_rows, q))
        want_t = S.encode(MX.matvec(rows, cols, vals, xt, n_cols, q, True))
        if name == "empty_rows":
            assert 0 not in rows and want[:32] == bytes(32)   # an empty row's output is 0, not the pattern

        def product(transpose):
            # (a small matrix takes its values as a host list: uploaded through stage_ into a new handle on every run)
            m = par.sparseMatrix(arows, acols, svals if nnz <= 4096 else va, (n_rows, n_cols), "both")
            out = par.matVec(m, xtr if transpose else x, transpose=transpose)
            raw = _raw_scalars(curve, out)
            out.free()
            m.free()
            return raw
        under_poison(curve, lambda: product(False), want, (name, nnz))
        under_poison(curve, lambda: product(True), want_t, (name, nnz, "transposed"))
        x.free(); xtr.free(); va.free()


@pytest.mark.parametrize("label", ALL)
def test_matrix_one_tile_plus_one(curves, label):
    """nnz = T + 1: one row (the carry chains across the tiles), one entry per row (outputs cleared, then written), and
    a matrix with empty rows, whose outputs must be 0"""
    T, E, _ = _geometry("msmz_test_matrix_geometry", 3)
    every = MX.structures(T + 1, T, E)
    _matrix_case(curves(label), label, T + 1, {k: every[k] for k in ("one_row", "one_per_row", "empty_rows")})


@pytest.mark.parametrize("name", ["one_row", "one_per_row"])
def test_matrix_fold_loops(curves, name):
    """the smallest nnz whose tile carries are more than one pass of k_matrix_fold: one row, where the sum crosses from
    pass to pass, and one entry per row, where the outputs are cleared and then written from every tile's carry; plain
    and transposed, matrix_create under every pattern as well"""
    T, _, per_pass = _geometry("msmz_test_matrix_geometry", 3)
    nnz = T * per_pass + 1
    rows = {"one_row": ([0] * nnz, 1), "one_per_row": (list(range(nnz)), nnz)}[name]   # (as matrix_util.structures)
    _matrix_case(curves(BIG), BIG, nnz, {name: rows})


# ================================================================================================ point sets
def _strip(p):
    return {"x": p["x"], "y": p["y"], "isZero": bool(p.get("isZero", False))}


@pytest.mark.parametrize("label", ALL)
def test_points_mul(curves, label):
    """points_mul and points_mul_opts (subgroup, scalar_bits 128) over points_mul_util.build_set(label, 65): the results
    are new handles, with the endomorphism images behind them"""
    curve, params, par = curves(label), P.CURVES[label], curves(label).Parallel
    n = 65
    rows = M.build_set(label, n, 1000 * M.ALL.index(label) + n)
    pa = par.pointsFromBigints([p for _, p, _ in rows])
    qa = par.pointsFromBigints([q for _, _, q in rows])
    sa = par.scalarsFromBigints([s for s, _, _ in rows])
    want = [M.expected(params, s, p, q) for s, p, q in rows]

    def mul():
        out = par.mulPoints(sa, pa, n, addend=qa)
        got = [M.canon(params, _strip(p)) for p in curve.Affine.toBigints(out)]
        raw = _raw_points(curve, out)
        out.free()
        return got, raw
    assert under_poison(curve, mul, None, "points_mul")[0] == want
    # subgroup points (multiples of G) and scalars below 2^128
    rng = random.Random("opts" + label)
    g = U.generator(params)
    pts = [U.scale(params, rng.randrange(1, params["order"]), g) for _ in range(8)]
    pts = [pts[i % 8] for i in range(n)]
    ss = [rng.randrange(1 << 128) for _ in range(n)]
    ss[0], ss[1], ss[n - 1] = 0, (1 << 128) - 1, 1
    pb, sb = par.pointsFromBigints(pts), par.scalarsFromBigints(ss)
    want = [M.expected(params, s, p) for s, p in zip(ss, pts)]

    def mul_opts():
        out = par.mulPoints(sb, pb, n, scalarBits=128, subgroup=True)
        got = [M.canon(params, _strip(p)) for p in curve.Affine.toBigints(out)]
        raw = _raw_points(curve, out)
        out.free()
        return got, raw
    assert under_poison(curve, mul_opts, None, "points_mul_opts")[0] == want
    for a in (pa, qa, sa, pb, sb):
        a.free()


@pytest.mark.parametrize("label", ALL)
def test_points_fixed_base(mod, label):
    """the planner's width and forced width 4: poisoned before the table is built, and again before a call that the
    cache serves.  A context of its own, so that the first call does build the table."""
    params = P.CURVES[label]
    L = _lib()
    n = 257
    ss = FB.gpu_scalars(params, n, 5)
    g = U.generator(params)
    want = [FB.expected(label, s, g) for s in ss]
    with fresh(mod, label) as curve:
        par = curve.Parallel
        sa = par.scalarsFromBigints(ss)
        built = C.c_uint64(0)

        def tables():
            assert L.msmz_test_fixed_base_tables(curve._ctx, C.byref(built)) == 0
            return built.value

        def run():
            out = par.fixedBaseMul(sa)
            got = [M.canon(params, _strip(p)) for p in curve.Affine.toBigints(out)]
            raw = _raw_points(curve, out)
            out.free()
            return got, raw
        cc, K, entries = C.c_int32(0), C.c_int32(0), C.c_uint64(0)
        assert L.msmz_test_fixed_base_plan(params["curve_id"], n, 0, C.byref(cc), C.byref(K), C.byref(entries)) == 0
        first = None
        for width in (0, 4):
            assert L.msmz_test_set_fixed_base_window(curve._ctx, width) == 0
            for pat in PATTERNS:
                # a table is built by the first call of a width (unless the planner's own width is the forced one)
                new = 1 if pat == PATTERNS[0] and (width == 0 or cc.value != 4) else 0
                poison(curve, pat)
                t0 = tables()
                got = run()
                assert got[0] == want, (width, hex(pat), "built")
                assert tables() == t0 + new, (width, hex(pat))
                poison(curve, pat)
                assert run() == got, (width, hex(pat), "cached")
                assert tables() == t0 + new
                first = first or got
                assert got == first
        assert L.msmz_test_set_fixed_base_window(curve._ctx, 0) == 0


@pytest.mark.parametrize("label", ALL)
def test_check_points_and_compressed(curves, label):
    """check_points with verdict bytes over a set with planted bad points; compressed import and compressed download"""
    curve, params, par = curves(label), P.CURVES[label], curves(label).Parallel
    n = 1100
    made = par.randomPointsFast(n, 808)
    good = [_strip(p) for p in curve.Affine.toBigints(made)]
    made.free()
    pts, where = U.planted_set(label, good)
    data, inf = U.encode(params, pts)
    arr = par.pointsFromBytes(data, n, inf)
    planted = set(where)
    verdicts = [U.verdict(params, q) if i in planted else U.verdict_fast(params, q) for i, q in enumerate(pts)]
    want = U.summary(verdicts)

    def check():
        r = par.checkPoints(arr, verdicts=True)
        first = U.NO_INDEX if r.firstBad is None else r.firstBad
        return (r.offCurve, r.offSubgroup, first), r.verdicts
    got = under_poison(curve, check, None, "check_points")
    assert got[0] == want and list(got[1]) == verdicts
    arr.free()
    # compressed records in, compressed records out
    m = 257
    cpts, flags = Z.round_trip_points(label, m)
    for sign in ("largest", "parity"):
        recs = Z.records(params, cpts, flags, sign, random.Random(sign))
        want = Z.want_compressed(params, cpts, sign)

        def round_trip():
            a = par.pointsFromBytes(recs, m, flags, compressed=True, sign=sign)
            out = curve.Affine.toCompressedBytes(a, sign=sign)
            raw = _raw_points(curve, a)
            a.free()
            return out, raw
        assert under_poison(curve, round_trip, None, ("compressed", sign))[0] == want


@pytest.mark.parametrize("label", ALL)
def test_import_export_host_strided_narrow(curves, label):
    """import_* and export_* from host memory with a stride and a narrow width: the records pass through stage_ packed"""
    from msm_zprize_amd._native import MsmzDst, MsmzSrc
    curve, par, L = curves(label), curves(label).Parallel, _lib()
    n, width, stride = 257, 8, 40
    rng = random.Random("narrow" + label)
    vals = [rng.randrange(1 << 64) for _ in range(n)]
    vals[0], vals[n - 1] = (1 << 64) - 1, 0
    src_bytes = bytearray(b"\xee" * (n * stride))
    for i, v in enumerate(vals):
        src_bytes[i * stride:i * stride + width] = v.to_bytes(width, "little")
    src_buf = (C.c_char * len(src_bytes)).from_buffer(src_bytes)
    fb = curve.fe_bytes
    prow = 2 * fb + 16
    pts_arr = par.randomPointsFast(n, 606)
    xy, pinf = _raw_points(curve, pts_arr)

    def scalars():
        h = C.c_uint64(0)
        src = MsmzSrc(C.addressof(src_buf), stride, width, 0, None, None)
        assert L.msmz_import_scalars(curve._ctx, C.byref(src), n, C.byref(h)) == 0
        from msm_zprize_amd.parallel import DeviceArray
        arr = DeviceArray(curve, h.value, n, "scalars")
        got = _raw_scalars(curve, arr)
        out = C.create_string_buffer(b"\xa7" * (n * stride), n * stride)
        dst = MsmzDst(C.addressof(out), stride, width, 0, None, None)
        assert L.msmz_export_scalars(curve._ctx, arr.handle, 0, n, C.byref(dst)) == 0
        arr.free()
        return got, out.raw
    got, out = under_poison(curve, scalars, None, "scalars")
    assert got == S.encode(vals)
    for i, v in enumerate(vals):
        assert out[i * stride:i * stride + width] == v.to_bytes(width, "little"), i
        assert out[i * stride + width:(i + 1) * stride] == b"\xa7" * (stride - width), i   # between the records: untouched

    def points():
        out = C.create_string_buffer(b"\xa7" * (n * prow), n * prow)
        flags = C.create_string_buffer(b"\xa7" * n, n)
        dst = MsmzDst(C.addressof(out), prow, 2 * fb, 0, None, C.addressof(flags))
        assert L.msmz_export_points(curve._ctx, pts_arr.handle, 0, n, C.byref(dst)) == 0
        # and back in from the strided records
        h = C.c_uint64(0)
        src = MsmzSrc(C.addressof(out), prow, 2 * fb, 0, None, C.addressof(flags))
        assert L.msmz_import_points(curve._ctx, C.byref(src), n, C.byref(h)) == 0
        from msm_zprize_amd.parallel import DeviceArray
        arr = DeviceArray(curve, h.value, n, "points")
        back = _raw_points(curve, arr)
        arr.free()
        return out.raw, flags.raw, back
    out, flags, back = under_poison(curve, points, None, "points")
    assert back == (xy, pinf) and flags == pinf
    for i in range(n):
        assert out[i * prow:i * prow + 2 * fb] == xy[2 * fb * i:2 * fb * (i + 1)], i
        assert out[i * prow + 2 * fb:(i + 1) * prow] == b"\xa7" * 16, i
    pts_arr.free()


@pytest.mark.parametrize("label", ALL)
def test_generators_first_call(mod, label):
    """random_points on a context of its own, armed before anything ran: the first call builds gen_table_ in freshly
    filled memory, through a freshly filled stage_; the sets must be those of an undisturbed context, which are the
    oracle's: point i = splitmix64(seed, i) G, scalar i by rejection sampling (oracle/prng.py)"""
    from oracle import prng
    n = 300
    params = P.CURVES[label]
    g = {"x": params["generator"]["x"], "y": params["generator"]["y"], "isZero": False}
    with fresh(mod, label) as ref:
        made = ref.Parallel.randomPointsFast(n, 17)
        want_p = _raw_points(ref, made)
        want_s = _raw_scalars(ref, ref.Parallel.randomScalars(n, 18))
        got = [_pt(label, p) for p in ref.Affine.toBigints(made)]
    assert got == [_pt(label, c_oracle.scale(params, prng.point_multiplier(17, i), g)) for i in range(n)]
    assert want_s == S.encode([prng.scalar(18, i, params["order"]) for i in range(n)])
    for pat in PATTERNS:
        with fresh(mod, label) as curve:
            assert poison(curve, pat)[0] >= 1      # (meta_: the only scratch a new context holds)
            p = curve.Parallel.randomPointsFast(n, 17)
            s = curve.Parallel.randomScalars(n, 18)
            assert _raw_points(curve, p) == want_p and _raw_scalars(curve, s) == want_s, hex(pat)
            poison(curve, pat)
            assert _raw_points(curve, curve.Parallel.randomPointsFast(n, 17)) == want_p, hex(pat)


# ================================================================================================ errors under poison
@pytest.mark.parametrize("label", ALL)
def test_errors_under_poison(curves, msm_data, mod, label):
    """an error word read before it is cleared would show here: a resident scalar >= q and an MSM scalar at the
    scalar_bits bound give the unpoisoned status under every pattern, *out_handle stays untouched, and the next valid
    call is correct"""
    Err = mod._native.MsmzError
    from msm_zprize_amd._native import MsmzScalarTerm
    curve, d, par, L = curves(label), msm_data(label), curves(label).Parallel, _lib()
    q, n = d.q, N_SMALL
    xs, ys = S.build_vectors(label, n, 90)
    x, y = _upload(curve, xs), _upload(curve, ys)
    bad = _upload(curve, xs)
    _plant(curve, bad, n - 1, q)
    good_dot = sum(a * b for a, b in zip(xs, ys)) % q
    opts = {"glv": 0} if label in WEIER else {}
    short = [v % (1 << 64) for v in d.s[:n]]
    want_short = _oracle(label, short, d.big[:n])
    at_bound = list(short)
    at_bound[n // 2] = 1 << 64

    def statuses():
        out = []
        # a combine into a NEW handle with a refused record: the status, and the handle word untouched
        h = C.c_uint64(0)
        t = MsmzScalarTerm(bad.handle, 0, 0, 0, (1).to_bytes(32, "little"))
        out.append(L.msmz_scalars_combine(curve._ctx, C.byref(t), None, n, 0, C.byref(h)))
        out.append(h.value)
        buf = C.create_string_buffer(32)
        out.append(L.msmz_scalars_dot(curve._ctx, bad.handle, 0, y.handle, 0, n, buf))
        h = C.c_uint64(0)
        zeros = C.c_uint64(UNTOUCHED)
        out.append(L.msmz_scalars_inverse(curve._ctx, bad.handle, 0, n, 0, C.byref(h), C.byref(zeros)))
        out += [h.value, zeros.value]
        for sc in (bad, _enc(at_bound)):
            o = dict(opts, scalarBits=64) if sc is not bad else opts
            try:
                par.msm(sc, d.pts, n, False, o)
                out.append(0)
            except Err as e:
                out.append(e.status)
        # the next valid calls
        out.append(par.innerProduct(x, y))
        out.append(_msm(curve, label, "msm", _enc(short), d.pts, n, dict(opts, scalarBits=64))[0])
        out.append(_msm(curve, label, "msm", d.res, d.pts, n, opts)[0])
        return out
    want = [MSMZ_ERR_RANGE, 0, MSMZ_ERR_RANGE, MSMZ_ERR_RANGE, 0, UNTOUCHED, MSMZ_ERR_RANGE, MSMZ_ERR_RANGE, good_dot,
            want_short, d.want[n]]
    under_poison(curve, statuses, want, "errors")
    for a in (x, y, bad):
        a.free()


# ================================================================================================ two engines on one GPU
@pytest.mark.parametrize("label", ["bls12-377", "ed-on-bls12-377"])
def test_two_engines_on_one_gpu(mod, label):
    """devices = [0, 0], 2^16 + 5 entries: the plain MSM, scalars_inverse and points_fixed_base equal a single engine's
    under every pattern, and *buffers / *bytes are the sums over both engines"""
    n = (1 << 16) + 5
    params = P.CURVES[label]
    opts = {"glv": 0} if label in WEIER else {}

    def workload(curve, sc, pts):
        par = curve.Parallel
        r = par.msm(sc, pts, n, False, opts)["result"]
        inv, zeros = par.invertScalars(sc)
        fixed = par.fixedBaseMul(sc, N=300)
        out = (_pt(label, r), _raw_scalars(curve, inv), zeros, _raw_points(curve, fixed))
        inv.free(); fixed.free()
        return out
    with fresh(mod, label) as one:
        want = workload(one, one.Parallel.randomScalars(n, 12), one.Parallel.randomPointsFast(n, 11))
        single = poison(one, 0xa5)
    # the MSM against the closed form over the generators' multipliers, so that the yardstick is not the engine
    from oracle import prng
    t = prng.sum_of_products_mod(prng.scalars_np(12, n, params["order"]), prng.multipliers_np(11, n), params["order"])
    g = params["generator"]
    assert want[0] == _pt(label, c_oracle.scale(params, t, {"x": g["x"], "y": g["y"], "isZero": False}))
    with fresh(mod, label, devices=[0, 0]) as two:
        assert _lib().msmz_ctx_n_devices(two._ctx) == 2
        sc, pts = two.Parallel.randomScalars(n, 12), two.Parallel.randomPointsFast(n, 11)
        under_poison(two, lambda: workload(two, sc, pts), want, "two engines")
        # exactly the sum over both engines, of buffers and of bytes, against each engine's own count
        per = [scratch(two, g) for g in (0, 1)]
        total = (per[0][0] + per[1][0], per[0][1] + per[1][1])
        for pat in PATTERNS:
            assert poison(two, pat) == total, (hex(pat), per)
        assert [scratch(two, g) for g in (0, 1)] == per      # (a fill allocates nothing)
        # engine 0 holds 2^16 entries and runs what the single engine ran, on all but five of its entries.  Engine 1 holds
        # five: its MSM and its inversion still ensure meta_, the sort's refs_ and off_, sscan_ and more, in fewer bytes.
        assert single[0] + 4 <= total[0] <= 2 * single[0], (per, single)
        assert min(per[0][0], per[1][0]) >= 4 and per[0][1] > per[1][1] > 0, (per, single)
        assert per[0][1] > single[1] // 2, (per, single)
        nb, by = C.c_uint64(UNTOUCHED), C.c_uint64(UNTOUCHED)
        for engine in (2, -1):
            assert _lib().msmz_test_scratch(two._ctx, engine, C.byref(nb), C.byref(by)) == MSMZ_ERR_ARG
        # an invalid pattern leaves the outputs of a two-engine context untouched too
        for pattern in (256, -2):
            assert _lib().msmz_test_poison(two._ctx, pattern, C.byref(nb), C.byref(by)) == MSMZ_ERR_ARG, pattern
        assert (nb.value, by.value) == (UNTOUCHED, UNTOUCHED)
        assert [scratch(two, g) for g in (0, 1)] == per


# ================================================================================================ the hook itself
def test_hook_arguments(curves):
    L = _lib()
    curve = curves("pallas")
    nb, by = C.c_uint64(UNTOUCHED), C.c_uint64(UNTOUCHED)
    for pattern in (256, -2, 1 << 20, -(1 << 20)):
        assert L.msmz_test_poison(curve._ctx, pattern, C.byref(nb), C.byref(by)) == MSMZ_ERR_ARG, pattern
        assert (nb.value, by.value) == (UNTOUCHED, UNTOUCHED)
    assert L.msmz_test_poison(None, 0xa5, C.byref(nb), C.byref(by)) == MSMZ_ERR_ARG
    assert L.msmz_test_poison(None, -1, None, None) == MSMZ_ERR_ARG
    for pattern in (0, 255, -1):
        assert L.msmz_test_poison(curve._ctx, pattern, None, None) == 0
        assert L.msmz_test_poison(curve._ctx, pattern, C.byref(nb), None) == 0
        assert L.msmz_test_poison(curve._ctx, pattern, None, C.byref(by)) == 0
    assert L.msmz_test_poison(curve._ctx, -1, C.byref(nb), C.byref(by)) == 0
    assert (nb.value, by.value) == (0, 0)   # disarming fills nothing
    # msmz_test_scratch: what a fill writes, without writing it; a single engine is engine 0
    assert scratch(curve) == poison(curve, 0x5a) == scratch(curve)
    assert L.msmz_test_poison(curve._ctx, -1, None, None) == 0
    nb, by = C.c_uint64(UNTOUCHED), C.c_uint64(UNTOUCHED)
    for ctx, engine in ((curve._ctx, 1), (curve._ctx, -1), (None, 0)):
        assert L.msmz_test_scratch(ctx, engine, C.byref(nb), C.byref(by)) == MSMZ_ERR_ARG
        assert (nb.value, by.value) == (UNTOUCHED, UNTOUCHED)
    assert L.msmz_test_scratch(curve._ctx, 0, None, None) == 0


def test_disarmed_allocations_are_not_filled(mod):
    """after -1 a new allocation is no longer filled.  A fill is visible only through *buffers / *bytes of a later call,
    and through what an armed context returns for memory no kernel writes: the pad word of a check_points result record
    is never written, so nothing can be read back -- the counts are the evidence."""
    label = "pallas"
    with fresh(mod, label) as curve:
        par = curve.Parallel
        base = poison(curve, 0xa5)                 # armed: what a new context holds (meta_)
        assert base[0] >= 1 and base[1] > 0
        assert _lib().msmz_test_poison(curve._ctx, -1, None, None) == 0
        x = par.randomScalars(3000, 1)
        assert par.innerProduct(x) == sum(curve.Scalar.toBigints(x)) % S.order(label)   # sdot_ grows, disarmed
        grown = poison(curve, 0x5a)                # the fill of (a) sees the new buffer whether or not (b) filled it
        assert grown[0] == base[0] + 1 and grown[1] > base[1]
        assert poison(curve, 0x5a) == grown        # nothing ran in between: the same buffers, the same bytes


def _family_counts(mod, label, workload):
    """(buffers, bytes) of a fresh context after one workload"""
    with fresh(mod, label) as curve:
        workload(curve)
        return poison(curve, 0xa5)


def test_fill_reaches_the_buffers_of_every_family(mod):
    """*buffers is at least the number of scratch buffers the family's code path ensures, *bytes at least the sum of
    their ensure arguments for the shape: the fill is not a no-op.  Counted from the code (csrc/engine.h, sort.h,
    reduce.h, sets_core.h and the family stages that resident.h holds); the byte sums use only the terms that the shape
    fixes without the planner."""
    label = "bls12-377"
    fe = 48
    n = N_SET
    meta = 16 + 2 * 32 * 4       # MsmMeta: four words, round_pairs[32], round_base[32]
    report = {}

    def affine(curve):
        par = curve.Parallel
        par.msmUnsafe(par.randomScalars(n, 2), par.randomPointsFast(n, 1), n, False, {"glv": 0, "c": 8})
    # meta_; sort: refs_, off_, packed_, bins_, counts_, tilecnt_, tileoff_; plan: rscan_, desc_, bfin_; slots_;
    # reduction: red_[0..3], final_  (resident scalars: no stage_)
    K = -(-(253 + 1) // 8)
    nb_, by_ = report["affine MSM"] = _family_counts(mod, label, affine)
    assert nb_ >= 17
    assert by_ >= meta + 2 * K * n * 4 + (K * 128 + 1) * 4 + K * n * 8 + K * 128 * 16 + (K * n + 64) * 2 * fe

    def fallback(curve):
        par = curve.Parallel
        par.msmUnsafe(par.randomScalars(n, 2), par.randomPointsFast(n, 1), n, False, {"glv": 0, "c": 22})
    # meta_; sort: refs_, off_, digits_, counts_, cursor_, partials_; rscan_, desc_, bfin_; slots_; red_[0..3], final_
    K22 = -(-(253 + 1) // 22)
    nb_, by_ = report["affine MSM, fallback sort"] = _family_counts(mod, label, fallback)
    assert nb_ >= 16
    assert by_ >= meta + 2 * K22 * n * 4 + 3 * K22 * (1 << 21) * 4 + K22 * (1 << 21) * 16

    def basic(curve):
        par = curve.Parallel
        rng = random.Random(3)
        host = _enc([rng.randrange(P.CURVES[label]["order"]) for _ in range(700)])
        par.msmProjective(host, par.randomPointsFast(700, 1), 700, {"c": 2})
    # stage_ (host scalars), meta_; sort: refs_, off_ and five more (packed_, bins_, counts_, tilecnt_, tileoff_, or the
    # fallback's digits_, counts_, cursor_, partials_); rscan_, partials_, slots_; bsum_ (c = 2: two buckets per window,
    # ~9 accumulators each); red_[0..3], final_
    K2 = -(-(253 + 1) // 2)
    nb_, by_ = report["msmBasic, bucket sums"] = _family_counts(mod, label, basic)
    assert nb_ >= 17
    assert by_ >= 700 * 32 + meta + K2 * 700 * 4 + 2 * (K2 * 2 + 1) * 4 + K2 * 2 * 4 * fe

    def f2(curve):
        par = curve.Parallel
        par.msmUnsafe(par.randomScalars(n, 2), par.randomPointsFast(n, 1), n, False, {"glv": 0, "c": 8, "reduceAffine": 1})
    nb_, by_ = report["reduceAffine"] = _family_counts(mod, label, f2)
    assert nb_ >= 18    # as the affine MSM, and f2desc_ (red_[0], red_[1] are level_inputs', the other pair the levels')
    assert by_ >= meta + 2 * K * n * 4 + (K * n + 64 + 13 * K * 64 + 256) * 2 * fe

    two = NT.pass_log(_lib()) + 1               # the smallest transform of two passes

    def scalar_sets(curve):
        par = curve.Parallel
        x = par.randomScalars(1 << two, 1)
        par.innerProduct(x)                     # sdot_
        par.scalarRecurrence(None, x)           # sscan_
        par.ntt(x, two, nIn=(1 << two) - 3, shift=5)   # ntt_scratch_ (one copy between the two passes), ntt_coset_
    # meta_, sdot_, sscan_, ntt_scratch_, ntt_coset_
    nb_, by_ = report["scalar sets"] = _family_counts(mod, label, scalar_sets)
    assert nb_ >= 5
    assert by_ >= meta + (64 + 32) + (64 + 4 * 32) + (1 << two) * 32 + 2 * 32

    def matrix(curve):
        par = curve.Parallel
        x = par.randomScalars(64, 1)
        m = par.sparseMatrix(list(range(64)), list(range(64)), [3] * 64, (64, 64))
        par.matVec(m, x)
    # meta_, stage_ (the permutation of the values), mat_carry_
    nb_, by_ = report["matrix"] = _family_counts(mod, label, matrix)
    assert nb_ >= 3 and by_ >= meta + 2 * 64 * 4 + 9 * 4

    def points(curve):
        par = curve.Parallel
        p = par.randomPointsFast(300, 1)        # stage_ (the generator's bases)
        par.checkPoints(p)                      # check_
        curve.Affine.toBigints(p)               # stage_
    nb_, by_ = report["point sets"] = _family_counts(mod, label, points)
    assert nb_ >= 3 and by_ >= meta + 300 * 2 * fe + 16 + 300
    print("msmz_test_poison (buffers, bytes) per family:", report)

"""The host orchestration that cuts one call into several device pipelines and folds their results (csrc/engine.h):

  * index-range passes, the range loop of Engine::run_problems: inputs beyond one sort pass, every msmBasic call and
    every problem of a batch that does not batch run pass by pass, each pass with offset scalars and points (its GLV
    images behind the WHOLE set), the partial sums folded on the host (fold_partial), the logs merged;
  * sub-batches, msm_batch -> run_problems -> Planner::batch_size -> batch_split: a batch beyond the entries one batched
    pass takes runs as consecutive sub-batches.

Both limits are constants that only very large inputs reach (2^24 half-scalars, 2^26 entries), so msmz_test_set_limits
lowers them for one context and msmz_test_passes counts what ran (include/msmz_test.h).  Every expected point comes from
the C oracle or from the closed form over randomPointsFast multipliers, never from the engine; every lowered-limit call
is also compared with the same call at the built-in limits, and the counters prove that the split path was taken."""
import ctypes as C
import math
import random
from contextlib import contextmanager

import pytest

from oracle import c_oracle
from oracle import params as P
from oracle import prng

pytestmark = pytest.mark.gpu

WEIER = ["bls12-377", "pallas", "bls12-381"]
ALL = WEIER + ["ed-on-bls12-377"]
MSMZ_ERR_ARG, MSMZ_ERR_DEGENERATE, MSMZ_ERR_RANGE = 1, 5, 6
N, SET, PASS = 2500, 4000, 1000


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


def _oracle(label, scalars, points):
    return _pt(label, c_oracle.msm(P.CURVES[label], scalars, points))


def _neg(label, p):
    m = P.CURVES[label]["modulus"]
    if label in WEIER:
        return {"x": p["x"], "y": (m - p["y"]) % m, "isZero": False}
    return {"x": (m - p["x"]) % m, "y": p["y"]}


def passes(curve):
    from msm_zprize_amd._native import lib
    rp, sb = C.c_uint64(), C.c_uint64()
    assert lib().msmz_test_passes(curve._ctx, C.byref(rp), C.byref(sb)) == 0
    return rp.value, sb.value


@contextmanager
def limits(curve, pass_entries=0, batch_entries=0):
    """the two limits lowered for the calls inside, the built-in ones restored whatever happens"""
    from msm_zprize_amd._native import lib
    assert lib().msmz_test_set_limits(curve._ctx, pass_entries, batch_entries) == 0
    try:
        yield
    finally:
        assert lib().msmz_test_set_limits(curve._ctx, 0, 0) == 0


def split_run(curve, call, pass_entries=0, batch_entries=0, unsplit=None):
    """call() at the built-in limits, then at the lowered ones: the results must be identical.  -> (result, range passes
    and sub-batches the lowered call added).  unsplit: the call that runs at the built-in limits, if another"""
    base = (unsplit or call)()
    with limits(curve, pass_entries, batch_entries):
        r0, s0 = passes(curve)
        got = call()
        r1, s1 = passes(curve)
    assert got == base, "the lowered limits changed a result"
    return got, r1 - r0, s1 - s0


class Data:
    """One curve's shared inputs: a resident set of SET device-generated points, its first N as a set of their own (the
    same points: point i depends on the seed and i only), N random scalars as host bytes and resident, and the oracle's
    MSM of them, computed once."""

    def __init__(self, mod, label):
        self.label, self.c = label, P.CURVES[label]
        self.q = self.c["order"]
        self.curve = _create(mod, label)
        par = self.curve.Parallel
        self.set = par.randomPointsFast(SET, 1234)
        self.pts = par.randomPointsFast(N, 1234)
        self.big = self.curve.Affine.toBigints(self.set)
        rng = random.Random("limits" + label)
        self.s = [rng.randrange(self.q) for _ in range(N)]
        self.s[0], self.s[PASS - 1], self.s[PASS], self.s[N - 1] = self.q - 1, 1, self.q - 2, self.q - 1   # pass edges
        self.host = _enc(self.s)
        self.res = par.scalarsFromBytes(self.host, N)
        self.want = _oracle(label, self.s, self.big[:N])

    def close(self):
        self.curve.close()


@pytest.fixture(scope="module")
def data(mod):
    cache = {}

    def get(label):
        if label not in cache:
            cache[label] = Data(mod, label)
        return cache[label]

    yield get
    for d in cache.values():
        d.close()


def _variants(label):
    """(name, function, options, GLV) of every MSM variant of a curve"""
    if label not in WEIER:
        return [("msm c=0", "msm", {}, 0), ("msm c=6", "msm", {"c": 6}, 0)]
    v = [(f"msmUnsafe glv={g}", "msmUnsafe", {"glv": g}, g) for g in (0, 1)]
    v += [(f"msm glv={g} c={c}", "msm", {"glv": g, "c": c}, g) for g in (0, 1) for c in (0, 7)]
    v += [("msmProjective", "msmProjective", {}, 0)]
    v += [(f"reduceAffine glv={g}", "msmUnsafe", {"glv": g, "reduceAffine": 1}, g) for g in (0, 1)]
    return v


def _call(curve, label, fn, scalars, pts, n, opts, verbose=False):
    if fn == "msmProjective":
        r = curve.Parallel.msmProjective(scalars, pts, n, dict(opts))
    else:
        r = getattr(curve.Parallel, fn)(scalars, pts, n, verbose, dict(opts))
    return _pt(label, r["result"]), r["stats"]


# ------------------------------------------------------------------------------------------------ 1. passes, every variant
@pytest.mark.parametrize("pass_entries", [1000, 2048, 2499, 2500])
@pytest.mark.parametrize("label", ALL)
def test_passes_every_variant(data, label, pass_entries):
    """n = 2500 in ragged passes (1000), a pass that ends off a sort tile (2048), a last pass of one point (2499) and
    exactly one pass (2500): every variant equals the oracle, resident and host scalars, and ran ceil(n / P) passes
    (P // 2 points per pass with GLV)"""
    d = data(label)
    for name, fn, opts, glv in _variants(label):
        per = pass_entries // 2 if glv else pass_entries
        for sc in (d.res, d.host):
            got, rp, sb = split_run(d.curve, lambda: _call(d.curve, label, fn, sc, d.pts, N, opts)[0], pass_entries)
            assert got == d.want, (name, pass_entries)
            assert (rp, sb) == (math.ceil(N / per), 0), (name, pass_entries)


# ------------------------------------------------------------------------------------------------ 2. GLV over a prefix
@pytest.mark.parametrize("label", WEIER)
def test_glv_prefix_in_passes(data, label):
    """the first 2500 points of a resident set of 4000, GLV, 500 points per pass: every pass reads its endomorphism
    images behind the WHOLE set (an image base of n, of the pass length or of the pass start gives another point)"""
    d = data(label)
    for fn, opts in (("msmUnsafe", {"glv": 1}), ("msm", {"glv": 1}), ("msm", {"glv": 1, "c": 7}),
                     ("msmUnsafe", {"glv": 1, "reduceAffine": 1})):
        got, rp, sb = split_run(d.curve, lambda: _call(d.curve, label, fn, d.res, d.set, N, opts)[0], PASS)
        assert got == d.want, (fn, opts)
        assert (rp, sb) == (5, 0), (fn, opts)


# ------------------------------------------------------------------------------------------------ 3. the fold's edge cases
FOLD_LAYOUTS = {   # blocks of points (+1: A, -1: -A), blocks of scalars (1: the vector s, 0: zeros)
    "A A -A: a doubling, then 2S - S": ((1, 1, -1), (1, 1, 1)),
    "A -A A: infinity, then infinity + S": ((1, -1, 1), (1, 1, 1)),
    "A A A, zero scalars first": ((1, 1, 1), (0, 1, 1)),
    "A A A, zero scalars in the middle": ((1, 1, 1), (1, 0, 1)),
    "A -A, then zero scalars: infinity": ((1, -1, 1), (1, 1, 0)),
}


@pytest.mark.parametrize("label", ALL)
def test_fold_edge_cases(data, label):
    """three passes of 512 uploaded points whose partial sums are equal, opposite or infinity: fold_partial adds S + S,
    S + (-S), infinity + S and S + infinity on the host.  (Unsafe additions: every pass holds distinct points, but in ONE
    pass equal and opposite points with equal scalars share their buckets, which msmUnsafe rightly refuses; the unsplit
    call it is compared with is therefore the one with safe additions.)"""
    d = data(label)
    blk = 512
    A = [dict(p) for p in d.big[:blk]]
    nA = [_neg(label, p) for p in A]
    rng = random.Random("fold" + label)
    s = [rng.randrange(d.q) for _ in range(blk)]
    fns = ("msm", "msmUnsafe") if label in WEIER else ("msm",)
    for name, (pblocks, sblocks) in FOLD_LAYOUTS.items():
        points = [p for b in pblocks for p in (A if b > 0 else nA)]
        scalars = [v for b in sblocks for v in (s if b else [0] * blk)]
        want = _oracle(label, scalars, points)
        if name.endswith("infinity"):
            assert want == ((0, 1, True) if label in WEIER else (0, 1, False))
        pts = d.curve.Parallel.pointsFromBigints(points)
        host = _enc(scalars)
        try:
            for fn in fns:
                opts = {"glv": 0} if label in WEIER else {}
                got, rp, sb = split_run(d.curve, lambda: _call(d.curve, label, fn, host, pts, 3 * blk, opts)[0], blk,
                                        unsplit=lambda: _call(d.curve, label, "msm", host, pts, 3 * blk, opts)[0])
                assert got == want, (name, fn)
                assert (rp, sb) == (3, 0), (name, fn)
        finally:
            pts.free()


# ------------------------------------------------------------------------------------------------ 4. errors in a later pass
@pytest.mark.parametrize("label", ALL)
def test_error_in_a_later_pass_then_usable(data, mod, label):
    """a scalar equal to the group order in pass 3 (pass 5 with GLV), a scalar at a scalarBits bound in pass 2, and (unsafe
    additions) two equal points with equal scalars in pass 3: the call fails with the status an unsplit call gives, and
    the same context then returns the oracle's result for the clean inputs, still in passes"""
    Err = mod._native.MsmzError
    d = data(label)
    par = d.curve.Parallel
    weier = label in WEIER
    with limits(d.curve, PASS):
        for glv in ((0, 1) if weier else (0,)):
            opts = {"glv": glv} if weier else {}
            bad = list(d.s)
            bad[2400] = d.q
            with pytest.raises(Err) as e:
                par.msm(_enc(bad), d.pts, N, False, opts)
            assert e.value.status == MSMZ_ERR_RANGE
            assert _call(d.curve, label, "msm", d.host, d.pts, N, opts)[0] == d.want
        # a bound of 64 bits
        rng = random.Random("bound" + label)
        short = [rng.randrange(1 << 64) for _ in range(N)]
        want = _oracle(label, short, d.big[:N])
        bad = list(short)
        bad[1500] = 1 << 64
        for glv in ((0, 1) if weier else (0,)):
            opts = dict({"glv": glv} if weier else {}, scalarBits=64)
            res = par.scalarsFromBytes(_enc(bad), N)
            try:
                for sc in (_enc(bad), res):
                    with pytest.raises(Err) as e:
                        par.msm(sc, d.pts, N, False, opts)
                    assert e.value.status == MSMZ_ERR_RANGE
            finally:
                res.free()
            assert _call(d.curve, label, "msm", _enc(short), d.pts, N, opts)[0] == want
        if weier:
            # two equal points with equal scalars, alone in their bucket in most windows of c = 16
            points = [dict(p) for p in d.big[:N]]
            points[2300] = dict(points[2100])
            scalars = list(d.s)
            scalars[2300] = scalars[2100]
            pts = par.pointsFromBigints(points)
            opts = {"glv": 0, "c": 16}
            try:
                with pytest.raises(Err) as e:
                    par.msmUnsafe(_enc(scalars), pts, N, False, opts)
                assert e.value.status == MSMZ_ERR_DEGENERATE
                r0 = passes(d.curve)[0]
                assert _call(d.curve, label, "msmUnsafe", d.host, d.pts, N, opts)[0] == d.want
                assert passes(d.curve)[0] - r0 == 3
                # (the safe additions take the same inputs)
                assert _call(d.curve, label, "msm", _enc(scalars), pts, N, opts)[0] == _oracle(label, scalars, points)
            finally:
                pts.free()


# ------------------------------------------------------------------------------------------------ 5. short scalars
@pytest.mark.parametrize("bound", [64, 130])
@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_short_scalars_in_passes(data, label, bound):
    """a scalar bit bound sizes the windows of every pass: oracle == bounded == unbounded, in three (GLV: five) passes"""
    d = data(label)
    rng = random.Random(f"short{label}{bound}")
    s = [rng.randrange(1 << bound) for _ in range(N)]
    s[0], s[PASS], s[N - 1] = (1 << bound) - 1, (1 << bound) - 1, 1 << (bound - 1)
    want = _oracle(label, s, d.big[:N])
    host = _enc(s)
    for glv in (0, 1):
        for fn in ("msm", "msmUnsafe"):
            for opts in ({"glv": glv, "scalarBits": bound}, {"glv": glv}):
                got, rp, sb = split_run(d.curve, lambda: _call(d.curve, label, fn, host, d.pts, N, opts)[0], PASS)
                assert got == want, (glv, fn, opts)
                assert (rp, sb) == (5 if glv else 3, 0), (glv, fn, opts)


# ------------------------------------------------------------------------------------------------ 6. a batch beyond a pass
@pytest.mark.parametrize("label", WEIER)
def test_batch_whose_n_exceeds_a_pass(data, label):
    """msmBatch of 3 vectors of 2500 scalars with 1000 per pass: no batched pipeline, every problem in three passes"""
    d = data(label)
    B = 3
    rng = random.Random("batch" + label)
    vecs = [d.s] + [[rng.randrange(d.q) for _ in range(N)] for _ in range(B - 1)]
    want = [d.want] + [_oracle(label, v, d.big[:N]) for v in vecs[1:]]
    host = [_enc(v) for v in vecs]
    res = d.curve.Parallel.scalarsFromBytes(b"".join(host), B * N)
    try:
        for fn in (d.curve.Parallel.msmBatch, d.curve.Parallel.msmBatchUnsafe):
            for sc in (host, res):
                call = lambda: [_pt(label, r) for r in fn(sc, d.pts, N, {"glv": 0})]
                got, rp, sb = split_run(d.curve, call, PASS)
                assert got == want
                assert (rp, sb) == (9, 0)
    finally:
        res.free()


# ------------------------------------------------------------------------------------------------ 7. sub-batch splits
def batch_split(remaining, entries_per_problem, cap):
    """csrc/multi.h batch_split: at most cap entries per sub-batch, the problems dealt into equally large sub-batches"""
    fit = max(cap // entries_per_problem, 1)
    if fit >= remaining:
        return remaining
    parts = -(-remaining // fit)
    return -(-remaining // parts)


def split_sizes(B, entries_per_problem, cap):
    sizes, remaining = [], B
    while remaining:
        sizes.append(batch_split(remaining, entries_per_problem, cap))
        remaining -= sizes[-1]
    return sizes


class BatchData:
    """17 vectors of 257 scalars over 257 points of BLS12-377, the oracle's results and a loop of single MSMs"""
    n, Bmax, label = 257, 17, "bls12-377"

    def __init__(self, d):
        rng = random.Random("sub-batches")
        self.vecs = [[rng.randrange(d.q) for _ in range(self.n)] for _ in range(self.Bmax)]
        self.short = [[rng.randrange(1 << 64) for _ in range(self.n)] for _ in range(self.Bmax)]
        self.want = [_oracle(self.label, v, d.big[:self.n]) for v in self.vecs]
        self.want_short = [_oracle(self.label, v, d.big[:self.n]) for v in self.short]


@pytest.fixture(scope="module")
def batch_data(data):
    return BatchData(data(BatchData.label))


def _batch(d, vecs, pts, n, opts, unsafe=True):
    f = d.curve.Parallel.msmBatchUnsafe if unsafe else d.curve.Parallel.msmBatch
    return [_pt(d.label, r) for r in f([_enc(v) for v in vecs], pts, n, dict(opts))]


def test_split_sizes_mirror():
    """the mirror of batch_split gives the documented deal (64 problems with room for 40: 2 x 32) and the sequences the
    tests below expect"""
    assert batch_split(64, 1, 40) == 32 and batch_split(5, 10, 9) == 1 and batch_split(0, 1, 1) == 0
    assert split_sizes(5, 7, 7) == [1] * 5 and split_sizes(5, 7, 14) == [2, 2, 1] and split_sizes(5, 7, 28) == [3, 2]
    assert split_sizes(17, 7, 14) == [2] * 8 + [1] and split_sizes(17, 7, 28) == [4, 4, 3, 3, 3]
    assert split_sizes(17, 7, 112) == [9, 8] and split_sizes(17, 7, 119) == [17] and split_sizes(5, 7, 112) == [5]


@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("B", [5, 17])
def test_sub_batch_splits(data, batch_data, B, glv):
    """user c = 8, caps of 1, 2, 4, 16 and B problems' entries: the sub-batch sizes are batch_split's, a sub-batch of one
    problem runs the range loop, every result equals the oracle and a loop of single MSMs"""
    d, bd = data(BatchData.label), batch_data
    n = bd.n
    vecs, want = bd.vecs[:B], bd.want[:B]
    opts = {"glv": glv, "c": 8}
    assert _batch(d, vecs, d.pts, n, opts) == want
    K = d.curve.Parallel.lastBatchLog.K
    M = n * (2 if glv else 1)
    assert K == -(-((127 if glv else 253) + 1) // 8)   # (BLS12-377: 253-bit scalars, 127-bit GLV halves)
    loop = [_call(d.curve, d.label, "msmUnsafe", _enc(v), d.pts, n, opts)[0] for v in vecs]
    assert loop == want
    for fit in (1, 2, 4, 16, B):
        cap = fit * K * M + (K * M - 1 if fit != 1 else 0)   # cap // (K M) = fit, not a multiple of K M
        sizes = split_sizes(B, K * M, cap)
        assert sum(sizes) == B and max(sizes) <= fit
        for unsafe in (True, False):
            got, rp, sb = split_run(d.curve, lambda: _batch(d, vecs, d.pts, n, opts, unsafe), 0, cap)
            assert got == want, (fit, unsafe)
            assert sb == sum(1 for s in sizes if s > 1), (fit, sizes)
            assert rp == sum(1 for s in sizes if s == 1), (fit, sizes)


def test_sub_batch_split_variations(data, batch_data):
    """default c (the window size follows the sub-batch size), precomputed sets with all windows in one bucket set and
    with two per set, a scalar bit bound, and a GLV redo of whole sub-batches: the oracle's results from more than one
    pipeline"""
    from msm_zprize_amd._native import lib
    d, bd = data(BatchData.label), batch_data
    n, B = bd.n, bd.Bmax
    par = d.curve.Parallel

    def check(vecs, want, pts, opts, M):
        assert _batch(d, vecs, pts, n, opts) == want
        cap = 2 * par.lastBatchLog.K * M
        got, rp, sb = split_run(d.curve, lambda: _batch(d, vecs, pts, n, opts), 0, cap)
        assert got == want, opts
        assert rp + sb > 1, opts

    for glv in (0, 1):
        check(bd.vecs, bd.want, d.pts, {"glv": glv}, n << glv)
        check(bd.short, bd.want_short, d.pts, {"glv": glv, "c": 8, "scalarBits": 64}, n << glv)
        for factor in (0, 2):
            pre = par.precomputePoints(d.pts, n, {"glv": glv, "c": 8}, factor)
            try:
                check(bd.vecs, bd.want, pre, {}, n << glv)
            finally:
                pre.free()
    retries = lib().msmz_test_retries(d.curve._ctx)
    assert lib().msmz_test_set_glv_bits(d.curve._ctx, 100) == 0
    try:
        check(bd.vecs, bd.want, d.pts, {"glv": 1, "c": 8}, 2 * n)
    finally:
        assert lib().msmz_test_set_glv_bits(d.curve._ctx, 0) == 0
    assert lib().msmz_test_retries(d.curve._ctx) >= retries + 2   # (the unsplit batch once, every sub-batch once)


# ------------------------------------------------------------------------------------------------ 8. multi-engine
def _closed_form(label, pseed, sseed, n):
    c = P.CURVES[label]
    t = prng.sum_of_products_mod(prng.scalars_np(sseed, n, c["order"]), prng.multipliers_np(pseed, n), c["order"])
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    return _pt(label, c_oracle.scale(c, t, gen))


@pytest.mark.parametrize("label", ["bls12-377", "ed-on-bls12-377"])
def test_multi_engine_passes(mod, label):
    """three engines on one GPU, 3 x 65536 + 1000 points in blocks of 2^16: the limit reaches every engine, each runs
    its share in passes of 20000 entries, and the counters are summed over the engines"""
    from msm_zprize_amd.sharding import block_shard_count
    n, G, per = 3 * 65536 + 1000, 3, 20000
    want = _closed_form(label, 61, 62, n)
    mod.startThreads(devices=[0])
    one = _create(mod, label)
    mod.startThreads(devices=[0] * G)
    multi = _create(mod, label)
    mod.startThreads()
    try:
        p1, s1 = one.Parallel.randomPointsFast(n, 61), one.Parallel.randomScalars(n, 62)
        pm, sm = multi.Parallel.randomPointsFast(n, 61), multi.Parallel.randomScalars(n, 62)
        for glv in ((0, 1) if label in WEIER else (0,)):
            fn, opts = ("msmUnsafe", {"glv": glv}) if label in WEIER else ("msm", {})
            assert _call(one, label, fn, s1, p1, n, opts)[0] == want
            got, rp, sb = split_run(multi, lambda: _call(multi, label, fn, sm, pm, n, opts)[0], per)
            assert got == want, glv
            pp = per // 2 if glv else per
            assert (rp, sb) == (sum(math.ceil(block_shard_count(n, g, G) / pp) for g in range(G)), 0), glv
    finally:
        one.close()
        multi.close()


# ------------------------------------------------------------------------------------------------ 9. logs
@pytest.mark.parametrize("label", ["bls12-377", "ed-on-bls12-377"])
def test_logs_of_a_call_in_passes(data, label):
    """merge_log(SEQUENTIAL) over three passes: the digits do not depend on the split, so n_entries is the one-pass
    call's; c is the caller's; the stage times are sums of finite times; the longest bucket is no longer than in one
    pass"""
    d = data(label)
    variants = [("msmUnsafe", {"glv": 0}), ("msmUnsafe", {"glv": 1}), ("msmProjective", {})] if label in WEIER else \
        [("msm", {})]
    for fn, o in variants:
        opts = dict(o, c=9)
        got1, one = _call(d.curve, label, fn, d.res, d.pts, N, opts, True)
        one = (one.n_entries, one.max_bucket, one.K, one.glv)
        with limits(d.curve, PASS):
            r0 = passes(d.curve)[0]
            got, log = _call(d.curve, label, fn, d.res, d.pts, N, opts, True)
            assert passes(d.curve)[0] - r0 == (5 if o.get("glv") else 3)
        assert got == got1 == d.want, fn
        assert log.c == 9 and (log.K, log.glv) == one[2:], fn
        assert log.n_entries == one[0] and 0 < log.max_bucket <= one[1], fn
        assert all(math.isfinite(t) and t >= 0 for t in log.stage_ms), list(log.stage_ms)
        assert all(math.isfinite(t) and t >= 0 for t in log.batch_add_ms), list(log.batch_add_ms)


# ------------------------------------------------------------------------------------------------ 10. hook arguments
def test_hook_arguments(data):
    from msm_zprize_amd._native import lib
    L = lib()
    d = data("pallas")
    ctx = d.curve._ctx
    rp, sb = C.c_uint64(), C.c_uint64()
    try:
        for pe, be in ((1, 0), ((1 << 24) + 1, 0), (0, (1 << 26) + 1), ((1 << 64) - 1, 0), (0, (1 << 64) - 1)):
            assert L.msmz_test_set_limits(ctx, pe, be) == MSMZ_ERR_ARG, (pe, be)
        assert L.msmz_test_set_limits(None, 1000, 1000) == MSMZ_ERR_ARG
        assert L.msmz_test_passes(None, C.byref(rp), C.byref(sb)) == MSMZ_ERR_ARG
        for pe, be in ((2, 1), (1 << 24, 1 << 26), (1000, 0), (0, 1000)):
            assert L.msmz_test_set_limits(ctx, pe, be) == 0, (pe, be)
        assert L.msmz_test_passes(ctx, None, None) == 0
        assert L.msmz_test_passes(ctx, C.byref(rp), None) == 0 and L.msmz_test_passes(ctx, None, C.byref(sb)) == 0
        assert (rp.value, sb.value) == passes(d.curve)
        te = data("ed-on-bls12-377")
        try:
            assert L.msmz_test_set_limits(te.curve._ctx, 1000, 1000) == 0
        finally:
            assert L.msmz_test_set_limits(te.curve._ctx, 0, 0) == 0
        # a refused call leaves the limits as they were: (0, 1000) from above, then the built-in ones
        assert L.msmz_test_set_limits(ctx, 100, 0) == 0 and L.msmz_test_set_limits(ctx, 1, 0) == MSMZ_ERR_ARG
        r0 = passes(d.curve)[0]
        assert _call(d.curve, "pallas", "msm", d.host, d.pts, 300, {"glv": 0})[0] == _oracle("pallas", d.s[:300], d.big[:300])
        assert passes(d.curve)[0] - r0 == 3
        assert L.msmz_test_set_limits(ctx, 0, 0) == 0
        for c in (d, te):
            r0, s0 = passes(c.curve)
            opts = {"glv": 0} if c.label in WEIER else {}
            want = _oracle(c.label, c.s[:300], c.big[:300])
            assert _call(c.curve, c.label, "msm", c.host, c.pts, 300, opts)[0] == want
            assert passes(c.curve) == (r0 + 1, s0)
    finally:
        assert L.msmz_test_set_limits(ctx, 0, 0) == 0

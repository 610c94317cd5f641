"""The tree-round schedule alone (k_plan_count / k_plan_emit of csrc/plan_kernels.h) through msmz_test_plan
(csrc/test_hooks.h -> Engine::plan_phase), on caller-built buckets, against oracle/schedule_ref.py.

A whole MSM shows the schedule through one result point, and which of its paths run -- the one-thread-per-pair rounds
below PLAN_RL = 6 with their 4096-pair owner tiles, the bucket-by-bucket rounds above with their running pair numbers in
global scratch, the second bucket of a thread, the strided chunk sums beyond 512 chunks, the empty-chunk exit, the
main / top split -- is an accident of its bucket histogram.  Here the histogram is the input.  The stage is pure
integers, so every comparison is exact: the descriptors the device wrote are replayed symbolically
(schedule_ref.expand: every record becomes a range of positions of one bucket, every record is consumed exactly once,
operands precede their launch, bfin tiles each bucket) and compared, round by round, with the reference's in-place rule
(schedule_ref.reference_round, msm-batched-affine.ts:232-247), in the bucket-by-bucket numbering the consumers rely on.
References carry a distinct index per entry and random negate bits, so every original word is decidable.  A failure
names case, tail_skip, round, pair, bucket and the chunk (workgroup) that owns the bucket.

Mutations run against this module on an MI355X (one at a time, values only, each in a scratch build of msmz.hip,
`pytest -x`) and the first test that failed:
  (a) location(): `rr > r - 1` -> `rr > r`
        test_schedule[max-3]: tail_skip=0, round 1, pair 0, bucket 0 (size 3, chunk 0): operand A is record 1010, not
        below round 1's base 1010 (the pair reads its own record)
  (b) location(): `pos >> (rr + 1)` -> `pos >> rr`
        test_schedule[max-4]: tail_skip=0, round 1, pair 0, bucket 1 (size 4, chunk 0): operands from buckets 1 and 7
  (c) k_plan_emit: `b < blockIdx.x` -> `b <= blockIdx.x` in the `pre` sum
        test_schedule[max-2]: tail_skip=0, round 0, pair 0, bucket 0 (chunk 0): the descriptor was never written (it
        still holds the hook's fill pattern; the chunk wrote one chunk further)
  (d) k_plan_emit: the `s_pair[...] += pairs_in_round(sz, r)` advance skipped for q = 0
        test_schedule[pow2-7]: tail_skip=0, round 6, pair 5, bucket 11 (size 127, chunk 0): never written (the thread's
        second bucket wrote over its first one's pairs)
  (e) k_plan_emit: fin.w from `2u << R`
        test_schedule[nb-1-size-64]: tail_skip=2, bucket 0 (size 64): record 58 = positions [32, 48) consumed twice
  (f) k_plan_emit: the negate bit of r1 dropped in the round-0 fast path
        test_schedule[max-2]: tail_skip=0, round 0, pair 1, operand B: negate bit 0 on entry 5 (bucket 5, position 1),
        refs has 1
  (g) k_plan_count: tail_skip ignored
        test_schedule[max-3]: tail_skip=1: chunk_pairs of round 1, chunk 0 (buckets 0 .. 1023) = 207, expected 0

Measured on one MI355X in one visit: this module 10 s (111 tests; the 2^24-entry bucket 4 s of it), the rest of
the `-m gpu` suite 133 s (675 passed, 1 skipped).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import schedule_ref as SR

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED = 1, 4      # include/msmz.h
PLAN_T, PLAN_PER, PLAN_CHUNK, PLAN_RMAX, PLAN_RL, PLAN_TILE = 512, 2, 1024, 26, 6, 4096   # csrc/plan.h, plan_kernels.h
N = SR.LOC_NONE


# --------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def ctxs():
    import msm_zprize_amd as m
    m.startThreads()
    cache = {}

    def get(label):
        if label not in cache:
            params = m.curves.BY_LABEL[label]
            cache[label] = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
        return cache[label]

    yield get
    for c in cache.values():
        c.close()


def _native():
    from msm_zprize_amd import _native
    return _native


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def plan(curve, off, refs, chunk, nb_main, chunk_top, tail_skip, desc_cap=None, bfin_cap=None, cp_cap=None,
         want_chunk_pairs=True, nb=None, null=()):
    """msmz_test_plan.  Returns (status, meta words, desc, bfin, chunk_pairs or None); capacities default to what the
    buckets need by schedule_ref's count."""
    nt = _native()
    off = np.ascontiguousarray(off, dtype=np.uint32)
    refs = np.ascontiguousarray(refs, dtype=np.uint32)
    nb = len(off) - 1 if nb is None else nb
    sizes = np.diff(off.astype(np.int64))
    ok_sizes = len(sizes) > 0 and sizes.min() >= 0
    R = SR.plan_rounds(int(sizes.max()), tail_skip) if ok_sizes and 0 <= tail_skip <= 2 else 0
    total = sum(int(SR.pairs_in_round(sizes, r).sum()) for r in range(min(R, PLAN_RMAX))) if ok_sizes else 0
    n_main = -(-nb_main // max(chunk, 1))
    n_chunks = n_main + -(-max(nb - nb_main, 0) // max(chunk_top, 1))
    desc_cap = total if desc_cap is None else desc_cap
    bfin_cap = nb if bfin_cap is None else bfin_cap
    cp_cap = PLAN_RMAX * n_chunks if cp_cap is None else cp_cap
    meta = np.zeros(SR.META_WORDS, dtype=np.uint32)
    desc = np.zeros((max(desc_cap, 1), 2), dtype=np.uint32)
    bfin = np.zeros((max(bfin_cap, 1), 4), dtype=np.uint32)
    cp = np.zeros(max(cp_cap, 1), dtype=np.uint32) if want_chunk_pairs else None
    a = nt.MsmzTestPlanArgs(nb=nb, chunk=chunk, nb_main=nb_main, chunk_top=chunk_top, tail_skip=tail_skip, reserved=0,
                            off=_ptr(off), refs=_ptr(refs), desc_cap=desc_cap, bfin_cap=bfin_cap, chunk_pairs_cap=cp_cap,
                            meta=_ptr(meta), desc=_ptr(desc), bfin=_ptr(bfin), chunk_pairs=_ptr(cp))
    for name in null:
        setattr(a, name, None)
    st = nt.lib().msmz_test_plan(curve._ctx, C.byref(a))
    return (st, meta, desc[:total], bfin[:nb],
            cp[:PLAN_RMAX * n_chunks].reshape(PLAN_RMAX, n_chunks) if want_chunk_pairs and cp_cap >= PLAN_RMAX * n_chunks else None)


class Geo:
    """PlanChunks (csrc/plan.h) of a launch: buckets [0, nb_main) in chunks of `chunk`, the rest in chunks of chunk_top"""

    def __init__(self, chunk=PLAN_CHUNK, nb_main=None, chunk_top=None):
        self.chunk, self.nb_main, self.chunk_top = chunk, nb_main, chunk_top

    def resolve(self, nb):
        nb_main = nb if self.nb_main is None else self.nb_main
        return self.chunk, nb_main, self.chunk if self.chunk_top is None else self.chunk_top

    def __repr__(self):
        return f"chunk={self.chunk} nb_main={self.nb_main} chunk_top={self.chunk_top}"


def chunk_starts(nb, chunk, nb_main, chunk_top):
    return np.concatenate([np.arange(0, nb_main, chunk), np.arange(nb_main, nb, chunk_top)]).astype(np.int64)


def make_refs(n, rng):
    """a distinct index per entry (a permutation of 0 .. n-1) and random negate bits"""
    return rng.permutation(n).astype(np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31))


def check(curve, name, sizes, geo, tail_skip, rng, refs=None):
    """One run of the hook on buckets of `sizes`, every assertion of the module; returns (meta, desc, bfin)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    nb = len(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    refs = make_refs(n, rng) if refs is None else refs
    chunk, nb_main, chunk_top = geo.resolve(nb)
    starts = chunk_starts(nb, chunk, nb_main, chunk_top)
    n_chunks = len(starts)
    tag = f"{name} tail_skip={tail_skip} nb={nb} chunk={chunk} nb_main={nb_main} chunk_top={chunk_top} n_chunks={n_chunks}"

    def where(bucket):
        w = int(np.searchsorted(starts, bucket, side="right") - 1)
        return f"bucket {int(bucket)} (size {int(sizes[bucket])}, chunk {w}, bucket {int(bucket - starts[w])} of it)"

    st, mwords, desc, bfin, cp = plan(curve, off, refs, chunk, nb_main, chunk_top, tail_skip)
    assert st == 0, f"{tag}: status {st}"
    meta = SR.parse_meta(mwords)
    mx = int(sizes.max())
    R = SR.plan_rounds(mx, tail_skip)
    per_round = [SR.pairs_in_round(sizes, r) for r in range(R)]
    want_pairs = np.array([int(p.sum()) for p in per_round] + [0] * (32 - R), dtype=np.int64)
    want_base = np.concatenate([[0], np.cumsum(want_pairs)])[:32]
    total = int(want_pairs.sum())
    print(f"{tag}: max {mx} rounds {meta['rounds']} (want {R}) entries {meta['n_entries']} pairs "
          f"{meta['round_pairs'][:max(R, 1)].tolist()}")
    assert meta["max_bucket"] == mx and meta["error"] == 0, f"{tag}: meta {meta}"
    assert meta["rounds"] == R, f"{tag}: rounds {meta['rounds']}, plan_rounds({mx}, {tail_skip}) = {R}"
    assert meta["n_entries"] == n, f"{tag}: n_entries {meta['n_entries']}, off[nb] = {n}"
    # the per-chunk table first: it says which chunk miscounted which round
    ends = np.concatenate([starts[1:], [nb]])
    want_cp = np.zeros((PLAN_RMAX, n_chunks), dtype=np.int64)
    for r in range(R):
        c = np.concatenate([[0], np.cumsum(per_round[r])])
        want_cp[r] = c[ends] - c[starts]
    if not np.array_equal(cp, want_cp):
        r, w = np.argwhere(cp != want_cp)[0]
        pytest.fail(f"{tag}: chunk_pairs of round {r}, chunk {w} (buckets {starts[w]} .. {ends[w] - 1}) = {cp[r, w]}, "
                    f"expected {want_cp[r, w]}")
    for r in range(32):
        assert meta["round_pairs"][r] == want_pairs[r], (f"{tag}: round_pairs[{r}] = {meta['round_pairs'][r]}, the "
                                                         f"reference adds {want_pairs[r]} pairs in round {r}")
        assert meta["round_base"][r] == want_base[r], f"{tag}: round_base[{r}] = {meta['round_base'][r]}, expected {want_base[r]}"

    try:
        ex = SR.expand(desc, bfin, meta, off, refs)
    except SR.ScheduleError as e:
        b = e.bucket
        if b is None and e.round is not None and e.pair is not None:   # the bucket the numbering gives this pair
            b = int(np.searchsorted(np.cumsum(per_round[e.round]), e.pair, side="right"))
        fill = " [0xa5a5a5a5: the word was never written]" if e.record == 0xA5A5A5A5 else ""
        pytest.fail(f"{tag}: {e}{fill}" + (f" -- {where(b)}" if b is not None and b < nb else ""))

    for r in range(R):
        g, pa, pb = SR.reference_round(sizes, r)
        sl = slice(int(want_base[r]), int(want_base[r] + want_pairs[r]))
        got = (ex.rec_bucket[sl], ex.rec_lo[sl], ex.rec_mid[sl])
        if not all(np.array_equal(x, y) for x, y in zip(got, (g, pa, pb))):
            # the same additions in another order, or other additions?
            same = all(np.array_equal(x[np.lexsort(got[::-1])], y) for x, y in zip(got, (g, pa, pb)))
            t = _first_diff(got, (g, pa, pb))
            pytest.fail(f"{tag}: round {r}, pair {t} (desc[{want_base[r]} + {t}]) adds position {got[2][t]} into "
                        f"{got[1][t]} of bucket {got[0][t]}; "
                        + ("the round's additions are the reference's, but pairs are not numbered bucket by bucket: "
                           if same else "the reference's round differs: ")
                        + f"pair {t} is {pb[t]} into {pa[t]} of {where(g[t])}")
        hi = np.minimum(pa + (2 << r), sizes[g])
        if not np.array_equal(ex.rec_hi[sl], hi):
            t = int(np.flatnonzero(ex.rec_hi[sl] != hi)[0])
            pytest.fail(f"{tag}: round {r}, pair {t}: the record stands for positions [{pa[t]}, {ex.rec_hi[sl][t]}), "
                        f"expected [{pa[t]}, {hi[t]}) of {where(g[t])}")
    want_fin = -(-sizes // (1 << R))
    assert want_fin.max(initial=0) <= 4
    if not np.array_equal(ex.fin_count, want_fin):
        b = int(np.flatnonzero(ex.fin_count != want_fin)[0])
        pytest.fail(f"{tag}: bfin holds {ex.fin_count[b]} locations, expected ceil(size / 2^{R}) = {want_fin[b]}: {where(b)}")
    # (expand has checked that they tile 0 .. size-1 in order; with the count, location k starts at k 2^R)
    assert np.array_equal(ex.fin_lo % (1 << R), np.zeros_like(ex.fin_lo)), tag
    assert total == len(desc)
    return meta, desc, bfin


def _first_diff(a, b):
    return int(np.flatnonzero((a[0] != b[0]) | (a[1] != b[1]) | (a[2] != b[2]))[0])


# --------------------------------------------------------------------------------------------------- cases
def mixed(rng, nb, pool, p_empty=0.2):
    s = rng.choice(np.asarray(pool, dtype=np.int64), size=nb)
    s[rng.random(nb) < p_empty] = 0
    return s


def _pow2(k):
    def f(rng):
        pat = [(1 << k) - 1, 0, 1 << k, 1, (1 << k) + 1, 0, 0, 1, 1, 1 << k, (1 << k) + 1, (1 << k) - 1]
        return np.concatenate([np.array(pat), mixed(rng, 700, [0, 1, 2, 3, 5]), np.array(pat[::-1])])
    return f


def _with(nb, base_pool, **at):
    """small random buckets with given sizes at given places; keys are 'i<index>'"""
    def f(rng):
        s = mixed(rng, nb, base_pool)
        for k, v in at.items():
            s[int(k[1:])] = v
        return s
    return f


def _two_per_thread(kind):
    def f(rng):
        s = mixed(rng, 2 * PLAN_CHUNK + 301, [0, 1, 2, 3, 9])
        long = lambda: int(rng.integers(65, 700))
        for t in range(0, 2 * PLAN_CHUNK + 300, 2):       # buckets t, t + 1 belong to one thread (chunks are even)
            if rng.random() < 0.15:
                s[t], s[t + 1] = {"long-long": (long(), long()), "long-empty": (long(), 0), "empty-long": (0, long())}[kind]
        s[-1] = long()                                   # the last thread of the last chunk owns one bucket
        return s
    return f


def _empty_chunks(where):
    def f(rng):
        c = 256
        s = mixed(rng, 12 * c + 5, [0, 1, 2, 3, 70, 200])
        for w in {"middle": (3, 4, 7), "end": (10, 11, 12), "first": (0,), "first-two-and-middle": (0, 1, 5)}[where]:
            s[w * c:(w + 1) * c] = 0
        return s
    return f


def _tile(kind):
    def f(rng):
        if kind == "dense":            # rounds 0 and 1 of every chunk beyond 4096 pairs, buckets across the tile edges
            return rng.integers(9, 40, size=3 * PLAN_CHUNK)
        if kind == "one-bucket":       # one bucket alone: 20000, 10000, 5000 pairs in rounds 0, 1, 2
            s = mixed(rng, 1500, [0, 1, 2, 5, 33])
            s[700] = 40000
            return s
        if kind == "exact-4096":
            return np.full(PLAN_CHUNK, 8)
        if kind == "exact-4097":
            s = np.full(PLAN_CHUNK, 8)
            s[513] = 10
            return s
        if kind == "single-4096":      # one bucket of exactly 4096 round-0 pairs, and of 4097 with its neighbour's one
            s = np.zeros(2 * PLAN_CHUNK, dtype=np.int64)
            s[5] = 8192
            s[PLAN_CHUNK + 7], s[PLAN_CHUNK + 8] = 8192, 2
            return s
    return f


def _seam(mx):
    def f(rng):
        pool = [x for x in (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 600, 1025) if x <= mx]
        s = mixed(rng, 1300, pool, p_empty=0.1)
        s[rng.integers(0, 1300)] = mx
        return s
    return f


def _geometry(nb, seed_pool=(0, 0, 1, 2, 3, 4, 7, 8, 9, 33, 64, 65, 130)):
    return lambda rng: mixed(rng, nb, seed_pool)


def _long(n_long, nb=5000, size=(1 << 20) + 1):
    def f(rng):
        s = mixed(rng, nb, [0, 1, 2, 3, 5, 8])
        for i in range(n_long):
            s[1500 + 2049 * i] = size
        return s
    return f


ALL_TS = (0, 1, 2)
CASES = []   # (id, sizes builder(rng), Geo, tail_skips)


def case(cid, build, geo=None, ts=ALL_TS):
    CASES.append(pytest.param(build, geo or Geo(), ts, id=cid))


# degenerate
case("all-empty", lambda rng: np.zeros(3000, dtype=np.int64))
case("all-single", lambda rng: np.ones(3000, dtype=np.int64))
for _mx in (2, 3, 4):
    case(f"max-{_mx}", lambda rng, m=_mx: mixed(rng, 2500, list(range(m + 1))))
for _s in (0, 1, 2, 3, 5, 64, 300, 5000):
    case(f"nb-1-size-{_s}", lambda rng, s=_s: np.array([s]))
# every power of two
for _k in range(1, 13):
    case(f"pow2-{_k}", _pow2(_k))
# the seam at PLAN_RL: with tail_skip 0 .. 2 these maxima give 5 .. 11 rounds, so round 6 is absent, the last, the first
# bucket-by-bucket round and an inner one; from 257 on location() reads pair numbers of rounds >= PLAN_RL from the scratch
for _mx in (32, 33, 64, 65, 128, 129, 256, 257, 1025):
    case(f"seam-max-{_mx}", _seam(_mx))
# owner tile
for _kind in ("dense", "one-bucket", "exact-4096", "exact-4097", "single-4096"):
    case(f"tile-{_kind}", _tile(_kind))
# two buckets per thread
for _kind in ("long-long", "long-empty", "empty-long"):
    case(f"per-thread-{_kind}", _two_per_thread(_kind))
case("per-thread-odd-nbk-chunk-64", _with(64 * 3 + 31, [0, 1, 2, 70], i222=300, i221=0, i220=90), Geo(64))
# chunk geometry
for _c in (64, 128, 256, 512, 1024):
    for _d in (-1, 0, 1):
        case(f"chunk-{_c}-nb-{'4c%+d' % _d if _d else '4c'}", _geometry(4 * _c + _d), Geo(_c))
    if _c >= 128:
        for _K, _L in ((4, 256), (2, 1024), (3, 2048)):
            case(f"chunk-{_c}-top-split-K{_K}-L{_L}", _geometry(_K * _L), Geo(_c, (_K - 1) * _L, _c // 2))
        # a short last main chunk, and a short last top chunk
        case(f"chunk-{_c}-top-split-short-main", _geometry(5 * _c + _c // 4 + 3 * (_c // 2) + 5),
             Geo(_c, 5 * _c + _c // 4, _c // 2))
case("chunk-edge-long-last-and-first", _with(4 * 256, [0, 1, 2, 3], i255=500, i256=700, i511=129, i512=4097, i1023=66), Geo(256))
case("chunk-edge-long-top-split", _with(2 * 1024, [0, 1, 2, 3], i1023=500, i1024=700, i1151=300, i1152=301, i2047=90),
     Geo(256, 1024, 128))
for _w in ("middle", "end", "first", "first-two-and-middle"):
    case(f"empty-chunks-{_w}", _empty_chunks(_w), Geo(256))
case("empty-chunks-top-split", _empty_chunks("first-two-and-middle"), Geo(256, 8 * 256, 128))
case("chunks-513", _with(64 * 513, [0, 0, 0, 1, 2, 5], i0=70, i32831=300, i32767=65, i32768=64), Geo(64))
case("chunks-1100", _with(64 * 1100 - 3, [0, 0, 0, 1, 2, 5], i3=129, i40000=1000, i65535=70, i65536=257, i70396=66), Geo(64))
case("chunks-1025-top-split", _with(1024 * 64 + 32, [0, 0, 1, 3], i65535=100, i65536=200, i65567=90), Geo(64, 1023 * 64 + 20, 32))
# long buckets
case("long-2^20+1", _long(1))
case("long-2^20+1-twice", _long(2))
case("long-2^24", _long(1, nb=2000, size=1 << 24), ts=(0, 1))

SHORT = {"seam-max-257", "tile-dense", "tile-single-4096", "per-thread-long-long", "chunk-256-top-split-K4-L256",
         "empty-chunks-first-two-and-middle", "chunks-513", "pow2-7", "all-empty", "long-2^20+1"}
SHORT_CASES = [c for c in CASES if c.id in SHORT]
assert len(SHORT_CASES) == len(SHORT)


def _run_case(ctxs, label, request, build, geo, tss):
    import zlib
    seed = zlib.crc32(request.node.callspec.id.encode())
    curve = ctxs(label)
    for ts in tss:
        rng = np.random.default_rng(seed)
        check(curve, request.node.callspec.id, build(rng), geo, ts, rng)


@pytest.mark.parametrize("build,geo,tss", CASES)
def test_schedule(ctxs, request, build, geo, tss):
    _run_case(ctxs, "bls12-377", request, build, geo, tss)


@pytest.mark.parametrize("label", ["pallas", "bls12-381"])
@pytest.mark.parametrize("build,geo,tss", SHORT_CASES)
def test_schedule_other_contexts(ctxs, request, label, build, geo, tss):
    """the plan kernels are not templated on the field; their launch sits in every engine's instantiation"""
    _run_case(ctxs, label, request, build, geo, tss)


# --------------------------------------------------------------------------------------------------- real histograms
def _sort(curve, scalars_raw, n, c, glv):
    lib = _native().lib()
    geom = (C.c_uint32 * 8)()
    assert lib.msmz_test_sort(curve._ctx, scalars_raw, n, c, glv, 0, geom, None, 0, None, 0) == 0
    cc, K, Keff, L, nb, E, maxb, spread = list(geom)
    off = np.zeros(nb + 1, dtype=np.uint32)
    refs = np.zeros(max(E, 1), dtype=np.uint32)
    assert lib.msmz_test_sort(curve._ctx, scalars_raw, n, c, glv, 0, geom, _ptr(off), nb + 1, _ptr(refs), max(E, 1)) == 0
    return dict(c=cc, K=K, Keff=Keff, L=L, nb=nb, E=E, maxb=maxb), off, refs[:E]


@pytest.mark.parametrize("label,c,glv,lgn", [("bls12-377", 16, 1, 17), ("bls12-377", 17, 0, 18), ("pallas", 16, 0, 18)],
                         ids=["bls12-377-c16-glv", "bls12-377-c17", "pallas-c16"])
def test_real_histograms(ctxs, label, c, glv, lgn):
    """off / refs as the sort leaves them for random scalars, planned with chunk = 1024 and the top window's bucket sets
    split off at (K - 1) L.  The sort's references repeat an index in every window, which no replay can place; so the
    schedule is checked on the sort's buckets and negate bits with the entry number as index, and the run on the sort's
    own references must then be that schedule word for word, with every original word's index mapped back."""
    from oracle import params as P
    curve = ctxs(label)
    q = P.CURVES[label]["order"]
    rng = np.random.default_rng(1000 * c + glv)
    n = 1 << lgn
    words = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64)
    raw = b"".join((int.from_bytes(w.astype("<u4").tobytes(), "little") % q).to_bytes(32, "little") for w in words)
    g, off, refs = _sort(curve, raw, n, c, glv)
    assert g["c"] == c and g["E"] == int(off[-1])
    sizes = np.diff(off.astype(np.int64))
    nb_main = (g["K"] - 1) * g["L"]
    assert nb_main <= g["nb"]
    for chunk_top in (512,):
        geo = Geo(1024, nb_main, chunk_top)
        for ts in ALL_TS:
            own = (refs & np.uint32(0x80000000)) | np.arange(len(refs), dtype=np.uint32)
            name = f"real-{label}-c{c}-glv{glv}-top{chunk_top}"
            meta, desc, bfin = check(curve, name, sizes, geo, ts, rng, refs=own)
            st, mw, d2, b2, _ = plan(curve, off, refs, 1024, nb_main, chunk_top, ts)
            assert st == 0 and np.array_equal(mw, np.concatenate([[meta["max_bucket"], meta["n_entries"], 0, meta["rounds"]],
                                                                  meta["round_pairs"], meta["round_base"]]))

            def back(w):
                orig = ((w & SR.LOC_ORIG) != 0) & (w != N)
                e = np.where(orig, w & SR.LOC_IDX, 0)
                return np.where(orig, (refs[e] & np.uint32(0xBFFFFFFF)) | np.uint32(SR.LOC_ORIG), w)

            assert np.array_equal(d2, back(desc)), f"{name} tail_skip={ts}: desc differs on the sort's own references"
            assert np.array_equal(b2, back(bfin)), f"{name} tail_skip={ts}: bfin differs on the sort's own references"


# --------------------------------------------------------------------------------------------------- rejections
def test_hook_rejects_bad_arguments(ctxs):
    """everything that could index outside an array is refused before any launch (statuses only), and the context still
    plans a good case afterwards"""
    curve = ctxs("bls12-377")
    rng = np.random.default_rng(3)
    sizes = np.array([3, 0, 1, 70, 2, 9] * 50, dtype=np.int64)
    nb = len(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    refs = make_refs(int(off[-1]), rng)
    good = dict(off=off, refs=refs, chunk=128, nb_main=nb, chunk_top=128, tail_skip=1)

    def status(**kw):
        return plan(curve, **{**good, **kw})[0]

    assert status() == 0
    lib = _native().lib()
    assert lib.msmz_test_plan(None, None) == MSMZ_ERR_ARG and lib.msmz_test_plan(curve._ctx, None) == MSMZ_ERR_ARG
    for name in ("off", "refs", "meta", "desc", "bfin"):
        assert status(null=(name,)) == MSMZ_ERR_ARG, name
    assert status(nb=0) == MSMZ_ERR_ARG
    assert status(nb=(1 << 22) + 1) == MSMZ_ERR_ARG      # (refused on nb alone: off is not read)
    bad = off.copy()
    bad[0] = 1
    assert status(off=bad) == MSMZ_ERR_ARG
    bad = off.copy()
    bad[7] = bad[6] - 1
    assert status(off=bad) == MSMZ_ERR_ARG
    assert status(off=np.array([0, (1 << 25) + 1], dtype=np.uint32), refs=refs, nb_main=1, desc_cap=8) == MSMZ_ERR_ARG
    # (a bucket of 2^26 entries needs off[nb] > 2^25: the entry cap refuses it first, so PLAN_RMAX cannot be exceeded)
    assert status(off=np.array([0, 1 << 26], dtype=np.uint32), refs=refs, nb_main=1, desc_cap=8) == MSMZ_ERR_ARG
    bad = refs.copy()
    bad[len(bad) // 2] |= np.uint32(0x40000000)
    assert status(refs=bad) == MSMZ_ERR_ARG
    for chunk in (0, PLAN_CHUNK + 1):
        assert status(chunk=chunk, chunk_top=1) == MSMZ_ERR_ARG, chunk
    for chunk_top in (0, 129):
        assert status(chunk_top=chunk_top) == MSMZ_ERR_ARG, chunk_top
    assert status(nb_main=nb + 1) == MSMZ_ERR_ARG
    for ts in (-1, 3):
        assert status(tail_skip=ts) == MSMZ_ERR_ARG, ts
    R = SR.plan_rounds(70, 1)
    total = sum(int(SR.pairs_in_round(sizes, r).sum()) for r in range(R))
    n_chunks = -(-nb // 128)
    assert status(desc_cap=total - 1) == MSMZ_ERR_ARG
    assert status(bfin_cap=nb - 1) == MSMZ_ERR_ARG
    assert status(cp_cap=PLAN_RMAX * n_chunks - 1) == MSMZ_ERR_ARG
    assert status(desc_cap=total, bfin_cap=nb, cp_cap=PLAN_RMAX * n_chunks) == 0
    assert status(want_chunk_pairs=False, cp_cap=0) == 0          # optional output left out
    te = ctxs("ed-on-bls12-377")
    assert plan(te, **good)[0] == MSMZ_ERR_UNSUPPORTED
    check(curve, "after-rejections", sizes, Geo(128), 1, rng)

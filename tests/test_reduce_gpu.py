"""The bucket reduction alone (BucketReduce of csrc/reduce.h: run_2d's two halves and levels; the kernels of
csrc/reduce2d_kernels.h and csrc/kernels.h) through msmz_test_reduce (csrc/test_hooks.h), on caller-built buckets, stage by stage against oracle/bigint_ref.py.

A whole MSM shows the reduction only through one point: which level kernel ran is decided by thresholds a release
build cannot move, every bucket sum of a large MSM is a distinct random point, and the row / column result of a bucket
set disappears in the host's Horner sum.  Here every bucket holds a small multiple m G, so the expectation of every
line sum and of every problem's weighted sum is known in the exponent (bigint_ref.reduce_multiples_2d, pinned against
the group computation in tests/test_oracle.py) and costs one scalar multiplication; equal, opposite and neutral
operands are placed on purpose; and the hook's arguments force k_reduce_quad / k_reduce_quad16, k_pairsum /
k_pairsum_x4 and k_reduce_tail at every shape.  Comparison is bit-exact on canonical affine coordinates.  A failure
names curve, mode, c, NC, thresholds, problem (set, rows / columns) and, for line sums, the line.

Mutations run against this module on an MI355X (one at a time, values only -- no address, bound or guard of a load or
store changes --, each in a scratch build, `pytest -x`) and the first test that failed:
  (a) xyzz_add_x4: the `!dbl && fe_is_zero(P)` branch never taken (P = Q undetected on the generic lanes)
        test_geometry[bls12-377-locations]: c=5 sets=1 NC=4, WEIGHTED SUM wrong, all line sums right, problems 0, 1
  (b) k_reduce2d_partial / _acc (since then one place, r2_chunk's `fold`): the `line == g.H / 2` fold of the weight-L
      bucket moved to line 0
        test_geometry[bls12-377-locations]: c=2, LINE SUM wrong in problem 0 (rows), lines 0 and 1
  (c) k_reduce2d_partial_acc: the look-ahead one bucket too early, `range(i + 1, ...)` -> `range(i, ...)`
        test_geometry[bls12-377-accs]: c=2, LINE SUM wrong in problem 1 (columns), line 0
  (d) k_fill_neutral storing an all-zero record (not a point on twisted Edwards)
        test_geometry[ed-on-bls12-377-accs]: c=2, WEIGHTED SUM wrong, all line sums right (Weierstrass runs pass)
  (e) k_reduce_quad: lane table of step 3 {0, 3, 1, 3} -> {0, 3, 3, 3}
        test_level_kernels_forced[bls12-377-locations]: c=2 tail_n=1 quad16_max=1, WEIGHTED SUM wrong in the row
        problems (test_geometry passes: the default thresholds never reach k_reduce_quad)

Measured on one MI355X in one visit: this module 36 s (210 tests), the rest of the `-m gpu` suite 41 s (382 passed,
1 skipped).  One default 2^20 BLS12-377 MSM (c = 17) under `rocprofv3 --kernel-trace` launches k_reduce2d_partial x1,
k_pairsum x3, k_pairsum_x4 x2, k_fill_neutral x1, k_reduce_quad16 x2, k_reduce_tail x1 and never k_reduce_quad.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import bigint_ref as BR
from oracle import params as P

pytestmark = pytest.mark.gpu

LOCS, ACCS, SUMMED, LEVELS = 0, 1, 2, 3           # MSMZ_TR_* (include/msmz_test.h)
MODE_NAMES = ["locations", "accs", "accs+bucket_sums", "levels"]
LOC_ORIG, LOC_NEG, LOC_NONE = 0x40000000, 0x80000000, 0xFFFFFFFF
MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6   # include/msmz.h
WEIER = ["bls12-377", "pallas", "bls12-381"]
ALL = WEIER + ["ed-on-bls12-377"]
MODES_OF = {label: ([LOCS] if label in WEIER else []) + [ACCS, SUMMED] for label in ALL}
CURVE_MODES = [(l, m) for l in ALL for m in MODES_OF[l]]
CM_IDS = [f"{l}-{MODE_NAMES[m]}" for l, m in CURVE_MODES]
# every window size on BLS12-377; on the other curves the shapes that differ in kind: H = 2 (c = 2, 3), even and odd
# splits (H = D and H = 2 D), levels ending in a group of two (odd ceil((c-1)/2)) and the largest
CS_OF = {"bls12-377": list(range(2, 13)) + [16], "pallas": [2, 3, 4, 5, 8, 11, 16], "bls12-381": [2, 3, 6, 7, 10, 16],
         "ed-on-bls12-377": [2, 3, 4, 5, 6, 9, 12, 16]}
# ... and for the degenerate contents (every kind of content on every curve, fewer window sizes per curve)
CS_CONTENTS = {"bls12-377": [2, 3, 4, 5, 6, 8, 9], "pallas": [2, 5, 8], "bls12-381": [3, 4, 9], "ed-on-bls12-377": [2, 6, 9]}
N_DEGENERATE = {"bls12-377": [2, 3, 4, 7, 16, 31, 33, 64, 100], "pallas": [3, 7, 16, 33], "bls12-381": [2, 4, 31, 64],
                "ed-on-bls12-377": [3, 7, 33, 100]}
NP = 1 << 12                  # pool: k G for |k| <= NP + 512
POOL = NP + 512
# level selection: (tail_n, quad16_max, pairsum_x4_max); 0 = the engine's (32, 8192, 16384).  quad16_max = 1 sends every
# level above the tail to k_reduce_quad, pairsum_x4_max = 1 every pair-sum launch to k_pairsum; tail 4096 > H: the tail
# kernel does every level; tail 1: it only copies C.
DEFAULT = (0, 0, 0)
KERNELS = [(t, q, p) for t in (1, 4, 32, 4096) for q in (1, 1 << 20) for p in (1, 1 << 20)]
FEW = [DEFAULT, (1, 1, 1), (1, 1 << 20, 1 << 20), (4, 1, 1 << 20), (4096, 0, 1)]


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


class Pool:
    """k G for |k| <= POOL as canonical affine rows (row POOL + k), and enc(k) for any k by one scalar multiplication"""

    def __init__(self, label):
        prm = P.CURVES[label]
        self.label, self.fb, self.q, self.p = label, prm["fe_bytes"], prm["order"], prm["modulus"]
        self.te = prm["kind"] != "weierstrass"
        fb = self.fb
        rows = np.zeros((2 * POOL + 1, 2 * fb), dtype=np.uint8)
        if self.te:
            E = self.E = BR.TwistedEdwards(prm)
            self.zero_row = np.frombuffer((0).to_bytes(fb, "little") + (1).to_bytes(fb, "little"), dtype=np.uint8)
            acc, pts = E.zero, []
            for _ in range(POOL):
                acc = E.add(acc, E.one)
                pts.append(acc)
            # one inversion for all of them (Montgomery's trick)
            pref, run = [], 1
            for X in pts:
                pref.append(run)
                run = run * X[2] % self.p
            inv = BR.inverse(run, self.p)
            for k in range(POOL - 1, -1, -1):
                zi = inv * pref[k] % self.p
                inv = inv * pts[k][2] % self.p
                x, y = pts[k][0] * zi % self.p, pts[k][1] * zi % self.p
                rows[POOL + k + 1] = self._row(x, y)
                rows[POOL - k - 1] = self._row((-x) % self.p, y)
        else:
            A = BR.AffineWeierstrass(prm)
            self.E = BR.ProjectiveWeierstrass(prm)
            self.zero_row = np.zeros(2 * fb, dtype=np.uint8)
            acc = A.zero
            for k in range(POOL):
                acc = A.add(acc, A.one)
                rows[POOL + k + 1] = self._row(acc[0], acc[1])
                rows[POOL - k - 1] = self._row(acc[0], (-acc[1]) % self.p)
        rows[POOL] = self.zero_row
        self.rows = rows
        self.memo = {}

    def _row(self, x, y):
        return np.frombuffer(x.to_bytes(self.fb, "little") + y.to_bytes(self.fb, "little"), dtype=np.uint8)

    def enc(self, k):
        k %= self.q
        if k <= POOL:
            return self.rows[POOL + k]
        if self.q - k <= POOL:
            return self.rows[POOL - (self.q - k)]
        if k not in self.memo:
            R = self.E.scale(k, self.E.one)
            if self.te:
                self.memo[k] = self._row(*self.E.to_affine(R))
            else:
                a = self.E.to_affine(R)
                self.memo[k] = self.zero_row if a[2] else self._row(a[0], a[1])
        return self.memo[k]

    def enc_many(self, ks):
        return np.stack([self.enc(int(k)) for k in ks]) if len(ks) else np.zeros((0, 2 * self.fb), np.uint8)

    def take(self, ks):
        """rows of small multiples (|k| <= POOL), vectorized"""
        ks = np.asarray(ks, dtype=np.int64)
        assert np.abs(ks).max(initial=0) <= POOL
        return self.rows[ks + POOL]


_pools = {}


def pool(label):
    if label not in _pools:
        _pools[label] = Pool(label)
    return _pools[label]


def _lib():
    from msm_zprize_amd import _native
    return _native.lib()


def call(curve, **kw):
    """msmz_test_reduce; array arguments as numpy arrays / bytes.  Returns (status, results, lines)."""
    from msm_zprize_amd import _native
    a = _native.MsmzTestReduceArgs()
    keep = []

    def buf(x):
        if x is None:
            return None
        b = x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()
        keep.append(b)
        return b

    def arr(x, dt):
        if x is None:
            return None
        x = np.ascontiguousarray(x, dtype=dt)
        keep.append(x)
        return x.ctypes.data

    fb = kw["fb"]
    for name in ("mode", "c", "nsets", "n_in", "nc", "tail_n", "quad16_max", "pairsum_x4_max", "n_points", "n_slots"):
        setattr(a, name, int(kw.get(name, 0)))
    for name in ("points_xy", "points_inf", "slots_xy", "slots_inf", "scale"):
        setattr(a, name, buf(kw.get(name)))
    a.loc = arr(kw.get("loc"), np.uint32)
    a.cscan = arr(kw.get("cscan"), np.uint32)
    n_res = kw.get("n_res", 64)
    n_lines = kw.get("n_lines", 0)
    out = np.full((n_res, 2 * fb), 0xEE, dtype=np.uint8)
    lines = np.full((max(n_lines, 1), 2 * fb), 0xEE, dtype=np.uint8)
    a.out_xy = out.ctypes.data
    a.lines_xy = lines.ctypes.data if n_lines else None
    st = _lib().msmz_test_reduce(curve._ctx, C.byref(a))
    return st, out, lines[:n_lines]


def scales(pl, n, seed):
    """n distinct field elements != 0, 1 as canonical bytes"""
    v = (np.arange(n, dtype=np.int64) * 7919 + seed) % 65521 + 2
    out = np.zeros((n, pl.fb), dtype=np.uint8)
    out[:, 0] = v & 0xFF
    out[:, 1] = (v >> 8) & 0xFF
    out[:, 2] = v >> 16
    return out


# --------------------------------------------------------------------------------------------------- 2-D cases
def split(c):
    H, D = BR.split_2d(c)
    return 1 << (c - 1), H, D


def default_nc(c, nsets):
    """Planner::split_2d's automatic chunks per line"""
    L, H, D = split(c)
    nc = 1
    while nc < 32 and nc * 2 <= D and 2 * nsets * H * nc < (1 << 18):
        nc *= 2
    return nc


def ncs(c, nsets):
    _, _, D = split(c)
    return sorted({1, min(2, D), D, 0}, key=lambda v: (v == 0, v))   # 0 = default, last


def encode_locations(pl, m, variant=0):
    """bucket multiples m (flat, |m| <= NT - 16) as location words: 1 .. 4 locations per bucket whose sum is m, point /
    negated point / slot record / infinity slot / infinity point in every position, LOC_NONE in every position with
    live-looking words behind it (the loader stops at the first).  Point i of the table = (i + 1) G for i < NT, point NT =
    infinity (flagged); slot i = (i + 1) G, slot NT + i = -(i + 1) G, slot 2 NT = infinity."""
    nb = len(m)
    NT = int(np.abs(m).max(initial=0)) + 16
    g = np.arange(nb, dtype=np.int64)

    def pt(k):
        k = np.asarray(k, dtype=np.int64)
        w = np.where(k > 0, LOC_ORIG | (k - 1), np.where(k < 0, LOC_ORIG | LOC_NEG | (-k - 1), LOC_ORIG | NT))
        return np.where((k == 0) & (g & 1 == 1), w | LOC_NEG, w)        # (a negated infinity is still infinity)

    def slot(k):
        k = np.asarray(k, dtype=np.int64)
        return np.where(k > 0, k - 1, np.where(k < 0, NT + (-k - 1), 2 * NT))

    a = (g * 5 + variant) % 7 - 3          # small offsets, zero included
    b = (g * 3 + variant) % 5 - 2
    half = m // 2
    even = m % 2 == 0
    NONE = np.full(nb, LOC_NONE, dtype=np.int64)
    junk = pt(np.full(nb, 7))              # behind a LOC_NONE: must never be read
    pats = [
        [pt(m), NONE, junk, junk],
        [slot(m), NONE, junk, NONE],
        [pt(a), slot(m - a), NONE, junk],
        [slot(a), pt(b), pt(m - a - b), NONE],
        [pt(a), slot(b), pt(-a), slot(m - b)],
        [np.where(even, pt(half), pt(m)), np.where(even, pt(half), NONE), NONE, junk],   # the same point twice
        [slot(0), pt(m), NONE, junk],
        [slot(m), slot(0), pt(0), NONE],
        [pt(0), slot(a), pt(0), slot(m - a)],
        [np.where(even, slot(half), slot(m)), np.where(even, pt(half), NONE), NONE, NONE],  # slot + the same point
        [pt(a), pt(-a), slot(m), NONE],
    ]
    # empty buckets: no location at all, or only infinities / a cancelling pair
    zero_pats = [[NONE, junk, junk, junk], [slot(0), NONE, junk, junk], [pt(3), pt(-3), NONE, junk], [pt(0), slot(0), pt(0), slot(0)]]
    sel = (g + variant) % len(pats)
    zsel = (g // 3 + variant) % len(zero_pats)
    loc = np.zeros((nb, 4), dtype=np.int64)
    for i in range(4):
        col = np.select([sel == k for k in range(len(pats))], [p[i] for p in pats])
        zcol = np.select([zsel == k for k in range(len(zero_pats))], [p[i] for p in zero_pats])
        loc[:, i] = np.where(m == 0, zcol, col)
    pts_xy = np.concatenate([pl.take(np.arange(1, NT + 1)), np.zeros((1, 2 * pl.fb), np.uint8)])
    slots_xy = np.concatenate([pl.take(np.arange(1, NT + 1)), pl.take(-np.arange(1, NT + 1)), np.zeros((1, 2 * pl.fb), np.uint8)])
    return dict(points_xy=pts_xy, points_inf=bytes(NT) + b"\1", n_points=NT + 1, slots_xy=slots_xy,
                slots_inf=bytes(2 * NT) + b"\1", n_slots=2 * NT + 1, loc=loc.astype(np.uint32))


def encode_accs(pl, m, cnt, lam):
    """bucket multiples m as cnt[g] accumulator records each (cnt = 0 only where m = 0): small filler multiples (zero =
    a neutral record among them) and a last record that completes the sum"""
    nb = len(m)
    assert not np.any((cnt == 0) & (m != 0))
    cscan = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    n = int(cscan[-1])
    bucket = np.repeat(np.arange(nb, dtype=np.int64), cnt)
    i = np.arange(n, dtype=np.int64) - cscan[bucket]
    fill = (bucket * 31 + i * 17) % 23 - 11
    last = i == cnt[bucket] - 1
    fill[last] = 0
    done = np.bincount(bucket, weights=fill, minlength=nb).astype(np.int64) if n else np.zeros(nb, np.int64)
    vals = fill.copy()
    vals[last] = (m - done)[bucket[last]]
    kw = dict(points_xy=pl.take(vals), n_points=n, cscan=cscan.astype(np.uint32))
    if lam:
        kw["scale"] = scales(pl, n, lam)
    return kw


def counts(nb, L, style):
    """chunk accumulators per bucket.  'one': the plain msmBasic shape.  'mixed': 0, 1, 2, 3 cycling with period 7 (odd:
    every position of every chunk of a line meets every count) and 40 every 97th bucket."""
    g = np.arange(nb, dtype=np.int64)
    if style == "one":
        return np.ones(nb, dtype=np.int64)
    cnt = np.array([1, 0, 2, 1, 3, 1, 2], dtype=np.int64)[g % 7]
    cnt[g % 97 == 5] = 40
    l = g % L
    if style == "edges_empty":        # first bucket, last bucket before L, the weight-L bucket: empty ranges
        cnt[(l == 0) | (l == L - 2) | (l == L - 1)] = 0
    elif style == "edges_long":       # ... and with several chunks
        cnt[(l == 0) | (l == L - 2)] = 2
        cnt[l == L - 1] = 40
    return cnt


def run_2d(ctxs, label, mode, c, nsets, m, nc=0, kern=DEFAULT, what="", cnt_style="mixed", lam=0, variant=0):
    """one call on bucket multiples m[nsets][L]; compares every line sum and every result with the oracle"""
    pl = pool(label)
    L, H, D = split(c)
    m = np.asarray(m, dtype=np.int64).reshape(nsets, L).copy()
    if mode == LOCS:
        kw = encode_locations(pl, m.reshape(-1), variant)
    else:
        cnt = counts(nsets * L, L, cnt_style)
        m.reshape(-1)[cnt == 0] = 0
        kw = encode_accs(pl, m.reshape(-1), cnt, lam)
    tail, quad, pair = kern
    st, out, lines = call(ctxs(label), fb=pl.fb, mode=mode, c=c, nsets=nsets, nc=nc, tail_n=tail, quad16_max=quad,
                          pairsum_x4_max=pair, n_res=2 * nsets, n_lines=2 * nsets * H, **kw)
    nc_eff = nc or default_nc(c, nsets)
    tag = (f"{label} {MODE_NAMES[mode]} c={c} (L={L} H={H} D={D}) sets={nsets} NC={nc_eff}{'' if nc else ' (default)'} "
           f"tail_n={tail} quad16_max={quad} pairsum_x4_max={pair} [{what}; chunks={cnt_style} lambda={lam}]")
    assert st == 0, f"{tag}: status {st}"
    want_lines, want_res = [], []
    for s in range(nsets):
        rows, cols, rr, cr = BR.reduce_multiples_2d([int(v) for v in m[s]], c, pl.q)
        want_lines += rows + cols
        want_res += [rr, cr]
    wl = pl.enc_many(want_lines)
    bad = np.nonzero((wl != lines).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        prob, line = divmod(i, H)
        pytest.fail(f"{tag}: LINE SUM wrong in problem {prob} (set {prob // 2}, {'columns' if prob & 1 else 'rows'}), line "
                    f"{line}: expected {want_lines[i]} G; {len(bad)} of {len(wl)} line sums differ "
                    f"(first lines: {[divmod(int(b), H) for b in bad[:8]]})")
    wr = pl.enc_many(want_res)
    bad = np.nonzero((wr != out).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        pytest.fail(f"{tag}: WEIGHTED SUM wrong (all line sums right) in problem {i} (set {i // 2}, "
                    f"{'columns' if i & 1 else 'rows'}): expected {want_res[i]} G; problems {bad.tolist()} differ")


def contents(c, nsets, kind, seed=0):
    """bucket multiples m[nsets][L] (bucket l = weight l + 1 at index l); different per set"""
    L, H, D = split(c)
    rng = np.random.default_rng(1000 * c + 10 * nsets + seed)
    m = np.zeros((nsets, L), dtype=np.int64)
    s1 = np.arange(1, nsets + 1, dtype=np.int64)[:, None]
    j = np.arange(1, L + 1, dtype=np.int64)[None, :]        # weights
    if kind == "empty":
        pass
    elif kind == "weight_L":
        m[:, L - 1] = 3 * s1[:, 0]
    elif kind == "bucket_1":
        m[:, 0] = 5 * s1[:, 0]
    elif kind == "last_before_L":
        m[:, max(L - 2, 0)] = 7 * s1[:, 0]
    elif kind == "full_row":            # row H - 1 (its buckets h D + d, all d)
        m[:] = np.where((j // D == H - 1) & (j < L), s1 + j % 5 + 1, 0)
    elif kind == "full_column":         # column D - 1 (column 0 has no bucket of weight 0)
        m[:] = np.where((j % D == D - 1) & (j < L), s1 + j % 3 + 1, 0)
    elif kind == "same":                # every bucket the same point: all R_h equal (but row 0 and H/2), all C_d equal
        m[:] = 2 * s1 + 1
    elif kind == "alternating":         # P, -P, ...: line sums cancel inside the chunks, the pair sums and the quads
        m[:] = np.where(j % 2 == 0, s1 + 3, -(s1 + 3))
        m[:, L - 1] = 0
    elif kind == "alternating_lines":   # R_h = +-P D: neighbouring LINES cancel inside the quads
        m[:] = np.where((j // D) % 2 == 0, s1, -s1)
        m[:, L - 1] = 0
    elif kind == "tri_doubles":         # R_1 + R_3 = 2 (R_2 + R_3) in every quad of lines: the generic tri lane meets P = Q
        line_val = np.array([9, 4, 1, 2], dtype=np.int64)[(j // D) % 4]
        m[:] = np.where((j % D == D - 1) & (j < L), line_val * s1, 0)
    elif kind == "neutral_quads":       # quads of neutral lines next to live ones
        m[:] = np.where(((j // D) // 4) % 2 == 1, s1 + j % 7, 0)
        m[:, L - 1] = 0
    elif kind == "random":              # distinct multiples (L > 256: 31 distinct values, so that every line sum stays
        for s in range(nsets):          # inside the pool), random signs, a tenth of the buckets empty
            mag = rng.permutation(np.arange(1, L + 1))
            m[s] = (mag if L <= 256 else mag % 31 + 1) * rng.choice([-1, 1], size=L) + (0 if L > 8 else 10 * s)
            m[s][rng.random(L) < 0.1] = 0
            m[s][L - 1] = min(L, 200) + 3 + s
    else:
        raise ValueError(kind)
    return m


CONTENT_KINDS = ["empty", "weight_L", "bucket_1", "last_before_L", "full_row", "full_column", "same", "alternating",
                 "alternating_lines", "tri_doubles", "neutral_quads", "random"]


@pytest.mark.parametrize("label,mode", CURVE_MODES, ids=CM_IDS)
def test_geometry(ctxs, label, mode):
    """every window size, NC in {1, 2, largest, default}, 1 / 2 / 5 bucket sets with different contents per set (a
    problem that reads its neighbour's lines fails), distinct random multiples, the engine's own level selection"""
    for c in CS_OF[label]:
        for nsets in (1, 2, 5):
            for nc in ncs(c, nsets):
                if c == 16 and nsets == 5 and nc not in (0, split(c)[2]):
                    continue      # (the largest shape: default and largest NC only)
                run_2d(ctxs, label, mode, c, nsets, contents(c, nsets, "random", nc), nc=nc, what="random", lam=nc)


@pytest.mark.parametrize("label,mode", CURVE_MODES, ids=CM_IDS)
def test_level_kernels_forced(ctxs, label, mode):
    """k_reduce_quad vs k_reduce_quad16, k_pairsum vs k_pairsum_x4 and tail thresholds 1 / 4 / 32 / beyond H, every
    combination at every shape"""
    for c in CS_OF[label]:
        D = split(c)[2]
        nsets = 1 if c == 16 else 2
        m = contents(c, nsets, "random", 77)
        for kern in KERNELS:
            run_2d(ctxs, label, mode, c, nsets, m, nc=min(4, D), kern=kern, what="random", variant=kern[0])


@pytest.mark.parametrize("kind", CONTENT_KINDS)
@pytest.mark.parametrize("label,mode", CURVE_MODES, ids=CM_IDS)
def test_contents(ctxs, label, mode, kind):
    """degenerate bucket contents under the default level selection and with each level kernel forced; H = 2, 4, 8, 16,
    32 (levels with and without a short last group); in the accumulator modes with one and with many chunk accumulators per
    bucket, all in one representation and each in its own"""
    for c in CS_CONTENTS[label]:
        D = split(c)[2]
        for nsets in (1, 3):
            m = contents(c, nsets, kind)
            for kern in FEW:
                for nc in sorted({1, D}):
                    if mode == LOCS:
                        run_2d(ctxs, label, mode, c, nsets, m, nc=nc, kern=kern, what=kind, variant=nc)
                    else:
                        run_2d(ctxs, label, mode, c, nsets, m, nc=nc, kern=kern, what=kind, cnt_style="one", lam=0)
                        run_2d(ctxs, label, mode, c, nsets, m, nc=nc, kern=kern, what=kind, cnt_style="one", lam=5)
                        run_2d(ctxs, label, mode, c, nsets, m, nc=nc, kern=kern, what=kind, cnt_style="mixed", lam=9)


@pytest.mark.parametrize("label", WEIER)
def test_location_encodings(ctxs, label):
    """1 .. 4 locations per bucket, LOC_NONE in each position, point / negated point / slot / infinity in each position,
    the same point twice, the weight-L bucket with several locations: every pattern of encode_locations at every bucket
    position (the pattern of a bucket rotates with `variant`)"""
    for c in (2, 4, 7, 9):
        L = split(c)[0]
        for variant in range(11):
            m = contents(c, 2, "random", variant)
            m[:, L - 1] = 20 + 2 * variant      # even: the weight-L bucket takes the two-location patterns too
            run_2d(ctxs, label, LOCS, c, 2, m, nc=0, what=f"location patterns, variant {variant}", variant=variant)
            run_2d(ctxs, label, LOCS, c, 2, contents(c, 2, "same"), nc=1, kern=(1, 1, 1), what=f"same, variant {variant}",
                   variant=variant)


@pytest.mark.parametrize("summed", [ACCS, SUMMED], ids=["ranges", "bucket_sums"])
@pytest.mark.parametrize("label", ALL)
def test_chunk_ranges(ctxs, label, summed):
    """cscan ranges of 0, 1, 2, 3 and 40 chunk accumulators; an empty range as the first bucket, the last before L and
    the last of every chunk of a line (period 7 against power-of-two chunks); the weight-L bucket empty and with 40"""
    for c in (2, 3, 5, 8, 10):
        D = split(c)[2]
        for style in ("mixed", "edges_empty", "edges_long"):
            for nc in sorted({1, min(2, D), D}):
                for lam in (0, 3):
                    run_2d(ctxs, label, summed, c, 3, contents(c, 3, "random", 5), nc=nc, what="random",
                           cnt_style=style, lam=lam)
                    run_2d(ctxs, label, summed, c, 3, contents(c, 3, "same", 5), nc=nc, kern=(4, 1, 1), what="same",
                           cnt_style=style, lam=lam)


# --------------------------------------------------------------------------------------------------- levels only
N_INS = [1, 2, 3, 4, 5, 7, 16, 17, 31, 32, 33, 63, 64, 100, 1000]


def run_levels(ctxs, label, rows, cs, kern=DEFAULT, what="", lam=0):
    """rows, cs: multiples [nprob][n_in]; result j = sum_e (C_e + e row_e)"""
    pl = pool(label)
    rows, cs = np.asarray(rows, dtype=np.int64), np.asarray(cs, dtype=np.int64)
    nprob, n_in = rows.shape
    vals = np.concatenate([rows.reshape(-1), cs.reshape(-1)])
    kw = dict(points_xy=pl.take(vals), n_points=len(vals))
    if lam:
        kw["scale"] = scales(pl, len(vals), lam)
    tail, quad, pair = kern
    st, out, _ = call(ctxs(label), fb=pl.fb, mode=LEVELS, nsets=nprob, n_in=n_in, tail_n=tail, quad16_max=quad,
                      n_res=nprob, **kw)
    tag = f"{label} levels n_in={n_in} nprob={nprob} tail_n={tail} quad16_max={quad} [{what}; lambda={lam}]"
    assert st == 0, f"{tag}: status {st}"
    e = np.arange(n_in, dtype=object)
    want = [int((cs[j].astype(object) + e * rows[j].astype(object)).sum()) % pl.q for j in range(nprob)]
    bad = np.nonzero((pl.enc_many(want) != out).any(axis=1))[0]
    if len(bad):
        j = int(bad[0])
        pytest.fail(f"{tag}: problem {j}: expected {want[j]} G; problems {bad.tolist()} differ")


LEVEL_KERNELS = [(t, q, 0) for t in (1, 4, 32, 4096) for q in (1, 1 << 20)]


@pytest.mark.parametrize("nprob", [1, 3, 33])
@pytest.mark.parametrize("label", ALL)
def test_levels_shapes(ctxs, label, nprob):
    """BucketReduce::levels on n_in entries that are not a power of four, with non-neutral C inputs (the form reduce_affine.h
    feeds it), every level kernel forced"""
    for n_in in N_INS:
        rng = np.random.default_rng(n_in * 64 + nprob)
        rows = rng.integers(-1000, 1001, size=(nprob, n_in))
        cs = rng.integers(-1000, 1001, size=(nprob, n_in))
        rows[:, n_in // 2] = 0
        for kern in (LEVEL_KERNELS if n_in <= 100 else LEVEL_KERNELS[::3]):
            run_levels(ctxs, label, rows, cs, kern=kern, what="random", lam=n_in if kern[0] == 4 else 0)


def degenerate_levels(n_in, nprob, kind):
    e = np.arange(n_in, dtype=np.int64)[None, :]
    j1 = np.arange(1, nprob + 1, dtype=np.int64)[:, None]
    rows = np.zeros((nprob, n_in), dtype=np.int64)
    cs = np.zeros((nprob, n_in), dtype=np.int64)
    q0 = e - e % 4
    if kind == "all_equal":             # r0 + r1, r1 + r3, r2 + r3 and c2 + c3, c0 + c1: P = Q on every generic lane
        rows[:] = j1 + 2
        cs[:] = j1 + 1
    elif kind == "alternating":         # r0 + r1 = 0, r2 + r3 = 0, r1 + r3 = 2 r1
        rows[:] = np.where(e % 2 == 0, j1, -j1)
        cs[:] = np.where(e % 2 == 0, -j1 - 1, j1 + 1)
    elif kind == "r1_is_minus_r3":      # b = r1 + r3 = 0
        rows[:] = np.select([e % 4 == 1, e % 4 == 3], [j1 + 4, -(j1 + 4)], j1)
    elif kind == "tri_doubles":         # r1 + r3 = 2 (r2 + r3): tri = b + 2a with b = 2a
        rows[:] = np.array([9, 4, 1, 2], dtype=np.int64)[e % 4] * j1
        cs[:] = e % 3
    elif kind == "cs_is_minus_tri":     # c0 = -(r1 + 2 r2 + 3 r3) of its quad -- the last, short quad included
        rows[:] = (e * 5 + j1) % 11 + 1
        pad = np.zeros((nprob, (-n_in) % 4), dtype=np.int64)
        r4 = np.concatenate([rows, pad], axis=1).reshape(nprob, -1, 4)
        tri = r4[:, :, 1] + 2 * r4[:, :, 2] + 3 * r4[:, :, 3]
        cs[:, 0::4] = -tri
    elif kind == "cs_is_tri":           # C' = cs + tri with cs = tri
        rows[:] = (e * 5 + j1) % 11 + 1
        pad = np.zeros((nprob, (-n_in) % 4), dtype=np.int64)
        r4 = np.concatenate([rows, pad], axis=1).reshape(nprob, -1, 4)
        cs[:, 0::4] = r4[:, :, 1] + 2 * r4[:, :, 2] + 3 * r4[:, :, 3]
    elif kind == "neutral_quads":       # an all-neutral quad (rows and C) next to a live one
        live = (q0 // 4) % 2 == 1
        rows[:] = np.where(live, j1 + e % 5, 0)
        cs[:] = np.where(live, j1, 0)
    elif kind == "all_neutral":
        pass
    return rows, cs


@pytest.mark.parametrize("kind", ["all_equal", "alternating", "r1_is_minus_r3", "tri_doubles", "cs_is_minus_tri",
                                  "cs_is_tri", "neutral_quads", "all_neutral"])
@pytest.mark.parametrize("label", ALL)
def test_levels_degenerate(ctxs, label, kind):
    """equal, opposite and neutral operands on every lane of a quad, in the first quad of a problem and in the last,
    short one; in one representation (lambda = 1) and with every record in its own"""
    for n_in in N_DEGENERATE[label]:
        for nprob in (1, 3):
            rows, cs = degenerate_levels(n_in, nprob, kind)
            for kern in LEVEL_KERNELS:
                for lam in (0, 11):
                    run_levels(ctxs, label, rows, cs, kern=kern, what=kind, lam=lam)


# --------------------------------------------------------------------------------------------------- arguments
def test_hook_rejects_bad_arguments(ctxs):
    """nothing the caller passes can make a kernel read or write outside its buffers; the hook's level selection does
    not outlive the call: an MSM on the same context still matches the oracle"""
    from oracle import c_oracle
    label = "bls12-377"
    pl, curve = pool(label), ctxs(label)
    c, nsets = 5, 2
    L, H, D = split(c)
    m = contents(c, nsets, "random").reshape(-1)
    base = dict(fb=pl.fb, c=c, nsets=nsets, n_res=2 * nsets, n_lines=2 * nsets * H)
    lk = dict(base, mode=LOCS, **encode_locations(pl, m))
    ak = dict(base, mode=ACCS, **encode_accs(pl, m, np.ones(nsets * L, dtype=np.int64), 3))
    st = lambda kw, **over: call(curve, **{**kw, **over})[0]
    assert st(lk) == 0 and st(ak) == 0 and st(ak, mode=SUMMED) == 0
    for bad in (dict(c=1), dict(c=17), dict(nsets=0), dict(nsets=17), dict(mode=4), dict(mode=-1), dict(nc=3),
                dict(nc=2 * D), dict(tail_n=4097), dict(quad16_max=(1 << 20) + 1), dict(pairsum_x4_max=(1 << 20) + 1)):
        assert st(lk, **bad) == MSMZ_ERR_ARG, bad
        assert st(ak, **bad) == MSMZ_ERR_ARG, bad
    for word in (LOC_ORIG | lk["n_points"], LOC_ORIG | LOC_NEG | lk["n_points"], lk["n_slots"], LOC_NEG | 1):
        for pos in (0, 3):
            loc = lk["loc"].copy()
            loc[nsets * L - 1, :pos] = LOC_ORIG        # (point 0 in the positions before it)
            loc[nsets * L - 1, pos] = word
            assert st(lk, loc=loc) == MSMZ_ERR_ARG, (hex(word), pos)
    assert st(lk, scale=scales(pl, lk["n_points"], 1)) == MSMZ_ERR_ARG
    cscan = ak["cscan"].copy()
    cscan[-1] += 1                                     # one record beyond the list
    assert st(ak, cscan=cscan) == MSMZ_ERR_ARG
    cscan = ak["cscan"].copy()
    cscan[7] = cscan[8] + 1                            # decreasing
    assert st(ak, cscan=cscan) == MSMZ_ERR_ARG
    big = ak["points_xy"].copy()
    big[3, pl.fb - 1] = 0xFF                           # x >= p
    assert st(ak, points_xy=big) == MSMZ_ERR_RANGE
    lam = ak["scale"].copy()
    lam[5, pl.fb - 1] = 0xFF
    assert st(ak, scale=lam) == MSMZ_ERR_RANGE
    lam = ak["scale"].copy()
    lam[5] = 0
    assert st(ak, scale=lam) == MSMZ_ERR_ARG
    big = lk["slots_xy"].copy()
    big[1, 2 * pl.fb - 1] = 0xFF
    assert st(lk, slots_xy=big) == MSMZ_ERR_RANGE
    lv = dict(fb=pl.fb, mode=LEVELS, nsets=2, n_in=5, points_xy=pl.take(np.arange(20)), n_points=20, n_res=2)
    assert st(lv) == 0
    for bad in (dict(n_in=0), dict(n_in=4097), dict(nsets=65), dict(n_points=19), dict(nc=2), dict(tail_n=5000)):
        assert st(lv, **bad) == MSMZ_ERR_ARG, bad
    assert st(dict(lk, fb=pl.fb), mode=LOCS) == 0
    te = ctxs("ed-on-bls12-377")
    assert call(te, **dict(lk, fb=32))[0] == MSMZ_ERR_UNSUPPORTED
    # forced kernels, then ordinary MSMs: planned and reduced as before
    run_2d(ctxs, label, ACCS, 6, 2, contents(6, 2, "random"), nc=4, kern=(1, 1, 1), what="before the MSM")
    n = 1 << 12
    pts = curve.Parallel.randomPointsFast(n, 11)
    sc = curve.Parallel.randomScalars(n, 12)
    want = c_oracle.msm(P.CURVES[label], curve.Scalar.toBigints(sc), curve.Affine.toBigints(pts))
    assert curve.Parallel.msm(sc, pts, n, False, {"glv": 0})["result"] == want
    assert curve.Parallel.msm(sc, pts, n, False, {"glv": 1, "c": 9})["result"] == want
    assert curve.Parallel.msm(sc, pts, n, False, {"glv": 0, "reduceAffine": 1})["result"] == want
    assert curve.Parallel.msmProjective(sc, pts, n)["result"] == want
    pts.free(); sc.free()

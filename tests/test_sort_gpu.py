"""The bucket sort stage by stage, at every geometry an MSM runs it in: msmz_test_sort_ex (include/msmz_test.h) drives
the engine's own make_plan / sort_layout / sort stage (BucketSort::run, csrc/sort.h) on caller-built scalars, and every
word it returns is compared with the host model oracle/sort_ref.py (pinned without a GPU by tests/test_sort_ref_cpu.py).

The comparison is exact and complete: for every problem and every bucket the multiset of reference words, the bucket
offsets, the scanned bin bases, the packed words of every bin, the entry count, the largest bucket and the error word.  A
failure names the first stage that disagrees (histogram / scan, k_coarse, k_fine or the fallback) and the bin or bucket.

Every case names the regimes it is there for, and the test asserts from the reported geometry (and the model's bin
sizes) that they were reached: a planner change that moves a case out of its regime fails here.

Checked against three one-value mutations of BucketSort::run's launches (never an address or a count): k_fine without
endo_delta (named by glv-prefix, pre-F2-glv-prefix at "k_fine"), k_fine without copy_stride (all five pre-* cases at
"k_fine"), k_scatter without endo_delta (fallback-glv-prefix at "fallback sort"); bin bases and packed words still agreed,
so each was attributed to the right stage."""
import ctypes as C
import itertools
import zlib

import numpy as np
import pytest

from oracle import params as P
from oracle import sort_ref as S

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = 1, 4                             # include/msmz.h
FINE_STAGE, COARSE_T, SORT_MAX_BINS = 37888, 1024, 8192     # csrc/plan.h

# what a case can be there for: tag -> predicate on (geometry, case, model)
REGIMES = {
    "bins>threads": lambda g, case, m: g["nbins"] > COARSE_T,
    "unstaged": lambda g, case, m: m["largest_bin"] > FINE_STAGE,
    "fbt<fb": lambda g, case, m: g["fbt"] < g["fb"],
    "spread": lambda g, case, m: g["spread"] > 0,
    "fold": lambda g, case, m: g["fold_shift"] != 0,
    "F>1": lambda g, case, m: g["F"] > 1,
    "batch": lambda g, case, m: case["nprob"] > 1 and g["two_level"] == 1,
    "scan3": lambda g, case, m: case["nprob"] * g["sbins"] > SORT_MAX_BINS,
    "cspec<max": lambda g, case, m: g["cspec"] != 0 and g["K"] < ((4 if case["glv"] else 8) * 32 + g["c"]) // g["c"],
    "generic": lambda g, case, m: g["cspec"] == 0 and g["two_level"] == 1,
    "fallback": lambda g, case, m: g["two_level"] == 0,
    "prefix": lambda g, case, m: g["endo_delta"] != 0,
    "bound": lambda g, case, m: g["sbits"] < 256 and m["error"] & 4,
    "flag>=q": lambda g, case, m: m["error"] & 4,
    "overflow": lambda g, case, m: m["error"] & 2,
    "singletons": lambda g, case, m: m["largest"] == 1,
    "tiles>1": lambda g, case, m: g["tiles"] > 1,
    "clean": lambda g, case, m: m["error"] == 0,
}


def case(name, label, n, c, regimes, glv=0, nprob=1, fallback=0, sbits=0, fold=0, pts_n=0, factor=0, stride=0, mix="random",
         glv_bits=0, big=False):
    return dict(name=name, label=label, n=n, c=c, regimes=regimes, glv=glv, nprob=nprob, fallback=fallback, sbits=sbits,
                fold=fold, pts_n=pts_n, factor=factor, stride=stride, mix=mix, glv_bits=glv_bits, big=big)


CASES = []
# ---- tile edges: one scalar, one short of a tile, a full tile, one into the next, three tiles and a few
for n in (1, 2, 2047, 2048, 2049, 3 * 2048 + 5):
    CASES.append(case(f"tile-{n}", "bls12-377", n, 17, ["cspec<max", "clean"] + (["singletons"] if n == 1 else [])
                      + (["tiles>1"] if n > 2048 else [])))
for n in (1023, 1024, 1025, 5 * 1024 + 3):
    CASES.append(case(f"tile-glv-{n}", "bls12-377", n, 16, ["cspec<max", "clean"] + (["tiles>1"] if n > 1024 else []), glv=1))
CASES += [
    case("tile-pallas-2049", "pallas", 2049, 16, ["cspec<max", "tiles>1"]),
    case("tile-pallas-glv-1025", "pallas", 1025, 11, ["generic", "tiles>1"], glv=1),
    case("tile-381-2047", "bls12-381", 2047, 12, ["generic"]),
    case("tile-381-glv-5123", "bls12-381", 5 * 1024 + 3, 16, ["cspec<max", "tiles>1"], glv=1),
    case("tile-ed-6149", "ed-on-bls12-377", 3 * 2048 + 5, 13, ["generic", "tiles>1"]),
    case("tile-ed-2048", "ed-on-bls12-377", 2048, 17, ["cspec<max"]),
    # ---- more coarse bins than threads: k_coarse parks the tile rows in LDS (per > 1)
    case("bins-c13-2^21", "bls12-377", 1 << 21, 13, ["bins>threads", "tiles>1"], big=True),
    case("bins-c19-2^15", "bls12-377", 1 << 15, 19, ["bins>threads", "tiles>1"]),
    case("bins-c20-glv-5123", "pallas", 5 * 1024 + 3, 20, ["bins>threads", "tiles>1"], glv=1),
    # ---- a bin beyond k_fine's staging: heavy repeats
    case("unstaged-mixed", "bls12-377", 1 << 17, 14, ["unstaged"], mix="repeat", big=True),
    case("unstaged-mixed-glv", "bls12-377", 1 << 17, 14, ["unstaged"], mix="repeat", glv=1, big=True),
    case("unstaged-equal", "bls12-377", 1 << 16, 14, ["unstaged"], mix="equal"),
    case("unstaged-equal-glv", "pallas", 1 << 16, 14, ["unstaged"], mix="equal", glv=1),
]
# ---- thin top window: spread over sub-windows, or folded into its own set
for c, glv in ((14, 0), (18, 0), (11, 0), (9, 1)):
    CASES.append(case(f"thin-c{c}-spread", "bls12-377", 4099, c, ["spread"], glv=glv))
    CASES.append(case(f"thin-c{c}-fold", "bls12-377", 4099, c, ["fold"], glv=glv, fold=1))
CASES += [
    # c = 16: 13 significant top bits, too wide to fold (the column index has 7): spread whether a fold is allowed or not
    case("thin-c16-spread", "bls12-377", 4099, 16, ["spread", "cspec<max"]),
    case("thin-c16-fold-allowed", "bls12-377", 4099, 16, ["spread", "cspec<max"], fold=1),
    case("thin-pallas-c17-fold", "pallas", 2049, 17, ["fold"], fold=1),
    case("dense-top-fbt", "bls12-377", 1 << 16, 12, ["fbt<fb"]),
    # ---- batches: one scan over all problems, vectors of different skew
    case("batch-2", "bls12-377", 5003, 11, ["batch"], nprob=2, mix="skew"),
    case("batch-3-glv", "bls12-377", 3001, 9, ["batch", "fold"], nprob=3, mix="skew", glv=1, fold=1),
    case("batch-17", "pallas", 2049, 12, ["batch", "tiles>1"], nprob=17, mix="skew"),
    case("batch-18-scan3", "bls12-377", 2049, 17, ["batch", "scan3", "cspec<max"], nprob=18, mix="skew"),
    # ---- precomputed sets: F windows per bucket set, copies copy_stride apart
    case("pre-F2", "bls12-377", 6149, 0, ["F>1"], factor=2, stride=7001),
    case("pre-F3", "bls12-377", 6149, 0, ["F>1"], factor=3, stride=6150),
    case("pre-FK", "bls12-377", 6149, 0, ["F>1"], factor=128, stride=9973),
    case("pre-F2-glv-prefix", "bls12-377", 5123, 0, ["F>1", "prefix"], factor=2, stride=20011, glv=1, pts_n=7000),
    case("pre-F3-batch3", "pallas", 4099, 0, ["F>1", "batch"], factor=3, stride=5000, nprob=3, mix="skew"),
    case("pre-FK-2^16-c17", "bls12-377", 1 << 16, 0, ["F>1", "cspec<max"], factor=128, stride=70001),
    case("glv-prefix", "bls12-381", 3001, 10, ["prefix", "generic"], glv=1, pts_n=4500),
    # ---- GLV halves above the assumed length: flagged; under a fold the overflowing top digit is in no bucket
    case("glv-overflow-spread", "bls12-377", 3001, 9, ["overflow"], glv=1, glv_bits=100),
    case("glv-overflow-fold", "bls12-377", 3001, 9, ["overflow", "fold"], glv=1, glv_bits=100, fold=1),
    case("glv-overflow-fallback", "pallas", 1500, 9, ["overflow", "fallback"], glv=1, glv_bits=100, fallback=1),
    # ---- the one-pass atomic fallback
    case("fallback-plain", "bls12-377", 3001, 10, ["fallback"], fallback=1),
    case("fallback-1", "bls12-377", 1, 10, ["fallback", "singletons"], fallback=1),
    case("fallback-spread", "bls12-377", 4099, 14, ["fallback", "spread"], fallback=1),
    case("fallback-glv-prefix", "pallas", 2049, 11, ["fallback", "prefix"], fallback=1, glv=1, pts_n=3000),
    case("fallback-bound", "bls12-377", 3001, 16, ["fallback", "bound"], fallback=1, sbits=128, mix="bound"),
    case("fallback-ed", "ed-on-bls12-377", 2049, 12, ["fallback"], fallback=1),
    case("fallback-c22", "bls12-377", 3001, 22, ["fallback"]),
    # ---- scalars >= the group order: flagged, no entry
    case("flag-q", "bls12-381", 2 * 2048 + 1, 13, ["flag>=q"], mix="geq"),
    case("flag-q-glv", "bls12-377", 2 * 1024 + 1, 16, ["flag>=q"], mix="geq", glv=1),
    case("fallback-flag-q", "bls12-377", 1500, 10, ["fallback", "flag>=q"], fallback=1, mix="geq"),
    case("fallback-flag-q-glv", "bls12-377", 1500, 10, ["fallback", "flag>=q"], fallback=1, mix="geq", glv=1),
]
# ---- caller-given bounds: 2^bits - 1 sorts, 2^bits is flagged and leaves no entry
for bits in (64, 128):
    for c in (7, 16, 17):
        CASES.append(case(f"bound-{bits}-c{c}", "bls12-377", 2 * 2048 + 1, c,
                          ["bound"] + (["cspec<max"] if c >= 16 else ["generic"]), sbits=bits, mix="bound"))
# (129 bits in windows of 16: the ninth holds the carry alone and folds)
CASES.append(case("bound-128-c16-fold", "bls12-377", 4099, 16, ["bound", "fold", "cspec<max"], sbits=128, mix="bound", fold=1))


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


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def sort_ex(curve, scalars, cs, outputs=True, **override):
    """one call of the hook: (status, geometry dict, meta, off, refs, bins, packed); with outputs=False the plan only"""
    N = _native()
    a = N.MsmzTestSortArgs()
    words = np.ascontiguousarray(scalars, dtype=np.uint32)
    a.scalars_le32 = ptr(words)
    a.n, a.pts_n, a.nprob = cs["n"], cs["pts_n"], cs["nprob"]
    a.factor, a.copy_stride, a.c, a.glv = cs["factor"], cs["stride"], cs["c"], cs["glv"]
    a.force_fallback, a.scalar_bits, a.allow_fold = cs["fallback"], cs["sbits"], cs["fold"]
    geom = np.zeros(len(N.TEST_SORT_GEOM), dtype=np.uint32)
    a.geom, a.geom_cap = ptr(geom), len(geom)
    for k, v in override.items():
        setattr(a, k, v)
    st = N.lib().msmz_test_sort_ex(curve._ctx, C.byref(a))
    g = dict(zip(N.TEST_SORT_GEOM, (int(x) for x in geom)))
    if st != 0 or not outputs:
        return st, g, None, None, None, None, None
    M = cs["n"] * (2 if cs["glv"] else 1)
    cap = cs["nprob"] * g["K"] * M
    meta = np.full(3, 0xa5a5a5a5, dtype=np.uint32)
    off = np.full(cs["nprob"] * g["nb"] + 1, 0xa5a5a5a5, dtype=np.uint32)
    refs = np.full(cap, 0xa5a5a5a5, dtype=np.uint32)
    bins = np.full(cs["nprob"] * g["sbins"] + 1, 0xa5a5a5a5, dtype=np.uint32) if g["two_level"] else None
    packed = np.full(cap, 0xa5a5a5a5, dtype=np.uint32) if g["two_level"] else None
    a.meta, a.off, a.off_cap, a.refs, a.refs_cap = ptr(meta), ptr(off), len(off), ptr(refs), len(refs)
    if g["two_level"]:
        a.bins, a.bins_cap, a.packed, a.packed_cap = ptr(bins), len(bins), ptr(packed), len(packed)
    for k, v in override.items():
        setattr(a, k, v)
    st = N.lib().msmz_test_sort_ex(curve._ctx, C.byref(a))   # (a refused call returns its outputs too: untouched)
    return st, g, meta, off, refs, bins, packed


def set_rows(words, rows, values):
    for r, v in zip(rows, values):
        words[r] = S.to_words([v], 8)[0]


def build_scalars(cs, g, q, rng):
    """nprob x n scalars as (nprob, n, 8) words: random below the order (or the bound), the case's mix, and the digit
    corners -- 0, 1, q - 1, all-ones windows, a digit exactly L (no carry) and L + 1 (carry) in the first, a middle and the
    top window -- at the first, a middle and the last position of a tile"""
    n, Pn, c, K = cs["n"], cs["nprob"], g["c"], g["K"]
    bits = min(q.bit_length() - 1, cs["sbits"] or 256)
    words = rng.integers(0, 1 << 32, size=(Pn, n, 8), dtype=np.uint64).astype(np.uint32)
    words[:, :, bits // 32 + 1:] = 0
    if bits % 32:
        words[:, :, bits // 32] &= np.uint32((1 << (bits % 32)) - 1)
    elif bits // 32 < 8:
        words[:, :, bits // 32] = 0
    top = min(q - 1, (1 << bits) - 1)
    L = 1 << (c - 1)
    for p in range(Pn):
        w = words[p]
        if cs["mix"] == "equal":
            w[:] = w[0]
        elif cs["mix"] == "repeat":        # 2^16 copies of one scalar between random ones
            w[0:1 << 17:2] = w[1]
        elif cs["mix"] == "skew":          # problem p: every (p + 2)-th scalar one of p + 1 values
            few = w[:p + 1].copy()
            idx = np.arange(0, n, p + 2)
            w[idx] = few[idx % (p + 1)]
        corners = [0, 1, top, top - 1, (1 << min(200, bits - 1)) - 1, (1 << (bits - 1)) - 1]
        for k in (0, K // 2, K - 1):
            corners += [v for v in ((L << (c * k)), ((L + 1) << (c * k))) if v <= top]
        flags = []                          # values that must be flagged and leave no entry
        if cs["mix"] == "bound":
            corners.append((1 << cs["sbits"]) - 1)
            flags = [1 << cs["sbits"], (1 << cs["sbits"]) + 12345, q - 1, 1 << 255]
        if cs["mix"] == "geq":
            flags = [q, q + 1, (1 << 256) - 1]
        if cs["mix"] == "equal":
            corners = []
        corners = corners[:max(0, n - 1 - len(flags))]      # (tiny inputs keep a random scalar)
        tile = 1024 if cs["glv"] else 2048
        # the flagged ones first, in the middle and last in a tile, and last of all
        place = {}
        if flags and n > 5:
            for r, v in zip((0, tile // 2, tile - 1, tile, n - 1), itertools.cycle(flags)):
                place[r % n] = v
        spots = itertools.chain((0, tile - 1, tile, n // 2, n - 1, 1, tile + 1, n - 2), itertools.count(211 + p, 211))
        for v in corners:
            r = next(spots) % n
            while r in place:
                r = (r + 1) % n
            place[r] = v
        rows, corners = list(place), list(place.values())
        set_rows(w, rows, corners)
    return words


def halves_of(curve, cs, words_p):
    """the (half-)scalars of one problem: the scalar itself, or the device's GLV halves (any valid split is acceptable;
    tests/test_glv_edges_gpu.py checks the split, and this sort, against the integer model of the split)"""
    n = cs["n"]
    if not cs["glv"]:
        return [(words_p, np.zeros(n, dtype=np.uint8))]
    s0, s1, neg = np.zeros((n, 4), dtype=np.uint32), np.zeros((n, 4), dtype=np.uint32), np.zeros((n, 2), dtype=np.uint8)
    assert _native().lib().msmz_test_glv(curve._ctx, np.ascontiguousarray(words_p).ctypes.data_as(C.c_char_p), n,
                                         s0.ctypes.data_as(C.c_char_p), s1.ctypes.data_as(C.c_char_p),
                                         neg.ctypes.data_as(C.c_char_p)) == 0
    return [(s0, neg[:, 0]), (s1, neg[:, 1])]


def check_sort(curve, cs, words, tag):
    """run the hook on `words` and compare every output with the model; returns (geometry, model)"""
    q = P.CURVES[cs["label"]]["order"]
    st, g, meta, off, refs, bins, packed = sort_ex(curve, words, cs)
    assert st == 0, f"{tag}: status {st}"
    probs = []
    for p in range(cs["nprob"]):
        bad = S.flagged(words[p], q, cs["sbits"])
        probs.append(S.problem_entries(halves_of(curve, cs, words[p]), bad, g, cs["n"], cs["stride"], detail=False))
    m = S.sort_model(probs, g)
    del probs
    err, n_entries, max_bucket = (int(x) for x in meta)
    nbk = cs["nprob"] * g["nb"]
    print(f"{tag}: geometry {g} entries {n_entries} largest {m['largest']} error {err}")
    assert err == m["error"], f"{tag}: error word {err}, model {m['error']}"
    assert n_entries == m["n_entries"], f"{tag}: n_entries {n_entries}, model {m['n_entries']}"
    if g["two_level"]:
        # stage 1: histogram + scan
        F, sb = g["F"], g["sbins"]
        binsz = np.diff(m["bins"])
        m["largest_bin"] = int(binsz.reshape(-1, F).sum(axis=1).max())
        b64 = bins.astype(np.int64)
        bad = np.nonzero(b64 != m["bins"])[0]
        assert bad.size == 0, (f"{tag}: k_hist / scan: bin base {int(bad[0])} (problem {int(bad[0]) // sb}, bin {int(bad[0]) % sb}) "
                               f"is {int(b64[bad[0]])}, model {int(m['bins'][bad[0]])}")
        # stage 2: the coarse scatter, bin by bin as multisets
        d = S.first_difference(S.keyed_ranges(b64, packed), m["by_bin"])
        assert d is None, (f"{tag}: k_coarse: bin {d[0]} (problem {d[0] // sb}, bin {d[0] % sb}): first word that differs "
                           f"got {d[1]}, model {d[2]}")
        assert (packed[n_entries:] == 0xa5a5a5a5).all(), f"{tag}: packed words written beyond n_entries"
    else:
        m["largest_bin"] = 0
    # stage 3: offsets and references (k_fine, or the fallback's scan and scatter)
    stage = "k_fine" if g["two_level"] else "fallback sort"
    o64 = off.astype(np.int64)
    assert o64[0] == 0 and o64[nbk] == n_entries, f"{tag}: {stage}: off[0] {o64[0]}, off[last] {o64[nbk]}, entries {n_entries}"
    dec = np.nonzero(np.diff(o64) < 0)[0]
    assert dec.size == 0, f"{tag}: {stage}: off decreases after bucket {int(dec[0]) if dec.size else None}"
    for p in range(cs["nprob"] + 1):
        assert o64[p * g["nb"]] == m["off"][p * g["nb"]], (f"{tag}: {stage}: seam of problem {p}: off {o64[p * g['nb']]}, "
                                                          f"model {m['off'][p * g['nb']]}")
    bad = np.nonzero(o64 != m["off"])[0]
    assert bad.size == 0, (f"{tag}: {stage}: off[{int(bad[0])}] (problem {int(bad[0]) // g['nb']}, bucket {int(bad[0]) % g['nb']}) "
                           f"is {int(o64[bad[0]])}, model {int(m['off'][bad[0]])}")
    d = S.first_difference(S.keyed_ranges(o64, refs), m["by_bucket"])
    assert d is None, (f"{tag}: {stage}: bucket {d[0]} (problem {d[0] // g['nb']}, bucket {d[0] % g['nb']}): first reference "
                       f"that differs got {d[1]}, model {d[2]}")
    assert (refs[n_entries:] == 0xa5a5a5a5).all(), f"{tag}: references written beyond n_entries"
    want_max = S.expected_max_bucket(m["largest"], g["two_level"])
    assert max_bucket == want_max, f"{tag}: max_bucket {max_bucket}, rule gives {want_max} (largest bucket {m['largest']})"
    return g, m


@pytest.mark.parametrize("cs", CASES, ids=[c["name"] for c in CASES])
def test_sort_against_model(ctxs, cs):
    """every word the sort leaves, for the case's geometry; then: the case reached the regimes it is named for"""
    cv = P.CURVES[cs["label"]]
    if cs["glv"]:
        assert "endomorphism" in cv, "GLV cases belong to curves with an endomorphism"
    curve = ctxs(cs["label"])
    lib = _native().lib()
    rng = np.random.default_rng(zlib.crc32(cs["name"].encode()))
    try:
        if cs["glv_bits"]:
            assert lib.msmz_test_set_glv_bits(curve._ctx, cs["glv_bits"]) == 0
        probe = np.zeros((cs["nprob"], cs["n"], 8), dtype=np.uint32)
        st, g0, *_ = sort_ex(curve, probe, cs, outputs=False)
        assert st == 0, f"{cs['name']}: the plan is refused: status {st}"
        del probe
        words = build_scalars(cs, g0, cv["order"], rng)
        g, m = check_sort(curve, cs, words, cs["name"])
        assert g == g0
    finally:
        if cs["glv_bits"]:
            assert lib.msmz_test_set_glv_bits(curve._ctx, 0) == 0
    assert cs["c"] == 0 or g["c"] == cs["c"]
    for tag in cs["regimes"]:
        assert REGIMES[tag](g, cs, m), f"{cs['name']} no longer reaches its regime '{tag}': geometry {g}, error {m['error']}, " \
                                       f"largest bucket {m['largest']}, largest bin {m['largest_bin']}"


def test_every_regime_has_a_case():
    named = {t for cs in CASES for t in cs["regimes"]}
    assert named == set(REGIMES)


def test_refused_arguments(ctxs):
    """every combination the hook refuses, with its documented status and before any launch; the context sorts correctly
    afterwards"""
    curve = ctxs("bls12-377")
    base = case("args", "bls12-377", 3001, 11, [])
    words = np.zeros((1, 3001, 8), dtype=np.uint32)
    words[0, :, 0] = np.arange(3001)
    st, g, *_ = sort_ex(curve, words, base, outputs=False)
    assert st == 0 and g["two_level"] == 1
    n_off, cap, n_bins = g["nb"] + 1, g["K"] * 3001, g["sbins"] + 1

    def refused(want, cs=base, **override):
        st, _, *outs = sort_ex(curve, words, cs, **override)
        assert st == want, (override, cs, st)
        for o in outs:
            assert o is None or (o == 0xa5a5a5a5).all(), "a refused call wrote an output"

    refused(ERR_ARG, scalars_le32=None)
    refused(ERR_ARG, n=0)
    refused(ERR_ARG, n=(1 << 22) + 1)
    refused(ERR_ARG, nprob=0)
    refused(ERR_ARG, nprob=65)
    refused(ERR_ARG, factor=129)
    refused(ERR_ARG, c=25)
    refused(ERR_ARG, c=-1)
    refused(ERR_ARG, scalar_bits=257)
    refused(ERR_ARG, scalar_bits=-1)
    refused(ERR_ARG, pts_n=3000)
    refused(ERR_ARG, pts_n=(1 << 30) + 1)
    refused(ERR_ARG, geom_cap=len(_native().TEST_SORT_GEOM) - 1)
    refused(ERR_ARG, off_cap=n_off - 1)
    refused(ERR_ARG, refs_cap=cap - 1)
    refused(ERR_ARG, bins_cap=n_bins - 1)
    refused(ERR_ARG, packed_cap=cap - 1)
    # a copy index that leaves the 31-bit reference: (F - 1) * copy_stride + the last index
    refused(ERR_ARG, cs=dict(base, factor=2, c=0), copy_stride=(1 << 31) - 3000)
    # batches and precomputed sets exist in the two-level sort only
    refused(ERR_UNSUPPORTED, nprob=2, force_fallback=1)
    refused(ERR_UNSUPPORTED, cs=dict(base, factor=2, c=0), force_fallback=1)
    refused(ERR_UNSUPPORTED, cs=dict(base, c=22), nprob=2)
    # GLV on a curve without an endomorphism
    ed = ctxs("ed-on-bls12-377")
    st, *_ = sort_ex(ed, words, dict(base, glv=1), outputs=False)
    assert st == ERR_UNSUPPORTED
    # null context / args
    lib = _native().lib()
    assert lib.msmz_test_sort_ex(None, C.byref(_native().MsmzTestSortArgs())) == ERR_ARG
    assert lib.msmz_test_sort_ex(curve._ctx, None) == ERR_ARG
    # ... and the context still sorts
    check_sort(curve, base, build_scalars(base, g, P.CURVES["bls12-377"]["order"], np.random.default_rng(1)), "after refusals")

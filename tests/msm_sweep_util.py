"""The option space of the MSM as a list of cases (host only: no GPU, no native library is needed to import this).

cases(seed) is a pure function of the seed: a greedy covering of the dimensions below under the rule table RULES, which
restates which combinations include/msmz.h supports.  Every pair of values the rules allow occurs in some case, and so
does every allowed triple of TRIPLES.  A case is a plain dict; tests/native/sweep_regimes.cpp predicts its regime on
the CPU (regimes()), tests/test_msm_sweep_gpu.py runs it, tools/fuzz_parity.py is a command line over both.

Expected values are closed forms: point i of a set is m_i G with a known multiplier m_i (randomPointsFast: a_i of
oracle/prng.py; q - a_i for a negated pool point, 0 for infinity), so an MSM over a range is [sum s_i m_i mod q] G."""
import ctypes as C
import os
import random
import subprocess
import time

import numpy as np

from oracle import c_oracle
from oracle import params as P
from oracle import prng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIER = ["bls12-377", "pallas", "bls12-381"]
TE = "ed-on-bls12-377"
GLV_HALF = 127          # the bit length the windows of a GLV half are sized for (Fr::GLV_BITS - 1, all three curves)
MAX_BATCH_N = 1 << 16   # batches and segments stay at n <= 2^16 per problem
PSEED = 0x5EED

SIZE_CLASSES = ["1..64"] + [f"{form}{k}" for k in range(10, 19) for form in ("2^k-1:", "2^k:", "2^k+1:", "3*2^(k-1):")]
# (2047, 2048, 2049, the sort tile, are k = 11; 2^16 -+ 1, the two-engine block edge, are k = 16)

DIMS = {
    "curve": WEIER + [TE],
    "entry": ["msmUnsafe", "msm", "msmProjective"],
    "shape": ["single", "batch2", "batch5", "segments", "pre0", "pre2"],
    "glv": [0, 1, -1],
    "c": [0, 2, 7, 12, 16, 17, 20],
    "scalarBits": [0, 16, 64, GLV_HALF, GLV_HALF + 1, 200],
    "reduceAffine": [0, 1],
    "source": ["resident", "host"],
    "sdist": ["uniform", "equal", "sparse", "edges"],
    "pdist": ["distinct", "pooled"],
    "engines": [1, 2],
    "limits": ["default", "passes", "subbatches"],
    "size": SIZE_CLASSES,
}
NAMES = list(DIMS)
TRIPLES = [("shape", "glv", "scalarBits"), ("shape", "c", "size"), ("entry", "sdist", "size")]


def size_min(cls):
    """the smallest n of a size class"""
    if cls == "1..64":
        return 1
    form, k = cls.split(":")
    k = int(k)
    return {"2^k-1": (1 << k) - 1, "2^k": 1 << k, "2^k+1": (1 << k) + 1, "3*2^(k-1)": 3 << (k - 1)}[form]


def _pre(c):
    return c["shape"] in ("pre0", "pre2")


def _batched(c):
    return c["shape"] in ("batch2", "batch5", "segments")


def _windows(c):
    """windows of a precomputed set with an explicit window size under a scalar bound (a GLV half is no longer)"""
    return -(-(min(c["scalarBits"], GLV_HALF) + 1) // c["c"])


def _pre_coarse_bins(c):
    """coarse bins per window of a precomputed set with an explicit window size (plan.h fine_bits: the packed 31-bit word
    holds the entry index, the copy index and at most 11 fine bucket bits)"""
    n, bits = size_min(c["size"]), c["scalarBits"]
    glv = c["glv"] == 1 or (c["glv"] < 0 and n < (1 << 15) and not 0 < bits <= GLV_HALF)
    b = min(bits or 256, GLV_HALF) if glv else (bits or 256)
    copies = -(-(min(b, 255) + 1) // c["c"])
    if glv:   # the copies also cover the windows of the GLV retry, sized for the proven length of a half
        copies = max(copies, -(-((127 if c["curve"] == "bls12-377" else 128) + 1) // c["c"]))
    copies = min(copies, 2) if c["shape"] == "pre2" else copies
    idx_bits = max(((2 * n if glv else n) - 1).bit_length(), 1) + (copies - 1).bit_length()
    fb = min(31 - idx_bits, 11, c["c"] - 1)
    return 1 << (c["c"] - 1 - fb)


# (name, the fields it reads, the line it restates, violated(case)).  A rule speaks only when all its fields are set.
RULES = [
    ("te-entry", ("curve", "entry"), "msmz.h:258 / msm-basic.ts: the twisted Edwards curve has msm only (msmBasic, safe additions)",
     lambda c: c["curve"] == TE and c["entry"] != "msm"),
    ("te-glv", ("curve", "glv"), "msmz.h:61: GLV is a split on Weierstrass curves; engine.h msm_basic refuses opt.glv",
     lambda c: c["curve"] == TE and c["glv"] == 1),
    ("projective-glv", ("entry", "glv"), "parallel.ts:69-87 msmProjective: no GLV, projective buckets; msm_basic refuses opt.glv",
     lambda c: c["entry"] == "msmProjective" and c["glv"] != 0),
    ("pre-te", ("curve", "shape"), "msmz.h:327: twisted Edwards is MSMZ_ERR_UNSUPPORTED for a precomputed handle",
     lambda c: c["curve"] == TE and _pre(c)),
    ("pre-projective", ("entry", "shape"), "msmz.h:327: MSMZ_BUCKETS_PROJECTIVE is MSMZ_ERR_UNSUPPORTED for a precomputed handle",
     lambda c: c["entry"] == "msmProjective" and _pre(c)),
    ("pre-reduce-affine", ("reduceAffine", "shape"), "msmz.h:327: reserved[0] = 1 is MSMZ_ERR_UNSUPPORTED for a precomputed handle",
     lambda c: c["reduceAffine"] == 1 and _pre(c)),
    ("pre-single-window", ("shape", "c", "scalarBits"), "msmz.h:320: a bound that leaves a single window is MSMZ_ERR_ARG",
     lambda c: _pre(c) and c["c"] > 0 and c["scalarBits"] > 0 and _windows(c) < 2),
    ("pre-single-window-auto", ("shape", "c", "scalarBits"),
     "msmz.h:320: a bound that leaves a single window is MSMZ_ERR_ARG (c = 0: the engine's choice for 16-bit scalars is one window)",
     lambda c: _pre(c) and c["c"] == 0 and c["scalarBits"] == 16),
    ("pre-coarse-bins", ("curve", "shape", "c", "size", "glv", "scalarBits"),
     "msmz.h:326: a bucket set of a precomputed handle fits one pass of the two-level sort: a window at most 512 coarse bins",
     lambda c: _pre(c) and c["c"] > 0 and _pre_coarse_bins(c) > 512),
    ("segments-multi", ("shape", "engines"), "msmz.h:301: msmz_msm_segments on a multi-device context is MSMZ_ERR_UNSUPPORTED",
     lambda c: c["shape"] == "segments" and c["engines"] == 2),
    ("batch-size", ("shape", "size"), "batches and segments stay at n <= 2^16 per problem (the larger sizes are the single MSM's)",
     lambda c: _batched(c) and size_min(c["size"]) > MAX_BATCH_N),
    ("pooled-entry", ("pdist", "entry"), "msmz.h:48: msmUnsafe hits P + (+-P) on pooled points; msmProjective takes distinct points here",
     lambda c: c["pdist"] == "pooled" and c["entry"] != "msm"),
    ("passes-pre", ("limits", "shape"), "msmz_test.h:86: a precomputed set longer than a lowered pass limit is not supported",
     lambda c: c["limits"] == "passes" and _pre(c)),
    ("sub-shape", ("limits", "shape"), "msmz_test.h:85: batch_entries cuts a batch; two sub-batches of two need B = 5",
     lambda c: c["limits"] == "subbatches" and c["shape"] != "batch5"),
    ("sub-te", ("limits", "curve"), "msmz.h:273: twisted Edwards runs the problems one by one: no sub-batches",
     lambda c: c["limits"] == "subbatches" and c["curve"] == TE),
    ("sub-projective", ("limits", "entry"), "msmz.h:273: MSMZ_BUCKETS_PROJECTIVE runs the problems one by one: no sub-batches",
     lambda c: c["limits"] == "subbatches" and c["entry"] == "msmProjective"),
    ("sub-reduce-affine", ("limits", "reduceAffine"), "msmz.h:273: reserved[0] = 1 runs the problems one by one: no sub-batches",
     lambda c: c["limits"] == "subbatches" and c["reduceAffine"] == 1),
    ("sub-size", ("limits", "size"), "sub-batches need a batch (sub-shape), and batches stay at n <= 2^16 (batch-size)",
     lambda c: c["limits"] == "subbatches" and size_min(c["size"]) > MAX_BATCH_N),
]


def violated(case):
    """names of the rules a (partial) case breaks"""
    return [name for name, fields, _, bad in RULES if all(f in case for f in fields) and bad(case)]


def complete(partial, rng=None):
    """a full supported case that extends `partial`, or None: depth-first over the open dimensions, the first value of a
    dimension first (or in the order `rng` deals)"""
    if violated(partial):
        return None
    todo = [d for d in NAMES if d not in partial]
    if not todo:
        return dict(partial)
    d = todo[0]
    vals = list(DIMS[d])
    if rng:
        rng.shuffle(vals)
    for v in vals:
        got = complete(dict(partial, **{d: v}), rng)
        if got:
            return got
    return None


def targets():
    """every pair of values of two dimensions and every triple of TRIPLES -> {target: reason}: None = some supported
    case holds it, else the rule that forbids it (a target is a sorted tuple of (dimension, value))"""
    out = {}
    groups = [(a, b) for i, a in enumerate(NAMES) for b in NAMES[i + 1:]] + TRIPLES
    for dims in groups:
        combos = [()]
        for d in dims:
            combos = [t + ((d, v),) for t in combos for v in DIMS[d]]
        for t in combos:
            t = tuple(sorted(t, key=lambda dv: NAMES.index(dv[0])))
            if complete(dict(t)) is not None:
                out[t] = None
            else:
                direct = violated(dict(t))
                out[t] = direct[0] if direct else "no-rule"
    return out


def _holds(case):
    keys = []
    for i, a in enumerate(NAMES):
        for b in NAMES[i + 1:]:
            keys.append(((a, case[a]), (b, case[b])))
    for dims in TRIPLES:
        keys.append(tuple(sorted(((d, case[d]) for d in dims), key=lambda dv: NAMES.index(dv[0]))))
    return keys


# Directed cases: regimes the covering need not reach (tests/test_msm_sweep_cpu.py names each; `n` and `glvBits` fixed)
DIRECTED = [
    # the GLV redo: halves longer than an assumed 100 bits (msmz_test_set_glv_bits)
    dict(curve="bls12-377", entry="msmUnsafe", shape="single", glv=1, c=0, glvBits=100, n=3000),
    dict(curve="pallas", entry="msm", shape="batch5", glv=1, c=7, glvBits=100, n=1500),
    dict(curve="bls12-381", entry="msm", shape="segments", glv=1, c=12, glvBits=100, n=5000),
    dict(curve="bls12-377", entry="msm", shape="pre0", glv=1, c=0, glvBits=100, n=2049),
    dict(curve="pallas", entry="msmUnsafe", shape="single", glv=1, c=16, glvBits=100, n=70000, engines=2),
    # msmBasic with k_bucket_sums and a grown chunk: long buckets (c = 2), all scalars equal
    dict(curve="ed-on-bls12-377", entry="msm", shape="single", glv=0, c=2, sdist="equal", n=1 << 16),
    dict(curve="pallas", entry="msmProjective", shape="single", glv=0, c=2, sdist="uniform", n=3 << 15),
    # the fixed window, the stepped-down one (Pallas: 17 would leave one bit to the top window) and the bounded case that
    # keeps 17, at 2^18 entries per window
    dict(curve="bls12-377", entry="msmUnsafe", shape="single", glv=0, c=0, scalarBits=0, n=1 << 18),
    dict(curve="pallas", entry="msmUnsafe", shape="single", glv=0, c=0, scalarBits=0, n=1 << 18),
    dict(curve="bls12-377", entry="msm", shape="single", glv=0, c=0, scalarBits=64, n=(1 << 18) + 1),
    dict(curve="pallas", entry="msmUnsafe", shape="single", glv=1, c=0, scalarBits=0, n=1 << 17),
    # the fallback sort: a window of more than 512 coarse bins (c = 22); a batch on it falls back to problem by problem
    dict(curve="bls12-377", entry="msmUnsafe", shape="single", glv=0, c=22, n=3000),
    dict(curve="pallas", entry="msm", shape="batch2", glv=1, c=22, n=1500),
    # precomputed sets: the c = 17 branch at 2^16 entries, and two windows per set
    dict(curve="bls12-381", entry="msmUnsafe", shape="pre0", glv=0, c=0, n=1 << 16),
    dict(curve="bls12-381", entry="msm", shape="pre2", glv=0, c=0, n=1 << 16),
]
DEFAULTS = dict(curve="bls12-377", entry="msm", shape="single", glv=0, c=0, scalarBits=0, reduceAffine=0, source="resident",
                sdist="uniform", pdist="distinct", engines=1, limits="default", size=None)


def _pick_n(case, rng):
    if case["size"] != "1..64":
        return size_min(case["size"])
    return rng.randint(8 if case["limits"] == "passes" else 1, 64)   # (two passes of a GLV call need 4 points; 8 leaves ragged ones)


def cases(seed=1):
    """the case list of a seed: the covering, then DIRECTED.  Every case: the 13 dimensions, n, glvBits, id, directed."""
    rng = random.Random(seed)
    open_ = [t for t, why in targets().items() if why is None]
    rng.shuffle(open_)
    todo = dict.fromkeys(open_)
    out = []
    while todo:
        t = next(iter(todo))
        case = dict(t)
        order = [d for d in NAMES if d not in case]
        rng.shuffle(order)
        for d in order:
            best, best_gain = None, -1
            vals = list(DIMS[d])
            rng.shuffle(vals)
            for v in vals:
                trial = dict(case, **{d: v})
                if violated(trial):
                    continue
                gain = sum(1 for a in case if tuple(sorted(((a, case[a]), (d, v)), key=lambda dv: NAMES.index(dv[0]))) in todo)
                for dims in TRIPLES:
                    if d in dims and all(x in trial for x in dims):
                        gain += 3 * (tuple((x, trial[x]) for x in sorted(dims, key=NAMES.index)) in todo)
                if gain > best_gain:
                    best, best_gain = v, gain
            if best is None:
                break
            case[d] = best
        if len(case) < len(NAMES) or complete(case) is None:
            case = complete(dict(t), rng)   # the greedy choice ran into a rule: any completion of the target
        for k in _holds(case):
            todo.pop(k, None)
        out.append(case)
    for c in out:
        c["n"], c["glvBits"], c["directed"] = _pick_n(c, rng), 0, False
    for d in DIRECTED:
        c = dict(DEFAULTS, glvBits=0, directed=True)
        c.update(d)
        c["size"] = "directed"
        assert not violated({k: v for k, v in c.items() if k != "size"}), (d, violated(c))
        out.append(c)
    for i, c in enumerate(out):
        c["id"] = i
    return out


# ------------------------------------------------------------------------------------------------ the shape of a case
def batch_of(case):
    return {"batch2": 2, "batch5": 5}.get(case["shape"], 1)


def segments_of(case):
    """three segments (firstPoint, firstScalar, n): two in one length class, one in another, both offsets non-zero"""
    n = case["n"]
    low = 1 << (n.bit_length() - 1)
    same = (n + low + 1) // 2                    # low <= same <= n: the class of n
    other = n // 3 if n >= 3 else 4              # another floor(log2)
    return [(3, 5, n), (other + 1, n + 7, same), (n // 2 + 1, 2 * n + 11, other)]


def pass_entries(case):
    """the lowered pass limit of limits = passes: at least two index-range passes (GLV: a pass takes half as many points)"""
    return 2 * ((case["n"] + 3) // 4) if case["limits"] == "passes" else 0


def points_needed(case):
    if case["shape"] == "segments":
        return max(p + n for p, _, n in segments_of(case))
    return case["n"]


def scalars_needed(case):
    if case["shape"] == "segments":
        return max(s + n for _, s, n in segments_of(case))
    return batch_of(case) * case["n"]


def shard_count(n, g, G, shift=16):
    """entries of the first n on engine g of G (msm_zprize_amd.sharding.block_shard_count, restated: this module imports
    without the package)"""
    full, rem = divmod(n, G << shift)
    return (full << shift) + min(max(rem - (g << shift), 0), 1 << shift)


def share(n, engines):
    """(engine whose plan the log of a multi-engine call reports, its share of the first n entries): sets are dealt in
    blocks of 2^16 round-robin (csrc/multi.h shard_count); the logs merge in engine order, the last one's plan stays"""
    counts = [shard_count(n, g, engines) for g in range(engines)]
    g = max(i for i, v in enumerate(counts) if v)
    return g, counts[g]


# ------------------------------------------------------------------------------------------------ predicted regimes
def build_predictor():
    src = os.path.join(ROOT, "tests", "native", "sweep_regimes.cpp")
    exe = os.path.join(ROOT, "tests", "native", "sweep_regimes")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(
            os.path.join(ROOT, "msm_zprize_amd", "csrc", "plan.h"))):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src])
    return exe


def predictor_line(case, set_points):
    """the case as sweep_regimes.cpp reads it; set_points: the size of the resident point set the case is a prefix of"""
    label = case["curve"]
    basic = label == TE or case["entry"] == "msmProjective"
    e = case["engines"]
    g, n = share(case["n"], e)
    pts_n = shard_count(set_points, g, e)   # the reporting engine's share of the set
    shape = {"single": 0, "batch2": 1, "batch5": 1, "segments": 2, "pre0": 3, "pre2": 3}[case["shape"]]
    if shape == 3:
        pts_n = n   # the precomputed handle holds exactly the case's points
    lens = [s[2] for s in segments_of(case)] if shape == 2 else [0, 0, 0]
    glv = 0 if case["entry"] == "msmProjective" else case["glv"]
    v = [case["id"], P.CURVES[label]["curve_id"], n, pts_n, case["n"], glv, case["c"], case["scalarBits"], shape,
         batch_of(case), 2 if case["shape"] == "pre2" else 0, int(basic), case["reduceAffine"], pass_entries(case),
         int(case["limits"] == "subbatches"), case["glvBits"], *lens, int(label != TE)]
    return " ".join(str(int(x)) for x in v)


def regimes(case_list, set_points):
    """{case id: the predicted regime, a dict of ints and strings}"""
    exe = build_predictor()
    text = "\n".join(predictor_line(c, set_points(c) if callable(set_points) else set_points) for c in case_list) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
    out = {}
    for line in r.stdout.splitlines():
        d = {}
        for word in line.split():
            k, v = word.split("=")
            d[k] = int(v) if v.lstrip("-").isdigit() else v
        out[d["id"]] = d
    return out


# the size of the shared point and scalar sets of the sweep: the largest single MSM, five vectors of 2^16, the segments
SET_POINTS = (3 << 17) + 64
SET_SCALARS = max(SET_POINTS, 5 * MAX_BATCH_N + 64)


# ------------------------------------------------------------------------------------------------ inputs, closed form
def bound_of(q, bits):
    """scalars of a case lie below this: min(q, 2^bits), q without a bound"""
    return q if bits == 0 or (1 << bits) >= q else 1 << bits


def _words(values):
    return np.array([[(v >> (64 * j)) & prng.MASK64 for j in range(4)] for v in values], dtype=np.uint64)


def scalar_words(label, sdist, bits, n, seed=0):
    """n scalars of a distribution as (n, 4) little-endian uint64 words, all below bound_of(q, bits)"""
    q = P.CURVES[label]["order"]
    top = bound_of(q, bits)
    sd = (hash_seed(label, sdist, bits) + seed) & prng.MASK64
    if top == q:
        uni = prng.scalars_np(sd, n, q)
    else:
        idx = np.arange(n, dtype=np.uint64) * np.uint64(4)
        uni = np.stack([prng.splitmix64_np(sd, idx + np.uint64(j)) for j in range(4)], axis=1)
        for j in range(4):
            lo = 64 * j
            uni[:, j] &= np.uint64(0 if bits <= lo else (1 << min(64, bits - lo)) - 1)
    if sdist == "uniform":
        return uni
    if sdist == "equal":
        v = int.from_bytes(uni[0].astype("<u8").tobytes(), "little") or 1
        return np.repeat(_words([v]), n, axis=0)
    pick = prng.splitmix64_np(sd ^ 0xA5A5, np.arange(n, dtype=np.uint64))
    if sdist == "sparse":
        uni[pick % np.uint64(10) != 0] = 0
        return uni
    assert sdist == "edges"
    nbits = (top - 1).bit_length()
    special = [0, 1, top - 1, top - 1, 1 << (nbits - 1) if (1 << (nbits - 1)) < top else 1, 2]
    special += [(1 << j) - 1 for j in (2, 7, 12, 16, 17, 20, 31, 33, 63, 64, 65, 126, 127, 128, 200) if j < nbits]   # windows of ones
    return _words(special)[(pick % np.uint64(len(special))).astype(np.int64)]


def hash_seed(*parts):
    h = 0xCBF29CE484222325
    for ch in repr(parts).encode():
        h = ((h ^ ch) * 0x100000001B3) & prng.MASK64
    return h


POOL_BASE = (1, 3, 5)   # the pool: these three points of the distinct set, their negatives, infinity


def pool_layout(n):
    """the pooled point set over indices 0 .. n-1: even entries come from the pool -- value (i // 2 // 3) % 7: base 0, 1,
    2, their negatives, infinity -- odd entries are the distinct set's.  -> (val, -1 where distinct)"""
    i = np.arange(n)
    val = ((i // 2) // 3) % 7
    return np.where(i % 2 == 0, val, -1)


def multipliers(pdist, n):
    """(a, sign): point i = sign_i a_i G, sign in {1, -1, 0}"""
    a = prng.multipliers_np(PSEED, n)
    sign = np.ones(n, dtype=np.int64)
    if pdist == "pooled":
        val = pool_layout(n)
        pooled = val >= 0
        base = np.array([a[k] for k in POOL_BASE], dtype=np.uint64)
        a = a.copy()
        a[pooled & (val < 6)] = base[val[pooled & (val < 6)] % 3]
        sign[pooled & (val >= 3)] = -1
        sign[pooled & (val == 6)] = 0
    return a, sign


def expected_scalar(q, s_words, a, sign):
    """sum_i s_i sign_i a_i mod q"""
    pos, neg = sign > 0, sign < 0
    t = prng.sum_of_products_mod(s_words[pos], a[pos], q) if pos.any() else 0
    if neg.any():
        t -= prng.sum_of_products_mod(s_words[neg], a[neg], q)
    return t % q


def problems_of(case):
    """the (firstPoint, firstScalar, n) of every problem of a case over the shared sets"""
    if case["shape"] == "segments":
        return segments_of(case)
    return [(0, k * case["n"], case["n"]) for k in range(batch_of(case))]


def options_of(case):
    o = {"c": case["c"], "glv": case["glv"], "reduceAffine": case["reduceAffine"]}
    if case["scalarBits"]:
        o["scalarBits"] = case["scalarBits"]
    if case["entry"] == "msmProjective":
        o["glv"] = 0
    return o


# ------------------------------------------------------------------------------------------------ running a case (GPU)
class Scalars:
    """one shared scalar set: its words, its wire bytes and (per context) the resident copy"""

    def __init__(self, label, sdist, bits):
        self.words = scalar_words(label, sdist, bits, SET_SCALARS)
        self.bytes = self.words.astype("<u8").tobytes()


_scalar_sets = {}


def scalar_set(label, sdist, bits):
    key = (label, sdist, bits)
    if key not in _scalar_sets:
        _scalar_sets[key] = Scalars(*key)
    return _scalar_sets[key]


class Env:
    """One (curve, engines) context: the distinct point set of the largest size, the pooled set made from it, resident
    copies of the scalar sets, and the multipliers of both point sets."""

    def __init__(self, mod, label, engines):
        self.label, self.params = label, P.CURVES[label]
        self.q = self.params["order"]
        mod.startThreads(devices=[0] * engines)
        params = mod.curves.BY_LABEL[label]
        self.curve = (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)
        mod.startThreads()
        self.par = self.curve.Parallel
        self.points = {"distinct": self.par.randomPointsFast(SET_POINTS, PSEED)}
        self.mult = {}
        self.resident = {}
        self.expected = {}

    def point_set(self, pdist):
        if pdist not in self.points:
            from msm_zprize_amd._native import check, lib
            n, fb, p = SET_POINTS, self.params["fe_bytes"], self.params["modulus"]
            raw = C.create_string_buffer(2 * fb * n)
            inf = C.create_string_buffer(n)
            check(lib().msmz_download_points(self.curve._ctx, self.points["distinct"].handle, 0, n, raw, inf), "download")
            rows = np.frombuffer(raw.raw, dtype=np.uint8).reshape(n, 2 * fb).copy()
            pool = [rows[k].copy() for k in POOL_BASE]
            for k in range(3):
                neg = pool[k].copy()
                lo, hi = (fb, 2 * fb) if self.label in WEIER else (0, fb)   # -(x, y) = (x, -y); twisted Edwards: (-x, y)
                v = int.from_bytes(neg[lo:hi].tobytes(), "little")
                neg[lo:hi] = np.frombuffer(((p - v) % p).to_bytes(fb, "little"), dtype=np.uint8)
                pool.append(neg)
            zero = np.zeros(2 * fb, dtype=np.uint8)
            if self.label not in WEIER:
                zero[fb] = 1   # the identity (0, 1): the twisted Edwards curve has no flag
            pool.append(zero)
            val = pool_layout(n)
            rows[val >= 0] = np.stack(pool)[val[val >= 0]]
            flags = ((val == 6) & (self.label in WEIER)).astype(np.uint8)
            self.points[pdist] = self.par.pointsFromBytes(rows.tobytes(), n, flags.tobytes())
        return self.points[pdist]

    def multipliers(self, pdist):
        if pdist not in self.mult:
            self.mult[pdist] = multipliers(pdist, SET_POINTS)
        return self.mult[pdist]

    def resident_scalars(self, sdist, bits):
        key = (sdist, bits)
        if key not in self.resident:
            self.resident[key] = self.par.scalarsFromBytes(scalar_set(self.label, sdist, bits).bytes, SET_SCALARS)
        return self.resident[key]

    def want(self, pdist, sdist, bits, first_p, first_s, n):
        """the expected point of one problem, computed once per range"""
        key = (pdist, sdist, bits, first_p, first_s, n)
        if key not in self.expected:
            a, sign = self.multipliers(pdist)
            words = scalar_set(self.label, sdist, bits).words
            t = expected_scalar(self.q, words[first_s:first_s + n], a[first_p:first_p + n], sign[first_p:first_p + n])
            g = self.params["generator"]
            r = c_oracle.scale(self.params, t, {"x": g["x"], "y": g["y"], "isZero": False})
            self.expected[key] = (r["x"], r["y"], bool(r.get("isZero", False)) and self.label in WEIER)
        return self.expected[key]

    def counters(self):
        from msm_zprize_amd._native import lib
        rp, sb = C.c_uint64(), C.c_uint64()
        assert lib().msmz_test_passes(self.curve._ctx, C.byref(rp), C.byref(sb)) == 0
        return rp.value, sb.value, lib().msmz_test_retries(self.curve._ctx)


def _pt(label, p):
    return (p["x"], p["y"], bool(p.get("isZero", False)) and label in WEIER)


def run_case(sweep, env, case):
    """-> (results, the call's log): the case through the entry point, shape, source and hooks it names"""
    from msm_zprize_amd._native import lib
    par, n = env.par, case["n"]
    pts = env.point_set(case["pdist"])
    opts = options_of(case)
    res = env.resident_scalars(case["sdist"], case["scalarBits"])
    host = scalar_set(env.label, case["sdist"], case["scalarBits"]).bytes
    entry, shape, B = case["entry"], case["shape"], batch_of(case)
    ctx = env.curve._ctx
    reg = sweep.regimes[case["id"]]
    assert lib().msmz_test_set_limits(ctx, pass_entries(case), reg.get("cap", 0)) == 0
    if case["glvBits"]:
        assert lib().msmz_test_set_glv_bits(ctx, case["glvBits"]) == 0
    pre = None
    try:
        if shape in ("single", "pre0", "pre2"):
            if shape != "single":
                pre = pts = par.precomputePoints(pts, n, opts, 2 if shape == "pre2" else 0)
            sc = res if case["source"] == "resident" else host[:32 * n]
            if entry == "msmProjective":
                r = par.msmProjective(sc, pts, n, opts)
            else:
                r = getattr(par, entry)(sc, pts, n, False, opts)
            return [_pt(env.label, r["result"])], r["stats"]
        if entry == "msmProjective":
            opts["buckets"] = 1
        unsafe = "Unsafe" if entry == "msmUnsafe" else ""
        if shape == "segments":
            got = getattr(par, "msmSegments" + unsafe)(res, pts, segments_of(case), opts)
        else:
            sc = res if case["source"] == "resident" else [host[32 * k * n:32 * (k + 1) * n] for k in range(B)]
            got = getattr(par, "msmBatch" + unsafe)(sc, pts, n, dict(opts, batch=B))
        return [_pt(env.label, r) for r in got], par.lastBatchLog
    finally:
        if pre is not None:
            pre.free()
        assert lib().msmz_test_set_limits(ctx, 0, 0) == 0
        if case["glvBits"]:
            assert lib().msmz_test_set_glv_bits(ctx, 0) == 0


def check_case(sweep, env, case):
    reg = sweep.regimes[case["id"]]
    assert reg["status"] == 0, f"the planner refuses a generated case: {case} {reg}"
    want = [env.want(case["pdist"], case["sdist"], case["scalarBits"], fp, fs, n) for fp, fs, n in problems_of(case)]
    r0, s0, t0 = env.counters()
    got, log = run_case(sweep, env, case)
    r1, s1, t1 = env.counters()
    rp, sb, redo = r1 - r0, s1 - s0, t1 - t0
    said = {k: getattr(log, k) for k in ("c", "K", "glv", "rounds", "n_entries", "n_pairs", "max_bucket")}
    said.update(range_passes=rp, sub_batches=sb, retries=redo)
    msg = f"\ncase: {case}\npredicted: {reg}\nreported: {said}"
    wrong = [k for k in range(len(want)) if k >= len(got) or got[k] != want[k]]
    assert got == want, f"result differs from the closed form (problems {wrong} of {len(want)})" + msg
    # it ran the plan it was chosen for
    c, K = (reg["redo_c"], reg["redo_K"]) if case["glvBits"] else (reg["c"], reg["K"])
    assert (said["c"], said["K"], said["glv"]) == (c, K, reg["glv"]), "not the predicted plan" + msg
    if case["glvBits"]:
        assert redo >= 1, "no GLV redo" + msg
        sweep.observed["glv_redo"] += 1
    B = len(want)
    if reg["bs"] > 1:
        assert sb >= (2 if case["limits"] == "subbatches" else 1), "no batched pipeline" + msg
    elif case["engines"] == 1 and B == 1:
        assert (rp, sb) == (reg["passes"], 0), "not the predicted index-range passes" + msg
    if reg["per_problem"]:
        assert sb == 0 and rp >= B, "the batch did not run problem by problem" + msg
        sweep.observed["per_problem"] += 1
    if case["limits"] == "passes":
        # (a lower bound: with GLV a pass takes half as many points)
        least = sum(-(-n // pass_entries(case)) for _, _, n in problems_of(case))
        assert least > B and rp >= least, "fewer index-range passes than the lowered limit asks for" + msg
        sweep.observed["range_passes"] += 1
    if case["limits"] == "subbatches":
        sweep.observed["sub_batches"] += 1
    if B == 1 and case["limits"] == "default" and case["engines"] == 1 and \
            (env.label == TE or case["entry"] == "msmProjective"):
        # msmBasic (engine.h msm_basic): chunks of 2^shift entries, shift raised to ~sqrt of the longest bucket;
        # k_bucket_sums runs when the chunk accumulators outnumber the buckets 3 : 2
        shift = 5
        while (1 << (2 * shift)) < said["max_bucket"]:
            shift += 1
        nb = reg["Keff"] * reg["L"]
        full = said["n_entries"] >> shift   # a lower bound of the chunks; + nb is an upper bound
        sweep.observed["basic_summed"] += 2 * full > 3 * nb
        sweep.observed["basic_plain"] += 2 * (full + nb) <= 3 * nb
        sweep.observed["chunk_grown"] += said["max_bucket"] > 1024
    sweep.observed["cases"] += 1


class Sweep:
    """The cases of a seed with their predicted regimes, the contexts they run in and what running them has shown."""

    def __init__(self, seed=1):
        self.cases = cases(seed)
        self.regimes = regimes(self.cases, SET_POINTS)
        self.envs = {}
        self.observed = {"cases": 0, "range_passes": 0, "sub_batches": 0, "per_problem": 0, "basic_summed": 0,
                         "basic_plain": 0, "chunk_grown": 0, "glv_redo": 0, "seconds": 0.0}

    def env(self, label, engines):
        if (label, engines) not in self.envs:
            import msm_zprize_amd as m
            self.envs[(label, engines)] = Env(m, label, engines)
        return self.envs[(label, engines)]

    def run(self, case):
        """one case; AssertionError with the case, the predicted regime and what the call reported if it fails"""
        t0 = time.time()
        try:
            check_case(self, self.env(case["curve"], case["engines"]), case)
        except AssertionError:
            raise
        except Exception as e:   # a status other than MSMZ_OK fails the case like a mismatch
            raise AssertionError(f"{type(e).__name__}: {e}\ncase: {case}\npredicted: {self.regimes[case['id']]}") from e
        self.observed["seconds"] += time.time() - t0

    def close(self):
        for e in self.envs.values():
            e.curve.close()
        self.envs.clear()

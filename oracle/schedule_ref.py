"""Plain model of the tree-round schedule (msm_zprize_amd/csrc/plan_kernels.h), for tests/test_plan_schedule_*.py.

Two independent things:

  reference_rounds(sizes)   the reference's in-place rule (msm-batched-affine.ts:232-247): for m = 1, 2, 4, ... below the
                            largest bucket size, inside every bucket, element j*2m + m is added into element j*2m while
                            j*2m + m < size.  Per round the additions as (bucket, posA, posB).
  expand(desc, bfin, ...)   a symbolic replay of what the device wrote: every location word resolves to an original
                            reference or to a record, a record to its two operands, so that every record and every final
                            location stands for a contiguous range of positions of one bucket.  It knows nothing of how
                            the kernels number their pairs; it only follows the words.

Everything is numpy-vectorized over ranges (bucket, lo, hi), round by round: the largest cases have 2^24 entries.
"""
import numpy as np

LOC_ORIG, LOC_NEG, LOC_NONE = 0x40000000, 0x80000000, 0xFFFFFFFF
LOC_IDX = 0x3FFFFFFF
META_WORDS = 68       # MsmMeta (csrc/kernels.h): max_bucket, n_entries, error, rounds, round_pairs[32], round_base[32]


class ScheduleError(AssertionError):
    """A descriptor list that is no schedule; names the round, the pair (inside the round) and the bucket where known"""

    def __init__(self, what, round=None, pair=None, bucket=None, record=None):
        self.what, self.round, self.pair, self.bucket, self.record = what, round, pair, bucket, record
        at = ", ".join(f"{k} {v}" for k, v in (("round", round), ("pair", pair), ("bucket", bucket), ("record", record))
                       if v is not None)
        super().__init__(f"{what} ({at})" if at else what)


def parse_meta(words):
    w = np.asarray(words, dtype=np.uint32)
    assert w.shape == (META_WORDS,)
    return dict(max_bucket=int(w[0]), n_entries=int(w[1]), error=int(w[2]), rounds=int(w[3]),
                round_pairs=w[4:36].astype(np.int64), round_base=w[36:68].astype(np.int64))


def plan_rounds(max_size, tail_skip):
    """rounds the plan schedules: ceil(log2 max) - tail_skip, at least 1 when a bucket has two entries, 0 when none has"""
    if max_size <= 1:
        return 0
    full = (max_size - 1).bit_length()          # rounds m = 1, 2, 4, ... < max_size
    return max(1, full - tail_skip)


def pairs_in_round(sizes, r):
    """number of j with j * 2^(r+1) + 2^r < size, per bucket"""
    s = np.asarray(sizes, dtype=np.int64)
    return np.maximum(s - (1 << r) + (2 << r) - 1, 0) // (2 << r)


def reference_round(sizes, r):
    """the additions of round r (m = 2^r) as arrays (bucket, posA, posB), bucket by bucket, j ascending"""
    s = np.asarray(sizes, dtype=np.int64)
    cnt = pairs_in_round(s, r)
    first = np.cumsum(cnt) - cnt
    bucket = np.repeat(np.arange(len(s), dtype=np.int64), cnt)
    j = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(first, cnt)
    pos_a = j << (r + 1)
    return bucket, pos_a, pos_a + (1 << r)


def reference_rounds(sizes):
    """every round m = 1, 2, 4, ... < max size"""
    s = np.asarray(sizes, dtype=np.int64)
    mx = int(s.max(initial=0))
    out, r = [], 0
    while (1 << r) < mx:
        out.append(reference_round(s, r))
        r += 1
    return out


class Expanded:
    """what expand() found: per record its bucket and the ranges [lo, mid) + [mid, hi) it adds; per final location of
    `bfin` (in bucket order) its bucket and range; per bucket the number of final locations"""

    def __init__(self, rec_bucket, rec_lo, rec_mid, rec_hi, fin_bucket, fin_lo, fin_hi, fin_count):
        self.rec_bucket, self.rec_lo, self.rec_mid, self.rec_hi = rec_bucket, rec_lo, rec_mid, rec_hi
        self.fin_bucket, self.fin_lo, self.fin_hi, self.fin_count = fin_bucket, fin_lo, fin_hi, fin_count


def _first(mask):
    return int(np.flatnonzero(mask)[0])


def expand(desc, bfin, meta, off, refs):
    """Replays desc (pairs x 2 location words), round after round as meta (parse_meta's dict, or the 68 words) lays
    them out, then bfin (buckets x 4 words).  refs must carry a distinct index per entry: an original word is placed by
    its index.  Raises ScheduleError unless
      * every original word names an entry of refs, with that entry's negate bit;
      * both operands of a round-r pair are originals or records below round r's base (launch order);
      * the two operands of a pair are adjacent ranges of the same bucket, lower one first;
      * every record is consumed exactly once, by a later pair or by bfin;
      * bfin[g] is 0 .. 4 locations, then LOC_NONE, which tile positions 0 .. size-1 of bucket g in order."""
    if not isinstance(meta, dict):
        meta = parse_meta(meta)
    off = np.asarray(off, dtype=np.int64)
    refs = np.asarray(refs, dtype=np.uint32)
    nb, n = len(off) - 1, int(off[-1])
    assert len(refs) == n
    sizes = np.diff(off)
    desc = np.asarray(desc, dtype=np.uint32).reshape(-1, 2)
    bfin = np.asarray(bfin, dtype=np.uint32).reshape(-1, 4)
    if len(bfin) != nb:
        raise ScheduleError(f"bfin has {len(bfin)} buckets, off has {nb}")
    rounds = meta["rounds"]
    if not 0 <= rounds <= 32:
        raise ScheduleError(f"{rounds} rounds")
    ridx = (refs & 0x7FFFFFFF).astype(np.int64)
    inv = np.full(int(ridx.max(initial=-1)) + 1, -1, dtype=np.int64)
    inv[ridx] = np.arange(n, dtype=np.int64)
    if n and not np.array_equal(inv[ridx], np.arange(n)):
        raise ValueError("expand() needs refs with a distinct index per entry")
    rneg = (refs >> 31).astype(np.int64)

    total = len(desc)
    rec_bucket = np.full(total, -1, dtype=np.int64)
    rec_lo = np.zeros(total, dtype=np.int64)
    rec_mid = np.zeros(total, dtype=np.int64)
    rec_hi = np.zeros(total, dtype=np.int64)
    consumed = []          # record numbers used as operands, all rounds and bfin

    def resolve(words, limit, fail):
        """(bucket, lo, hi) of every word; fail(i, what, record=None) raises for word i"""
        w = words.astype(np.int64)
        orig = (w & LOC_ORIG) != 0
        b = np.empty(len(w), dtype=np.int64)
        lo = np.empty(len(w), dtype=np.int64)
        hi = np.empty(len(w), dtype=np.int64)
        io = np.flatnonzero(orig)
        idx = w[io] & LOC_IDX
        bad = idx >= len(inv)
        if bad.any():
            fail(int(io[_first(bad)]), f"original word names index {int(idx[_first(bad)])}, no entry has it")
        e = inv[idx]
        if (e < 0).any():
            fail(int(io[_first(e < 0)]), f"original word names index {int(idx[_first(e < 0)])}, no entry has it")
        neg = (w[io] >> 31) & 1
        if (neg != rneg[e]).any():
            k = _first(neg != rneg[e])
            g = int(np.searchsorted(off, e[k], side="right") - 1)
            fail(int(io[k]), f"negate bit {int(neg[k])} on entry {int(e[k])} (bucket {g}, position {int(e[k] - off[g])}), "
                             f"refs has {int(rneg[e[k]])}")
        g = np.searchsorted(off, e, side="right") - 1
        b[io], lo[io], hi[io] = g, e - off[g], e - off[g] + 1
        ir = np.flatnonzero(~orig)
        rw = w[ir]
        if (rw >= limit).any():
            k = _first(rw >= limit)
            fail(int(ir[k]), f"operand is record {int(rw[k])}, not below {limit}: not written before this launch",
                 record=int(rw[k]))
        if (rec_bucket[rw] < 0).any():
            k = _first(rec_bucket[rw] < 0)
            fail(int(ir[k]), f"operand is record {int(rw[k])}, which no round wrote", record=int(rw[k]))
        b[ir], lo[ir], hi[ir] = rec_bucket[rw], rec_lo[rw], rec_hi[rw]
        consumed.append(rw)
        return b, lo, hi

    for r in range(rounds):
        base, cnt = int(meta["round_base"][r]), int(meta["round_pairs"][r])
        if base < 0 or cnt < 0 or base + cnt > total:
            raise ScheduleError(f"round spans records {base} .. {base + cnt}, desc has {total}", round=r)

        def fail(i, what, record=None, r=r, cnt=cnt):
            raise ScheduleError(("operand B: " if i >= cnt else "operand A: ") + what, round=r, pair=i % max(cnt, 1),
                                record=record)

        words = np.concatenate([desc[base:base + cnt, 0], desc[base:base + cnt, 1]])
        b, lo, hi = resolve(words, base, fail)
        ba, bb = b[:cnt], b[cnt:]
        if (ba != bb).any():
            k = _first(ba != bb)
            raise ScheduleError(f"operands from buckets {int(ba[k])} and {int(bb[k])}", round=r, pair=k, bucket=int(ba[k]))
        if (hi[:cnt] != lo[cnt:]).any():
            k = _first(hi[:cnt] != lo[cnt:])
            raise ScheduleError(f"operand A = positions [{int(lo[k])}, {int(hi[k])}), operand B = [{int(lo[cnt + k])}, "
                                f"{int(hi[cnt + k])}): not adjacent", round=r, pair=k, bucket=int(ba[k]))
        sl = slice(base, base + cnt)
        if (rec_bucket[sl] >= 0).any():
            raise ScheduleError("rounds overlap in desc", round=r)
        rec_bucket[sl], rec_lo[sl], rec_mid[sl], rec_hi[sl] = ba, lo[:cnt], hi[:cnt], hi[cnt:]

    unwritten = rec_bucket < 0
    if unwritten.any():
        raise ScheduleError("record belongs to no round", record=_first(unwritten))

    # ---- bfin
    valid = bfin != LOC_NONE
    if (valid[:, 1:] & ~valid[:, :-1]).any():
        g = _first((valid[:, 1:] & ~valid[:, :-1]).any(axis=1))
        raise ScheduleError(f"bfin = {[hex(int(x)) for x in bfin[g]]}: a location after LOC_NONE", bucket=g)
    fin_count = valid.sum(axis=1).astype(np.int64)
    fg, fk = np.nonzero(valid)              # row-major: bucket by bucket, word by word

    def fail_fin(i, what, record=None):
        raise ScheduleError(f"bfin word {int(fk[i])}: " + what, bucket=int(fg[i]), record=record)

    b, lo, hi = resolve(bfin[fg, fk], total, fail_fin)

    # ---- every record consumed exactly once
    uses = np.bincount(np.concatenate(consumed), minlength=total) if total else np.zeros(0, dtype=np.int64)
    for bad, what in ((uses > 1, "record consumed twice"), (uses == 0, "record never consumed")):
        if bad.any():
            t = _first(bad)
            r = int(np.searchsorted(meta["round_base"][:rounds], t, side="right") - 1)
            raise ScheduleError(f"{what}: positions [{int(rec_lo[t])}, {int(rec_hi[t])})", round=r,
                                pair=t - int(meta["round_base"][r]), bucket=int(rec_bucket[t]), record=t)

    # ---- bfin tiles every bucket
    if (b != fg).any():
        k = _first(b != fg)
        raise ScheduleError(f"bfin word {int(fk[k])} stands for bucket {int(b[k])}", bucket=int(fg[k]))
    empty_wrong = (fin_count == 0) != (sizes == 0)
    if empty_wrong.any():
        g = _first(empty_wrong)
        raise ScheduleError(f"{int(fin_count[g])} final locations for {int(sizes[g])} entries", bucket=g)
    first = fk == 0
    last = np.ones(len(fg), dtype=bool)
    last[:-1] = fg[1:] != fg[:-1]
    want_lo = np.where(first, 0, np.concatenate([[0], hi[:-1]]))
    if (lo != want_lo).any():
        k = _first(lo != want_lo)
        raise ScheduleError(f"bfin word {int(fk[k])} starts at position {int(lo[k])}, expected {int(want_lo[k])}",
                            bucket=int(fg[k]))
    if (hi[last] != sizes[fg[last]]).any():
        k = np.flatnonzero(last)[_first(hi[last] != sizes[fg[last]])]
        raise ScheduleError(f"bfin ends at position {int(hi[k])} of {int(sizes[fg[k]])}", bucket=int(fg[k]))
    return Expanded(rec_bucket, rec_lo, rec_mid, rec_hi, fg.astype(np.int64), lo, hi, fin_count)

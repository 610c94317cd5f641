"""Plain model of the bucket sort (msm_zprize_amd/csrc/sort_kernels.h and the fallback in kernels.h), for
tests/test_sort_*.py.  Written from the rule the planner documents (csrc/plan.h: SortGeom, Plan) and the reference's
slicing (msm-batched-affine.ts:180-199, 444-490), not from the kernels:

  a (half-)scalar of magnitude s and sign sg has K signed c-bit digits l_k in [0, L], L = 2^(c-1), sum (+-) l_k 2^(ck) = s;
  every non-zero digit is one ENTRY of bucket set (window) k, bucket weight l_k; entry number e = half * n + scalar index.
    plain           bucket k L + l - 1
    spread top      window K - 1 is dealt over 2^spread bucket sets by e mod 2^spread: (K - 1 + e mod 2^spread) L + l - 1
    folded top      window K - 1 keeps one set, weight (e mod 2^fold_rows) 2^fold_shift + l; a digit above 2^fold_shift
                    does not fit, is dropped and flagged (error bit value 2)
    F windows/set   window k adds into set k div F and references copy k mod F of the points
  reference word    index | negate << 31, index = e (+ endo_delta for the second GLV half) + (k mod F) copy_stride
  error             value 4: a scalar >= the group order or >= 2^sbits (it contributes nothing); value 2: a (half-)scalar
                    that does not fit K windows (a carry out of the last one, or bits beyond it), or a fold overflow.

The two-level sort's intermediates follow from the geometry words (fb / fbt fine bits, ncb / ncbt coarse bins per set):
  bucket index bi (weight - 1) = coarse << fbits | fine, fbits = fbt in the plain top window, fb elsewhere
  scan bin          k ncb + coarse; plain top window (K - 1) ncb + (e mod 2^spread) ncbt + coarse;
                    F > 1: ((k div F) ncb + coarse) F + k mod F
  packed word       ((fine << 1 | negate) << idx_bits) | (k mod F) << mbits | e

Everything is numpy-vectorized over the n scalars (the largest cases have 2^22 of them); the window loop is the only
Python loop.  Geometry: a dict with the names of msm_zprize_amd._native.TEST_SORT_GEOM.
"""
import numpy as np


def to_words(values, words):
    """Python integers -> (len, words) uint32 little-endian words"""
    raw = b"".join(int(v).to_bytes(4 * words, "little") for v in values)
    return np.frombuffer(raw, dtype="<u4").reshape(len(values), words).astype(np.uint32)


def words_geq(words, bound):
    """per row: value >= bound (a Python integer)"""
    n, W = words.shape
    if bound >= 1 << (32 * W):
        return np.zeros(n, dtype=bool)
    b = to_words([bound], W)[0]
    gt = np.zeros(n, dtype=bool)
    eq = np.ones(n, dtype=bool)
    for j in range(W - 1, -1, -1):
        gt |= eq & (words[:, j] > b[j])
        eq &= words[:, j] == b[j]
    return gt | eq


def flagged(scalar_words, q, sbits):
    """scalars that contribute nothing and raise error value 4: not below the group order or not below 2^sbits"""
    bad = words_geq(scalar_words, q)
    if 0 < sbits < 256:
        bad |= words_geq(scalar_words, 1 << sbits)
    return bad


def _bits_from(words, pos):
    """per row: is any bit at position >= pos set"""
    n, W = words.shape
    wi, sh = pos >> 5, pos & 31
    out = np.zeros(n, dtype=bool)
    if wi < W:
        out |= (words[:, wi] >> np.uint32(sh)) != 0
        for j in range(wi + 1, W):
            out |= words[:, j] != 0
    return out


def signed_digits(words, c, K):
    """(n, W) magnitudes -> l (n, K) int64 in [0, L], carry (n, K) uint8 (1 = the digit counts negatively), and
    overflow (n) bool: the value does not fit K windows"""
    n, W = words.shape
    L = 1 << (c - 1)
    w64 = np.concatenate([words.astype(np.uint64), np.zeros((n, 2), dtype=np.uint64)], axis=1)
    l = np.zeros((n, K), dtype=np.int64)
    cy = np.zeros((n, K), dtype=np.uint8)
    carry = np.zeros(n, dtype=np.int64)
    for k in range(K):
        pos = k * c
        wi, sh = pos >> 5, pos & 31
        if wi < W:
            v = ((w64[:, wi] | (w64[:, wi + 1] << np.uint64(32))) >> np.uint64(sh)) & np.uint64((1 << c) - 1)
        else:
            v = np.zeros(n, dtype=np.uint64)
        d = v.astype(np.int64) + carry
        over = d > L
        l[:, k] = np.where(over, 2 * L - d, d)
        carry = over.astype(np.int64)
        cy[:, k] = carry
    return l, cy, (carry != 0) | _bits_from(words, K * c)


def problem_entries(halves, bad, geom, n, copy_stride=0, detail=True):
    """The entries of one problem.  halves: [(magnitude words (n, W), sign (n))], one half or the two GLV halves; bad:
    flagged scalars (n, bool).  Returns a dict of flat arrays over the entries -- bucket (inside the problem), ref, sbin
    (scan bin inside the problem), packed -- plus error; with detail also window and entry (number) per entry and the
    digits per half."""
    c, K, L = geom["c"], geom["K"], geom["L"]
    F, spread = max(1, geom["F"]), geom["spread"]
    fs, fr = geom["fold_shift"], geom["fold_rows"]
    fb, fbt, ncb, ncbt = geom["fb"], geom["fbt"], geom["ncb"], geom["ncbt"]
    assert L == 1 << (c - 1) and not (fs and spread) and (F == 1 or (spread == 0 and fs == 0))
    error = 4 if bad.any() else 0
    cols = dict(bucket=[], ref=[], sbin=[], packed=[], window=[], entry=[])
    digits = []
    for h, (mag, sign) in enumerate(halves):
        mag = np.where(bad[:, None], np.uint32(0), mag)
        sign = np.where(bad, 0, np.asarray(sign)).astype(np.int64)
        l, cy, overflow = signed_digits(mag, c, K)
        if overflow.any():
            error |= 2
        ng = (cy.astype(np.int64) ^ sign[:, None]) & (l != 0)
        if detail:
            digits.append((l, ng))
        entry = h * n + np.arange(n, dtype=np.int64)
        for k in range(K):
            lk = l[:, k]
            keep = lk != 0
            top = k == K - 1 and F == 1
            if top and fs:
                lost = lk > (1 << fs)
                if lost.any():
                    error |= 2
                keep &= ~lost
            e, lk, neg = entry[keep], lk[keep], ng[keep, k]
            bi, sub, fbits = lk - 1, 0, fb
            if top:
                fbits = fbt
                if fs:
                    bi = ((e & ((1 << fr) - 1)) << fs) + lk - 1
                else:
                    sub = e & ((1 << spread) - 1)
            copy = k % F
            cols["bucket"].append(((k // F) + sub) * L + bi)
            cols["ref"].append((e + (geom["endo_delta"] if h else 0) + copy * copy_stride) | (neg << 31))
            coarse, fine = bi >> fbits, bi & ((1 << fbits) - 1)
            if F > 1:
                sbin = ((k // F) * ncb + coarse) * F + copy
            elif top:
                sbin = k * ncb + sub * ncbt + coarse
            else:
                sbin = k * ncb + coarse
            cols["sbin"].append(sbin + np.zeros_like(e))
            cols["packed"].append((((fine << 1) | neg) << geom["idx_bits"]) | (copy << geom["mbits"]) | e)
            if detail:
                cols["window"].append(np.full(len(e), k, dtype=np.int64))
                cols["entry"].append(e)
    out = {name: (np.concatenate(v) if v else np.zeros(0, dtype=np.int64)) for name, v in cols.items()}
    out["error"] = error
    out["digits"] = digits
    return out


def keyed(key, word):
    """(key, word) pairs as one sorted array of key << 32 | word: equal as multisets per key <=> equal arrays"""
    k = (np.asarray(key).astype(np.uint64) << np.uint64(32)) | np.asarray(word).astype(np.uint64)
    k.sort()
    return k


def keyed_ranges(bounds, words):
    """the same for words that lie in consecutive ranges: key g owns words[bounds[g]:bounds[g + 1]]"""
    bounds = np.asarray(bounds, dtype=np.int64)
    key = np.repeat(np.arange(len(bounds) - 1, dtype=np.int64), np.diff(bounds))
    return keyed(key, words[:len(key)])


def sort_model(problems, geom):
    """The whole sort from the problems' entries (problem_entries): what the hook returns, in a canonical order.
      by_bucket        every entry as (global bucket p nb + bucket) << 32 | reference word, sorted
      off              nprob nb + 1 offsets;  bins: nprob sbins + 1 scanned bin bases
      by_bin           every entry as (global scan bin p sbins + bin) << 32 | packed word, sorted
      n_entries, largest (bucket size), sizes, error"""
    nb, sbins, P = geom["nb"], geom["sbins"], len(problems)
    bucket = np.concatenate([p * nb + pr["bucket"] for p, pr in enumerate(problems)])
    assert bucket.size == 0 or (bucket.min() >= 0 and bucket.max() < P * nb)
    sizes = np.bincount(bucket, minlength=P * nb)
    out = dict(n_entries=int(bucket.size), largest=int(sizes.max()) if sizes.size else 0, error=0, sizes=sizes)
    for pr in problems:
        out["error"] |= pr["error"]
    out["off"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out["by_bucket"] = keyed(bucket, np.concatenate([pr["ref"] for pr in problems]))
    del bucket
    if geom["two_level"]:
        sbin = np.concatenate([p * sbins + pr["sbin"] for p, pr in enumerate(problems)])
        assert sbin.size == 0 or (sbin.min() >= 0 and sbin.max() < P * sbins)
        out["bins"] = np.concatenate([[0], np.cumsum(np.bincount(sbin, minlength=P * sbins))]).astype(np.int64)
        out["by_bin"] = keyed(sbin, np.concatenate([pr["packed"] for pr in problems]))
    return out


def expected_max_bucket(largest, two_level):
    """The meta word max_bucket (include/msmz_test.h): the largest bucket size when some bucket has two entries; when
    none has, the two-level sort leaves 0 and the fallback 1 (0 without any entry)."""
    if largest >= 2:
        return largest
    return 0 if two_level else largest


def first_difference(got, want):
    """None when two keyed arrays agree; else (key, got word or None, want word or None) at the first disagreement: the
    smallest key whose multisets differ"""
    m = min(len(got), len(want))
    bad = np.nonzero(got[:m] != want[:m])[0]
    if bad.size == 0 and len(got) == len(want):
        return None
    i = int(bad[0]) if bad.size else m
    g = int(got[i]) if i < len(got) else None
    w = int(want[i]) if i < len(want) else None
    key = min(v >> 32 for v in (g, w) if v is not None)
    return key, (None if g is None else (g >> 32, g & 0xffffffff)), (None if w is None else (w >> 32, w & 0xffffffff))

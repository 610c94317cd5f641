"""oracle/sort_ref.py against oracle/bigint_ref.py and a brute-force dictionary built with Python integers (no GPU): the
model the GPU module tests/test_sort_gpu.py measures the bucket sort with."""
import random
import zlib

import numpy as np
import pytest

from oracle import bigint_ref as B
from oracle import params as P
from oracle import sort_ref as S

Q = P.CURVES["bls12-377"]["order"]
LAM = P.CURVES["bls12-377"]["endomorphism"]["lambda_"]


def clog2(x):
    return max(1, (x - 1).bit_length())


def make_geom(c, K, M, spread=0, fold=(0, 0), F=1, fb=None, fbt=None, endo_delta=0):
    """geometry words written out by hand from the definitions in csrc/plan.h (SortGeom, Plan, SortLayout)"""
    L = 1 << (c - 1)
    fb = min(c - 1, 3) if fb is None else fb
    fbt = fb if fbt is None else fbt
    ncb, ncbt = L >> fb, L >> fbt
    Keff = K - 1 + (1 << spread) if F == 1 else -(-K // F)
    nbins = (K - 1) * ncb + (ncbt << spread)
    mbits = clog2(max(M, 2))
    return dict(c=c, K=K, Keff=Keff, L=L, nb=Keff * L, fb=fb, fbt=fbt, ncb=ncb, ncbt=ncbt, nbins=nbins,
                sbins=Keff * F * ncb if F > 1 else nbins, fbins=Keff * ncb if F > 1 else nbins, fine_top=0, spread=spread,
                fold_shift=fold[0], fold_rows=fold[1], F=F, mbits=mbits, idx_bits=mbits + clog2(F) * (F > 1), cspec=0,
                two_level=1, tiles=1, sbits=256, endo_delta=endo_delta)


def corner_scalars(c, K, bits, rng, count):
    L = 1 << (c - 1)
    top = (1 << bits) - 1
    out = [0, 1, 2, top, top - 1, L, L + 1, L - 1, (1 << c) - 1, 1 << c]
    for k in (0, K // 2, K - 1):           # a digit exactly L (no carry) and L + 1 (carry) in the first, a middle, the top window
        out += [(L << (c * k)) & top, ((L + 1) << (c * k)) & top]
    out += [rng.getrandbits(bits) for _ in range(count - len(out))]
    return out


@pytest.mark.parametrize("c", range(2, 25))
def test_digits_equal_bigint_signed_digits(c):
    rng = random.Random(c)
    for bits, W in ((253, 8), (127, 4), (256, 8), (64, 8)):
        K = -(-(bits + 1) // c)
        vals = corner_scalars(c, K, bits, rng, 80)
        l, cy, over = S.signed_digits(S.to_words(vals, W), c, K)
        assert not over.any()
        for i, v in enumerate(vals):
            want = B.signed_digits(v, c, K)
            assert [(int(a), int(b)) for a, b in zip(l[i], cy[i])] == want, (c, bits, i)
            assert sum((-a if b else a) << (c * k) for k, (a, b) in enumerate(want)) == v
        # one window short: exactly the values whose K - 1 digits do not reproduce them are flagged
        if K > 1:
            l1, cy1, over1 = S.signed_digits(S.to_words(vals, W), c, K - 1)
            for i, v in enumerate(vals):
                fits = sum((-a if b else a) << (c * k) for k, (a, b) in enumerate(B.signed_digits(v, c, K - 1))) == v
                assert bool(over1[i]) == (not fits), (c, bits, i, v)


def test_flagged_scalars():
    vals = [0, 1, Q - 1, Q, Q + 1, (1 << 256) - 1, (1 << 64) - 1, 1 << 64, (1 << 128) - 1, 1 << 128]
    w = S.to_words(vals, 8)
    assert S.flagged(w, Q, 0).tolist() == [v >= Q for v in vals]
    assert S.flagged(w, Q, 256).tolist() == [v >= Q for v in vals]
    assert S.flagged(w, Q, 64).tolist() == [v >= Q or v >= 1 << 64 for v in vals]
    assert S.flagged(w, Q, 128).tolist() == [v >= Q or v >= 1 << 128 for v in vals]


def brute(halves_int, bad, g, n, copy_stride):
    """the documented rule, entry by entry with Python integers: {bucket: [ref]}, {scan bin: [packed]}, error"""
    c, K, L, F = g["c"], g["K"], g["L"], g["F"]
    buckets, bins, err = {}, {}, 4 if any(bad) else 0
    for h, half in enumerate(halves_int):
        for i, sv in enumerate(half):
            if bad[i]:
                continue
            mag, sg = abs(sv), 1 if sv < 0 else 0
            dig = B.signed_digits(mag, c, K)
            if sum((-l if ng else l) << (c * k) for k, (l, ng) in enumerate(dig)) != mag:
                err |= 2
            e = h * n + i
            for k, (l, ng) in enumerate(dig):
                if l == 0:
                    continue
                neg = ng ^ sg
                kw, bi, fbits, top = k // F, l - 1, g["fb"], k == K - 1 and F == 1
                if top and g["fold_shift"]:
                    if l > 1 << g["fold_shift"]:
                        err |= 2
                        continue
                    bi = (e % (1 << g["fold_rows"])) * (1 << g["fold_shift"]) + l - 1
                sub = e % (1 << g["spread"]) if top else 0
                if top:
                    fbits = g["fbt"]
                idx = e + (g["endo_delta"] if h else 0) + (k % F) * copy_stride
                buckets.setdefault((kw + sub) * L + bi, []).append(idx | neg << 31)
                coarse, fine = bi >> fbits, bi % (1 << fbits)
                if F > 1:
                    sb = ((k // F) * g["ncb"] + coarse) * F + k % F
                else:
                    sb = k * g["ncb"] + (sub * g["ncbt"] if top else 0) + coarse
                bins.setdefault(sb, []).append(((fine << 1 | neg) << g["idx_bits"]) | (k % F) << g["mbits"] | e)
    return buckets, bins, err


def run_case(g, scalars, n, glv, sbits=0, copy_stride=0):
    bad = S.flagged(S.to_words(scalars, 8), Q, sbits)
    if glv:
        dec = [B.glv_decompose(s % Q, Q, LAM) for s in scalars]
        halves_int = [[d[0] for d in dec], [d[1] for d in dec]]
        halves = [(S.to_words([abs(v) for v in hv], 4), np.array([v < 0 for v in hv], dtype=np.uint8)) for hv in halves_int]
    else:
        halves_int = [list(scalars)]
        halves = [(S.to_words(scalars, 8), np.zeros(n, dtype=np.uint8))]
    pr = S.problem_entries(halves, bad, g, n, copy_stride)
    want_b, want_s, want_err = brute(halves_int, bad.tolist(), g, n, copy_stride)
    model = S.sort_model([pr], g)
    assert pr["error"] == want_err == model["error"]
    got_b = {}
    for v in model["by_bucket"].tolist():
        got_b.setdefault(v >> 32, []).append(v & 0xffffffff)
    assert got_b == {b: sorted(v) for b, v in want_b.items()}
    got_s = {}
    for v in model["by_bin"].tolist():
        got_s.setdefault(v >> 32, []).append(v & 0xffffffff)
    assert got_s == {b: sorted(v) for b, v in want_s.items()}
    assert model["n_entries"] == sum(len(v) for v in want_b.values())
    assert model["largest"] == max((len(v) for v in want_b.values()), default=0)
    assert model["off"][0] == 0 and model["off"][-1] == model["n_entries"] and len(model["off"]) == g["nb"] + 1
    for b in range(g["nb"]):
        assert model["off"][b + 1] - model["off"][b] == len(want_b.get(b, []))
    assert len(model["bins"]) == g["sbins"] + 1
    for b in range(g["sbins"]):
        assert model["bins"][b + 1] - model["bins"][b] == len(want_s.get(b, []))
    # summing (+-) 2^(c k) l over a scalar's entries reproduces the (half-)scalar, where nothing was flagged or dropped
    if want_err == 0:
        c, L, fs = g["c"], g["L"], g["fold_shift"]
        total = [0] * (len(halves_int) * n)
        for b, r, k, e in zip(pr["bucket"].tolist(), pr["ref"].tolist(), pr["window"].tolist(), pr["entry"].tolist()):
            l = b % L + 1
            if fs and k == g["K"] - 1:
                l = (b % L) % (1 << fs) + 1
            total[e] += (-l if r >> 31 else l) << (c * k)
        assert total == [v for hv in halves_int for v in hv]
    return pr, model


def scalars_for(c, K, bits, n, seed):
    rng = random.Random(seed)
    vals = corner_scalars(c, K, bits, rng, n)
    return [v if v < Q else v % Q for v in vals]


REGIMES = {
    # name: (c, bits the windows are sized for, glv, geometry extras, copy_stride, sbits)
    "plain": (5, 253, 0, dict(), 0, 0),
    "plain_fbt": (6, 253, 0, dict(fb=3, fbt=1), 0, 0),
    "spread": (12, 253, 0, dict(spread=2, fb=4, fbt=2), 0, 0),
    "fold": (14, 253, 0, dict(fold=(6, 7), fb=5), 0, 0),
    "F2": (7, 253, 0, dict(F=2), 1000, 0),
    "F3": (7, 253, 0, dict(F=3), 777, 0),
    "FK": (9, 253, 0, dict(F=29), 513, 0),
    "glv_delta": (6, 127, 1, dict(endo_delta=300), 0, 0),
    "glv_F2_delta": (8, 127, 1, dict(F=2, endo_delta=44), 5000, 0),
    "glv_fold": (9, 127, 1, dict(fold=(4, 4)), 0, 0),
    "bound64": (7, 64, 0, dict(), 0, 64),
    "bound128_spread": (16, 128, 0, dict(spread=3, fb=8, fbt=8), 0, 128),
}


@pytest.mark.parametrize("name", sorted(REGIMES))
@pytest.mark.parametrize("n", [1, 37, 512])
def test_buckets_equal_brute_force(name, n):
    c, bits, glv, extra, stride, sbits = REGIMES[name]
    K = -(-(bits + 1) // c)
    if name == "FK":
        extra = dict(extra, F=K)
    g = make_geom(c, K, 2 * n if glv else n, **extra)
    sbound = min(bits, 253) if not glv else 253
    scalars = scalars_for(c, K, sbound, n, zlib.crc32(f"{name}{n}".encode()) & 0xffff)[:n]
    if sbits:   # a bound: 2^bits - 1 sorts, 2^bits and a scalar >= q are flagged and leave no entry
        extras = [(1 << sbits) - 1, 1 << sbits, Q + 5]
        for j, v in enumerate(extras[:n]):
            scalars[(j * 7) % n] = v
    pr, model = run_case(g, scalars, n, glv, sbits, stride)
    if sbits and n >= 3:
        assert model["error"] & 4


def test_fold_overflow_drops_the_top_digit_only():
    # c = 9, K = 15 windows sized for 127 bits, folded by 4: a top digit above 16 is dropped and flagged, nothing else
    c, K, n = 9, 15, 4
    g = make_geom(c, K, n, fold=(4, 4))
    base = [3 << (c * (K - 1)), 16 << (c * (K - 1)), 5, (17 << (c * (K - 1))) | 9]
    pr, model = run_case(g, base, n, 0)
    assert model["error"] == 2 and model["n_entries"] == 4
    assert sorted(pr["entry"].tolist()) == [0, 1, 2, 3] and sorted(pr["window"].tolist()) == [0, 0, K - 1, K - 1]


def test_two_problems_share_one_scan():
    c, K, n = 5, 4, 16
    g = make_geom(c, K, n)
    rng = random.Random(2)
    probs = []
    for p in range(2):
        vals = [rng.getrandbits(c * K - 1) for _ in range(n)]
        probs.append(S.problem_entries([(S.to_words(vals, 8), np.zeros(n, dtype=np.uint8))], np.zeros(n, dtype=bool), g, n))
    m = S.sort_model(probs, g)
    assert m["off"][g["nb"]] == probs[0]["bucket"].size and m["bins"][g["sbins"]] == probs[0]["bucket"].size
    assert m["off"][-1] == m["n_entries"] == probs[0]["bucket"].size + probs[1]["bucket"].size
    first = probs[0]["bucket"].size
    assert ((m["by_bucket"][:first] >> np.uint64(32)) < g["nb"]).all() and ((m["by_bucket"][first:] >> np.uint64(32)) >= g["nb"]).all()
    # the device's arrays, keyed by the ranges of off / bins, compare equal to the model's
    refs = (m["by_bucket"] & np.uint64(0xffffffff)).astype(np.uint32)
    assert S.first_difference(S.keyed_ranges(m["off"], refs), m["by_bucket"]) is None


def test_max_bucket_rule_and_first_difference():
    assert [S.expected_max_bucket(v, 1) for v in (0, 1, 2, 9)] == [0, 0, 2, 9]
    assert [S.expected_max_bucket(v, 0) for v in (0, 1, 2, 9)] == [0, 1, 2, 9]
    a = S.keyed([0, 0, 3], [6, 5, 1])
    assert a.tolist() == [5, 6, (3 << 32) | 1]
    assert S.first_difference(a, a.copy()) is None
    assert S.first_difference(a, S.keyed([0, 0, 3], [5, 7, 1])) == (0, (0, 6), (0, 7))
    assert S.first_difference(a, a[:2]) == (3, (3, 1), None)
    assert S.keyed_ranges([0, 2, 2, 3], np.array([6, 5, 1])).tolist() == [5, 6, (2 << 32) | 1]

"""oracle/schedule_ref.py against brute force and hand-written descriptor lists (no GPU): the model the GPU module
tests/test_plan_schedule_gpu.py measures k_plan_count / k_plan_emit with."""
import numpy as np
import pytest

from oracle import schedule_ref as SR

O, N = SR.LOC_ORIG, SR.LOC_NONE


def brute_rounds(sizes):
    """the reference's in-place walk (msm-batched-affine.ts:232-247), carrying the set of positions every element holds"""
    held = [[{p} for p in range(s)] for s in sizes]
    rounds, m = [], 1
    while m < max(sizes, default=0):
        adds = []
        for g, s in enumerate(sizes):
            j = 0
            while j * 2 * m + m < s:
                a, b = j * 2 * m, j * 2 * m + m
                held[g][a] |= held[g][b]
                held[g][b] = None
                adds.append((g, a, b))
                j += 1
        rounds.append(adds)
        m *= 2
    return rounds, held


SIZE_LISTS = [[], [0], [1], [2], [3], [4], [5, 0, 1, 2], [0, 0, 7, 8, 9, 1], [63, 64, 65], [127, 128, 129, 0, 1],
              [300, 2, 0, 33], list(range(0, 40))]


@pytest.mark.parametrize("sizes", SIZE_LISTS, ids=[str(i) for i in range(len(SIZE_LISTS))])
def test_reference_rounds_is_the_in_place_walk(sizes):
    want, held = brute_rounds(sizes)
    got = SR.reference_rounds(sizes)
    assert len(got) == len(want)
    for r, (g, a, b) in enumerate(got):
        assert list(zip(g.tolist(), a.tolist(), b.tolist())) == want[r], r
        assert np.array_equal(SR.pairs_in_round(sizes, r), np.bincount(g, minlength=len(sizes))), r
    # after all rounds element 0 of every bucket holds the whole bucket
    for s, h in zip(sizes, held):
        assert s == 0 or h[0] == set(range(s))
        assert all(x is None for x in h[1:])


def test_reference_rounds_random_against_brute_force():
    rng = np.random.default_rng(5)
    pool = list(range(10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 100]
    for _ in range(60):
        sizes = [int(x) for x in rng.choice(pool, size=int(rng.integers(1, 12)))]
        want, _ = brute_rounds(sizes)
        got = SR.reference_rounds(sizes)
        assert [list(zip(*(x.tolist() for x in rd))) for rd in got] == want, sizes


@pytest.mark.parametrize("mx,want", [(0, (0, 0, 0)), (1, (0, 0, 0)), (2, (1, 1, 1)), (3, (2, 1, 1)), (4, (2, 1, 1)),
                                     (5, (3, 2, 1)), (64, (6, 5, 4)), (65, (7, 6, 5)), (1 << 24, (24, 23, 22))])
def test_plan_rounds(mx, want):
    assert tuple(SR.plan_rounds(mx, t) for t in (0, 1, 2)) == want
    assert SR.plan_rounds(mx, 0) == len(SR.reference_rounds([mx]))


# ---- expand on hand-written lists: buckets of 3, 0, 1, 2 entries; entry e carries index 10 + e and negate bit e & 1
SIZES = [3, 0, 1, 2]
OFF = np.array([0, 3, 3, 4, 6], dtype=np.uint32)
REFS = np.array([(10 + e) | ((e & 1) << 31) for e in range(6)], dtype=np.uint32)


def orig(e):
    return O | int(REFS[e])


def meta(rounds, pairs):
    rp = list(pairs) + [0] * (32 - len(pairs))
    rb = np.concatenate([[0], np.cumsum(rp)])[:32]
    return dict(max_bucket=3, n_entries=6, error=0, rounds=rounds, round_pairs=np.array(rp), round_base=rb)


GOOD_DESC = [[orig(0), orig(1)], [orig(4), orig(5)],      # round 0: records 0 (bucket 0), 1 (bucket 3)
             [0, orig(2)]]                                # round 1: record 2 = record 0 + entry 2
GOOD_BFIN = [[2, N, N, N], [N, N, N, N], [orig(3), N, N, N], [1, N, N, N]]


def run(desc=GOOD_DESC, bfin=GOOD_BFIN, rounds=2, pairs=(2, 1)):
    return SR.expand(np.array(desc, dtype=np.uint32).reshape(-1, 2), np.array(bfin, dtype=np.uint32), meta(rounds, pairs),
                     OFF, REFS)


def test_expand_good_list():
    ex = run()
    assert ex.rec_bucket.tolist() == [0, 3, 0]
    assert list(zip(ex.rec_lo.tolist(), ex.rec_mid.tolist(), ex.rec_hi.tolist())) == [(0, 1, 2), (0, 1, 2), (0, 2, 3)]
    assert ex.fin_count.tolist() == [1, 0, 1, 1]
    assert list(zip(ex.fin_bucket.tolist(), ex.fin_lo.tolist(), ex.fin_hi.tolist())) == [(0, 0, 3), (2, 0, 1), (3, 0, 2)]


def test_expand_one_round_leaves_two_locations():
    """tail_skip: after round 0 alone bucket 0 is left as record 0 + its last entry"""
    ex = run(desc=GOOD_DESC[:2], bfin=[[0, orig(2), N, N], GOOD_BFIN[1], GOOD_BFIN[2], GOOD_BFIN[3]], rounds=1, pairs=(2,))
    assert ex.fin_count.tolist() == [2, 0, 1, 1]
    assert list(zip(ex.fin_lo.tolist(), ex.fin_hi.tolist())) == [(0, 2), (2, 3), (0, 1), (0, 2)]


def bad(match, **kw):
    with pytest.raises(SR.ScheduleError, match=match) as e:
        run(**kw)
    return e.value


def test_expand_rejects_record_used_twice():
    e = bad("consumed twice", bfin=[[0, orig(2), N, N]] + GOOD_BFIN[1:])   # record 0: by round 1 and by bfin
    assert (e.round, e.pair, e.bucket, e.record) == (0, 0, 0, 0)


def test_expand_rejects_record_never_used():
    e = bad("never consumed", bfin=GOOD_BFIN[:3] + [[orig(4), orig(5), N, N]])   # record 1 dropped
    assert (e.round, e.pair, e.bucket, e.record) == (0, 1, 3, 1)


def test_expand_rejects_forward_reference():
    e = bad("not written before this launch", desc=[[2, orig(1)]] + GOOD_DESC[1:])   # round 0 reads a round-1 record
    assert (e.round, e.pair, e.record) == (0, 0, 2)
    e = bad("not written before this launch", desc=GOOD_DESC[:2] + [[2, orig(2)]])   # a pair reads its own record
    assert (e.round, e.pair) == (1, 0)


def test_expand_rejects_wrong_negate_bit_and_unknown_index():
    e = bad("negate bit", desc=[[orig(0), orig(1) ^ 0x80000000]] + GOOD_DESC[1:])
    assert (e.round, e.pair) == (0, 0) and "operand B" in str(e) and "position 1" in str(e)
    bad("no entry has it", desc=[[O | 9, orig(1)]] + GOOD_DESC[1:])
    bad("no entry has it", desc=[[O | 99, orig(1)]] + GOOD_DESC[1:])


def test_expand_rejects_operands_out_of_place():
    e = bad("not adjacent", desc=[[orig(1), orig(0)]] + GOOD_DESC[1:])            # swapped
    assert (e.round, e.pair, e.bucket) == (0, 0, 0)
    bad("not adjacent", desc=[[orig(0), orig(2)]] + GOOD_DESC[1:])                # a position skipped
    e = bad("buckets 0 and 2", desc=GOOD_DESC[:2] + [[0, orig(3)]])                # across buckets
    assert (e.round, e.pair) == (1, 0)


def test_expand_rejects_bad_bfin():
    bad("after LOC_NONE", bfin=[[N, 2, N, N]] + GOOD_BFIN[1:])
    bad("stands for bucket 3", bfin=[[1, N, N, N], GOOD_BFIN[1], GOOD_BFIN[2], [2, N, N, N]])
    bad("0 final locations for 1 entries", bfin=GOOD_BFIN[:2] + [[N, N, N, N]] + GOOD_BFIN[3:])
    bad("starts at position 2", desc=GOOD_DESC[:2], bfin=[[orig(2), 0, N, N]] + GOOD_BFIN[1:], rounds=1, pairs=(2,))
    bad("ends at position 2 of 3", desc=GOOD_DESC[:2], bfin=[[0, N, N, N]] + GOOD_BFIN[1:], rounds=1, pairs=(2,))
    bad("no round wrote|belongs to no round", rounds=1, pairs=(2,))                # record 2 outside every round
    bad("not written|no entry", bfin=[[0xA5A5A5A5, N, N, N]] + GOOD_BFIN[1:])      # the hook's fill pattern


def test_expand_needs_distinct_indices():
    with pytest.raises(ValueError):
        SR.expand(np.zeros((0, 2), np.uint32), np.full((1, 4), N, np.uint32), meta(0, ()), [0, 2],
                  np.array([5, 5], dtype=np.uint32))


def test_expand_random_lists_built_from_the_rule():
    """descriptor lists written straight from reference_rounds (records numbered in reference order) replay cleanly"""
    rng = np.random.default_rng(11)
    for trial in range(40):
        sizes = rng.choice([0, 1, 2, 3, 4, 5, 8, 9, 17, 40], size=int(rng.integers(1, 9)))
        tail_skip = trial % 3
        off = np.concatenate([[0], np.cumsum(sizes)])
        n = int(off[-1])
        refs = (rng.permutation(n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31))
        R = SR.plan_rounds(int(sizes.max()), tail_skip)
        holder = [{p: SR.LOC_ORIG | int(refs[off[g] + p]) for p in range(s)} for g, s in enumerate(sizes)]
        desc, pairs = [], []
        for r in range(R):
            g, a, b = SR.reference_round(sizes, r)
            pairs.append(len(g))
            for gg, aa, bb in zip(g.tolist(), a.tolist(), b.tolist()):
                desc.append([holder[gg][aa], holder[gg].pop(bb)])
                holder[gg][aa] = len(desc) - 1
        bfin = [[h[p] for p in sorted(h)] + [N] * (4 - len(h)) for h in holder]
        m = meta(R, pairs)
        ex = SR.expand(np.array(desc, dtype=np.uint32).reshape(-1, 2), np.array(bfin, dtype=np.uint32), m, off, refs)
        assert ex.fin_count.tolist() == [-(-int(s) // (1 << R)) for s in sizes]
        if len(desc) > 1:   # and a list with two records swapped in one operand does not
            d2 = np.array(desc, dtype=np.uint32)
            recs = np.argwhere((d2 & SR.LOC_ORIG) == 0)
            if len(recs) >= 1:
                i, k = recs[0]
                d2[i, k] = (int(d2[i, k]) + 1) % len(desc)
                with pytest.raises(SR.ScheduleError):
                    SR.expand(d2, np.array(bfin, dtype=np.uint32), m, off, refs)

"""The case list of the MSM sweep (tests/msm_sweep_util.py) and its predicted regimes (tests/native/sweep_regimes.cpp,
csrc/plan.h on a CPU): (a) the list covers every pair of values and every listed triple the rule table allows, (b) every
planner regime appears in some predicted plan, (c) nothing is dropped without a rule that says why and the list does
not shrink, (d) the closed form the GPU sweep expects equals the oracle's MSM on explicit points and scalars."""
import random

import numpy as np
import pytest

import msm_sweep_util as U
from oracle import c_oracle
from oracle import params as P

SEED = 1
N_CASES = 1374   # cases(1): 1359 of the covering and 15 directed ones


@pytest.fixture(scope="module")
def case_list():
    return U.cases(SEED)


@pytest.fixture(scope="module")
def predicted(case_list):
    return U.regimes(case_list, U.SET_POINTS)


def test_cases_are_a_pure_function_of_the_seed(case_list):
    assert U.cases(SEED) == case_list
    assert U.cases(SEED + 1) != case_list
    assert [c["id"] for c in case_list] == list(range(len(case_list)))


def test_only_supported_combinations(case_list, predicted):
    """no case breaks a rule, and the planner accepts every case (status 0: also the precomputed set's parameters)"""
    for c in case_list:
        assert not U.violated({k: c[k] for k in U.NAMES if not (k == "size" and c["directed"])}), c
        assert predicted[c["id"]]["status"] == 0, (c, predicted[c["id"]])
        assert 1 <= c["n"] <= (1 << 18) + (1 << 17)
        if c["shape"] in ("batch2", "batch5", "segments"):
            assert c["n"] <= U.MAX_BATCH_N, c
        if c["size"] not in ("1..64", "directed"):
            assert c["n"] == U.size_min(c["size"])
    sizes = {c["n"] for c in case_list}
    assert {2047, 2048, 2049, 65535, 65536, 65537} <= sizes and any(n <= 64 for n in sizes)
    assert {(1 << k) + d for k in range(10, 19) for d in (-1, 0, 1)} | {3 << (k - 1) for k in range(10, 19)} <= sizes


def test_a_pair_and_triple_coverage(case_list):
    """(a) every target the rules allow is held by a case of the covering (the directed cases are not counted)"""
    held = set()
    for c in case_list:
        if not c["directed"]:
            held.update(U._holds(c))
    allowed = [t for t, why in U.targets().items() if why is None]
    missing = [t for t in allowed if t not in held]
    assert not missing, missing[:10]
    # the dimensions are the issue's: 4 curves, 3 entry points, 6 shapes, 3 GLV choices, 7 window sizes, 6 bounds, ...
    assert [len(v) for v in U.DIMS.values()] == [4, 3, 6, 3, 7, 6, 2, 2, 4, 2, 2, 3, 37]
    assert len(allowed) > 4000


def test_c_no_silent_shrinkage(case_list):
    """(c) every target no case can hold is forbidden by a rule that reads only the target's own dimensions and cites
    the line it restates; the list is as long as when it was made"""
    names = {name for name, _, _, _ in U.RULES}
    for name, fields, cite, _ in U.RULES:
        assert cite and set(fields) <= set(U.DIMS), name
    dropped = {t: why for t, why in U.targets().items() if why is not None}
    assert dropped and all(why in names for why in dropped.values()), [t for t, w in dropped.items() if w not in names][:10]
    # a rule that forbids nothing would hide a typo
    assert {"te-entry", "te-glv", "projective-glv", "pre-te", "pre-projective", "pre-reduce-affine", "segments-multi",
            "batch-size", "pooled-entry", "passes-pre", "sub-shape"} <= set(dropped.values())
    assert len(case_list) == N_CASES, len(case_list)


def test_b_every_regime_appears(case_list, predicted):
    """(b) the planner regimes, each in at least one predicted plan"""
    R = [dict(predicted[c["id"]], case=c) for c in case_list]
    auto = [r for r in R if r["case"]["glv"] == -1 and r["case"]["curve"] != U.TE]
    seen = {
        "fold": any(r["fold_shift"] > 0 for r in R),
        "spread 1": any(r["spread"] == 1 for r in R),
        "spread 2": any(r["spread"] == 2 for r in R),
        "spread 3": any(r["spread"] == 3 for r in R),
        "fbt < fb": any(0 <= r["fbt"] < r["fb"] for r in R),
        "cspec 16": any(r["cspec"] == 16 for r in R),
        "cspec 17": any(r["cspec"] == 17 for r in R),
        "generic sort": any(r["cspec"] == 0 and r["two_level"] for r in R),
        "fallback sort": any(not r["two_level"] for r in R),
        "fallback sort under a batch": any(not r["two_level"] and r["per_problem"] and r["case"]["shape"] == "batch2" for r in R),
        "default GLV on": any(r["glv"] == 1 for r in auto),
        "default GLV off": any(r["glv"] == 0 for r in auto),
        "default GLV off by a bound": any(r["glv"] == 0 and r["case"]["n"] < 1 << 15 for r in auto),
        "cost-model window": any(r["rule"] == "model" for r in R),
        "fixed window 17": any(r["rule"] == "fixed" and r["c"] == 17 for r in R),
        "fixed window 16": any(r["rule"] == "fixed" and r["c"] == 16 and r["glv"] for r in R),
        "stepped-down window": any(r["rule"] == "stepped" for r in R),
        "bounded, keeps 17": any(r["rule"] == "bounded17" and r["c"] == 17 for r in R),
        "F > 1, c = 17 branch": any(r["F"] > 1 and r["rule"] == "pre17" and r["c"] == 17 for r in R),
        "F > 1, model": any(r["F"] > 1 and r["rule"] == "pre_model" for r in R),
        "F = 2": any(r["F"] == 2 and r["Keff"] > 1 for r in R),
        "chunk below PLAN_CHUNK": any(r["chunk"] < 1024 for r in R),
        "chunk = PLAN_CHUNK": any(r["chunk"] == 1024 for r in R),
        "top split on": any(r["top_split"] for r in R),
        "top split off": any(not r["top_split"] for r in R),
        "batched pipeline": any(r["bs"] > 1 for r in R),
        "sub-batches": any(r["case"]["limits"] == "subbatches" and 1 < r["bs"] < 5 and r["cap"] > 0 for r in R),
        "batch problem by problem": any(r["per_problem"] for r in R),
        "index-range passes": any(r["passes"] >= 2 for r in R),
        "GLV redo": any("redo_K" in r and r["redo_K"] > r["K"] for r in R),
    }
    assert all(seen.values()), [k for k, v in seen.items() if not v]
    # every case of limits = subbatches was given a cap that cuts it, every case of limits = passes two passes
    for r in R:
        if r["case"]["limits"] == "subbatches":
            assert 1 < r["bs"] < 5 and r["cap"] > 0, r
        if r["case"]["limits"] == "passes" and r["case"]["shape"] == "single" and r["case"]["engines"] == 1:
            assert r["passes"] >= 2, r


def _explicit(label, mult):
    """the points [m] G of signed multipliers, through the oracle's scalar multiplication"""
    c = P.CURVES[label]
    g = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    return [c_oracle.scale(c, m % c["order"], g) for m in mult]


@pytest.mark.parametrize("label", U.DIMS["curve"])
def test_d_closed_form_equals_the_oracle(label):
    """(d) on small explicit inputs of every scalar distribution, bound and both point distributions the closed form
    [sum s_i sign_i a_i mod q] G is the oracle's MSM"""
    c_oracle.build()
    c = P.CURVES[label]
    q = c["order"]
    g = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    rng = random.Random("closed form" + label)
    n_set = 48
    for pdist in U.DIMS["pdist"]:
        a, sign = U.multipliers(pdist, n_set)
        points = _explicit(label, [int(s) * int(v) for s, v in zip(sign, a)])
        if pdist == "pooled":
            assert (sign == 0).any() and (sign < 0).any()
            for i in np.nonzero(sign == 0)[0]:   # [0] G is the neutral element
                assert points[i]["isZero"] or (points[i]["x"], points[i]["y"]) == (0, 1)
        for sdist in U.DIMS["sdist"]:
            for bits in U.DIMS["scalarBits"]:
                words = U.scalar_words(label, sdist, bits, n_set)
                s = [int.from_bytes(w.astype("<u8").tobytes(), "little") for w in words]
                assert all(0 <= v < U.bound_of(q, bits) for v in s), (sdist, bits)
                first, n = rng.randrange(8), rng.randint(1, 40)
                want = c_oracle.msm(c, s[first:first + n], points[first:first + n])
                t = U.expected_scalar(q, words[first:first + n], a[first:first + n], sign[first:first + n])
                got = c_oracle.scale(c, t, g)
                assert (got["x"], got["y"], bool(got.get("isZero"))) == (want["x"], want["y"], bool(want.get("isZero"))), \
                    (pdist, sdist, bits, first, n)
    # the distributions are what they say
    big = U.scalar_words(label, "sparse", 64, 4000)
    zero = (big == 0).all(axis=1).mean()
    assert 0.85 < zero < 0.95
    eq = U.scalar_words(label, "equal", 0, 100)
    assert (eq == eq[0]).all() and eq[0].any()
    edges = {int.from_bytes(w.astype("<u8").tobytes(), "little") for w in U.scalar_words(label, "edges", 0, 2000)}
    assert {0, 1, q - 1} <= edges
    edges = {int.from_bytes(w.astype("<u8").tobytes(), "little") for w in U.scalar_words(label, "edges", 64, 2000)}
    assert {0, 1, (1 << 64) - 1, (1 << 16) - 1} <= edges


def test_segments_and_shares(case_list):
    """three segments: two in one length class, one in another, both offsets non-zero, inside the shared sets; the share
    of a two-engine context is the block deal of csrc/multi.h"""
    for c in case_list:
        assert U.points_needed(c) <= U.SET_POINTS and U.scalars_needed(c) <= U.SET_SCALARS, c
        if c["shape"] != "segments":
            continue
        segs = U.segments_of(c)
        cls = sorted(n.bit_length() for _, _, n in segs)
        assert len(segs) == 3 and len(set(cls)) == 2, (c, segs)
        assert all(p > 0 and s > 0 and n >= 1 for p, s, n in segs), segs
    assert U.share(65536, 2) == (0, 65536) and U.share(65537, 2) == (1, 1) and U.share(3 << 17, 2) == (1, 3 << 16)
    assert U.share(1000, 1) == (0, 1000)

"""The GLV split at its rounding thresholds and longest halves, without a GPU: the integer model of the device formula
(oracle/glv_edges.py) against the host build of csrc/scalar.h glv_decompose -- bit for bit, magnitudes and signs, not
only the congruence -- and the facts the windows of a GLV MSM rest on: no scalar below the group order has a half of
2^127 or more (the exact supremum follows from the lattice constants), and scalars exist whose halves come within 1 %
of that supremum.  tests/test_glv_edges_gpu.py puts the same scalars through the four device copies of the routine."""
import math
from fractions import Fraction

import pytest

from oracle import glv_edges as E
from test_fp_host import driver  # noqa: F401  (the fixture that builds and runs tests/native/fp_host_test.cpp)

FIELD = {"bls12-377": "bls377", "pallas": "pallas", "bls12-381": "bls381"}

_edges = {}


def edges(label):
    if label not in _edges:
        _edges[label] = (E.edge_scalars(label), E.edge_set(label))
    return _edges[label]


@pytest.mark.parametrize("label", E.LABELS)
def test_threshold_pairs_sit_on_thresholds(label):
    """|x_j| is k at thr - 1 and k + 1 at thr; both scalars of every pair are in the edge set; the ripple thresholds
    carry across a word"""
    named, every = edges(label)
    cases = E.threshold_cases(label)
    assert len(cases) >= 50
    for j, k, thr in cases:
        assert E.x_magnitudes(label, thr - 1)[j] == k, (j, k)
        assert E.x_magnitudes(label, thr)[j] == k + 1, (j, k)
        assert thr - 1 in every and thr in every
    assert len(named["ripple"]) >= 24
    words = set()
    for s in named["ripple"]:
        words |= {w for x in E.x_magnitudes(label, s) for w in (32, 64, 96) if x and x % (1 << w) == 0}
    assert words == {32, 64, 96}


@pytest.mark.parametrize("label", E.LABELS)
def test_host_equals_model(driver, label):  # noqa: F811
    """the host build of glv_decompose == the integer model on every edge scalar: both 16-byte magnitudes, both signs"""
    _, every = edges(label)
    got = driver([f"{FIELD[label]} glv 1 {s:x}" for s in every])
    for s, g in zip(every, got):
        n0, m0, n1, m1 = g.split(":")
        s0, s1 = E.model(label, s)
        # (a zero half has no sign: the routine leaves it positive)
        assert (int(m0, 16), int(n0), int(m1, 16), int(n1)) == (abs(s0), int(s0 < 0), abs(s1), int(s1 < 0)), hex(s)


@pytest.mark.parametrize("label", E.LABELS)
def test_small_scalars_decompose_back(label):
    """a + b lambda with |a|, |b| at the word boundaries up to 2^120 splits into exactly (a, b): the halves +-2^32,
    +-2^64, +-2^96 at which the sign conversion borrows across words are really in the set"""
    rows = E.small_pairs(label)
    assert len(rows) == 289
    for a, b, s in rows:
        assert E.model(label, s) == (a, b), (a, b)


@pytest.mark.parametrize("label", E.LABELS)
def test_supremum_facts(label):
    """sup |s_j| < 2^127 for every scalar below q; no edge scalar exceeds it; GLV_PROVEN_BITS covers it"""
    sup = E.supremum(label)
    print(f"{label}: sup |s0| = {float(sup[0] / (1 << 127)):.4f} * 2^127, sup |s1| = {float(sup[1] / (1 << 127)):.4f} * 2^127")
    assert sup[0] < 1 << 127 and sup[1] < 1 << 127
    _, every = edges(label)
    for s in every:
        s0, s1 = E.model(label, s)
        assert abs(s0) <= int(sup[0]) + 1 and abs(s1) <= int(sup[1]) + 1, hex(s)
        assert (s0 + s1 * E.constants(label)["lam"] - s) % E.constants(label)["q"] == 0
    assert E.constants(label)["proven_bits"] >= max(math.ceil(x) for x in sup).bit_length()


@pytest.mark.parametrize("label", E.LABELS)
def test_longest_halves_are_long(label):
    """each of the 64 `longest` scalars has a half at or above 99 % of its supremum"""
    named, _ = edges(label)
    assert len(named["longest"]) == 64
    ratios = [E.longest_ratio(label, s) for s in named["longest"]]
    print(f"{label}: smallest longest ratio {float(min(ratios)):.6f}, largest {float(max(ratios)):.6f}, edge set {len(edges(label)[1])}")
    assert min(ratios) >= Fraction(99, 100)
    if label == "bls12-377":   # the first step of the 126-step chain of k_points_mul_glv
        assert any(abs(h) >> 125 for s in named["longest"] for h in E.model(label, s))

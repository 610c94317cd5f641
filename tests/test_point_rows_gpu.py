"""The row form of the point addition (add_rows of the group policies: one addition per wave, a field element per DPP
row) on raw accumulator records, against oracle/bigint_ref.py: P + Q, P + P and P + (-P) with a different lambda on
each side, the neutral element on either side and on both, the doubling (of the neutral element too), and a chain of
eight operations feeding each other in registers."""
import os
import random
import sys

import pytest

from oracle import params as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fp_contract import Field, _points, te_affine, te_ext, te_neg, xyzz  # noqa: E402
from test_lazy_contract_gpu import CURVES, _chain_ref, _point_raw, ctxs  # noqa: E402,F401

pytestmark = pytest.mark.gpu

TPR_ADD_ROWS, TPR_DBL_ROWS, TPR_CHAIN_ROWS = 8, 9, 10
CHAIN_L = 8


@pytest.mark.parametrize("label", CURVES)
def test_point_rows(ctxs, label):
    curve = ctxs(label)
    f = Field(label)
    rng = random.Random(53 + CURVES.index(label))
    c, pts = _points(label, rng, 6)
    if P.CURVES[label]["kind"] == "twisted-edwards":
        ident = (0, 1)
        acc = lambda q: te_ext(f, q, rng)
        add = lambda u, v: te_affine(c, u, v)
        neg_pt = lambda q: te_neg(c, q)
        dbl = lambda u: add(u, u)
        norm = lambda r: r
    else:
        ident = c.zero
        acc = lambda q: xyzz(f, q, rng)
        add, neg_pt, dbl = c.add, c.negate, c.double
        norm = lambda r: c.zero if r == (0, 0) else (r[0], r[1], False)
    # every acc() call rescales with a fresh lambda: equal points meet in different representations
    A, Bq, want = [], [], []
    for i, a in enumerate(pts):
        b = pts[(i + 1) % len(pts)]
        for q in (b, a, neg_pt(a), ident):
            A += [acc(a), acc(q)]; Bq += [acc(q), acc(a)]; want += [add(a, q), add(q, a)]
    A.append(acc(ident)); Bq.append(acc(ident)); want.append(ident)
    assert [norm(r) for r in _point_raw(curve, TPR_ADD_ROWS, A, Bq)] == want
    D = [acc(q) for q in pts] + [acc(ident)]
    assert [norm(r) for r in _point_raw(curve, TPR_DBL_ROWS, D, D)] == [dbl(q) for q in pts] + [ident]
    # r <- r + b, r <- 2r alternately, eight operations, never stored in between
    CA = [acc(pts[i]) for i in range(4)] + [acc(ident), acc(pts[0])]
    CB = [acc(pts[i + 1]) for i in range(4)] + [acc(pts[1]), acc(neg_pt(pts[0]))]
    ends = list(zip(pts[:4], pts[1:5])) + [(ident, pts[1]), (pts[0], neg_pt(pts[0]))]
    cwant = [_chain_ref(add, dbl, a, b, CHAIN_L) for a, b in ends]
    assert [norm(r) for r in _point_raw(curve, TPR_CHAIN_ROWS, CA, CB, L=CHAIN_L)] == cwant

"""The lazy-limb contract on the device: msmz_test_field_limbs loads caller-chosen RAW register limbs unchanged, so the
field routines of the kernels run on the edge cases of oracle/lazy_limbs.py -- mul / sqr operands at +-(bound p - 1)
with limbs at the product limit, fe_reduce_small / fe_store at k p - 1, k p, k p + 1 for k in [-16, 15] in three limb
forms, fe_is_zero at k p (|k| <= 15) and its near misses, fe_store_mulout across (-1.5p, 0.5p), carries, inversions
and the slot-record round trips.  Each result is checked against Python integers, and every op the host contract
driver also runs (tests/native/fp_contract_test.cpp, the same code from csrc/test_ops.h) must agree with it bit for
bit."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import bigint_ref as B
from oracle import lazy_limbs as LZ
from oracle import params as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fp_contract import Field, _points, build_driver, field_limb_lines, niels, te_affine, te_ext, te_neg, xyzz  # noqa: E402,E501

pytestmark = pytest.mark.gpu

CURVES = ["bls12-377", "pallas", "bls12-381", "ed-on-bls12-377"]


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


def _device(curve, label, ops, a, b):
    """run op[i] on (a[i], b[i]) -- one launch per distinct op"""
    from msm_zprize_amd import _native
    _, n, _ = LZ.FIELDS[label]
    fb = curve.fe_bytes
    raw_all, canon_all = [None] * len(ops), [None] * len(ops)
    for op in sorted(set(ops)):
        idx = [i for i, o in enumerate(ops) if o == op]
        A = np.ascontiguousarray(np.array([a[i] for i in idx], dtype=np.int64).astype(np.int32))
        Bv = np.ascontiguousarray(np.array([b[i] for i in idx], dtype=np.int64).astype(np.int32))
        raw = np.zeros((len(idx), n), dtype=np.int32)
        canon = C.create_string_buffer(fb * len(idx))
        st = _native.lib().msmz_test_field_limbs(curve._ctx, op, A.ctypes.data, Bv.ctypes.data, len(idx),
                                                 raw.ctypes.data, canon)
        assert st == 0, st
        for k, i in enumerate(idx):
            raw_all[i] = [int(x) for x in raw[k]]
            canon_all[i] = int.from_bytes(canon.raw[fb * k:fb * (k + 1)], "little")
    return raw_all, canon_all


@pytest.mark.parametrize("label", CURVES)
def test_field_limbs_edges_match_host(ctxs, label):
    curve = ctxs(label)
    lines, cases = field_limb_lines(label)
    _, n, _ = LZ.FIELDS[label]
    zero = [0] * n
    extra = []
    # device-only ops: the wave-wide inversion on the inversion inputs, the slot records on mul outputs / lazy pairs
    extra += [(LZ.TFL_INVERSE_WAVE, a, b) for op, a, b in cases if op == LZ.TFL_INVERSE]
    extra += [(LZ.TFL_SLOT_MULOUT, limbs, zero) for _, limbs in LZ.mulout_cases(label)]
    red = [limbs for _, limbs in LZ.reduce_cases(label)]
    extra += [(LZ.TFL_SLOT_POINT, red[i], red[(i * 5 + 1) % len(red)]) for i in range(0, len(red), 3)]
    allc = cases + extra
    raw, canon = _device(curve, label, [c[0] for c in allc], [c[1] for c in allc], [c[2] for c in allc])
    for (op, a, b), r, cv in zip(allc, raw, canon):
        try:
            LZ.check_field_limb_result(label, op, a, b, r, cv)
        except AssertionError as e:
            raise AssertionError(f"op {op} a={a} b={b} -> raw {r} canon {cv:x}") from e
    # bit for bit against the host build of the same code
    exe = build_driver(0)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    host = out.stdout.split("\n")[:len(lines)]
    for l, h, r, cv in zip(lines, host, raw, canon):
        hraw, hcanon = h.split()
        assert [int(x) for x in hraw.split(",")] == r and int(hcanon, 16) == cv, l
    inv = {tuple(a): cv for (op, a, _), cv in zip(allc, canon) if op == LZ.TFL_INVERSE}
    for (op, a, _), cv in zip(allc, canon):
        if op == LZ.TFL_INVERSE_WAVE:
            assert cv == inv[tuple(a)]


# ------------------------------------------------------------------------------------------------ points, kernel form
(TPR_ADD, TPR_ADD_X4, TPR_MADD, TPR_DBL, TPR_DBL_X4, TPR_MDBL, TPR_CHAIN, TPR_CHAIN_X4) = range(8)
TP_MADD = 2
CHAIN_L = 300


def _point_raw(curve, op, a_recs, b_recs, neg=None, L=0):
    """a_recs / b_recs: lists of 4 hex coordinates (memory words); returns canonical affine results"""
    from msm_zprize_amd import _native
    fb = curve.fe_bytes
    n = len(a_recs)
    pack = lambda recs: b"".join(int(h, 16).to_bytes(fb, "little") for r in recs for h in r)
    out = C.create_string_buffer(2 * fb * n)
    nb = bytes(neg) if neg is not None else None
    st = _native.lib().msmz_test_point_raw(curve._ctx, op, pack(a_recs), pack(b_recs), nb, n, L, out)
    assert st == 0, st
    res = []
    for i in range(n):
        x = int.from_bytes(out.raw[2 * fb * i:2 * fb * i + fb], "little")
        y = int.from_bytes(out.raw[2 * fb * i + fb:2 * fb * (i + 1)], "little")
        res.append((x, y))
    return res


def _chain_ref(add, dbl, a, b, L):
    r = a
    for k in range(L):
        r = dbl(r) if k & 1 else add(r, b)
    return r


@pytest.mark.parametrize("label", CURVES)
def test_point_raw_kernel_form(ctxs, label):
    """the point formulas of the kernels -- scalar and 4-lane add / dbl, mixed add with the negated record, mdbl,
    register chains -- on lazy memory-format operands in [0, 3p) with rescaled (general-Z) accumulators: P + Q, P + P
    and P + (-P) with a different lambda on each side, infinity / the identity on either side"""
    curve = ctxs(label)
    f = Field(label)
    rng = random.Random(31 + CURVES.index(label))
    c, pts = _points(label, rng, 6)
    te = P.CURVES[label]["kind"] == "twisted-edwards"
    zero_rec = ["0"] * 4
    if te:
        ident = (0, 1)
        acc = lambda q: te_ext(f, q, rng)
        add = lambda u, v: te_affine(c, u, v)
        neg_pt = lambda q: te_neg(c, q)
        dbl = lambda u: add(u, u)
        rec = lambda q: niels(f, c, q, rng) + ["0"]
        norm = lambda r: r
    else:
        ident = c.zero
        acc = lambda q: xyzz(f, q, rng)
        add, neg_pt, dbl = c.add, c.negate, c.double
        rec = lambda q: (zero_rec if q[2] else [f.mem(q[0], rng), f.mem(q[1], rng), "0", "0"])
        norm = lambda r: c.zero if r == (0, 0) else (r[0], r[1], False)
    A, Bq, want = [], [], []
    for i, a in enumerate(pts):
        b = pts[(i + 1) % len(pts)]
        for q in (b, a, neg_pt(a), ident):
            A += [acc(a), acc(q)]; Bq += [acc(q), acc(a)]; want += [add(a, q), add(q, a)]
    A.append(acc(ident)); Bq.append(acc(ident)); want.append(ident)
    for op in (TPR_ADD, TPR_ADD_X4):
        got = [norm(r) for r in _point_raw(curve, op, A, Bq)]
        assert got == want, op
    D = [acc(q) for q in pts] + [acc(ident)]
    dwant = [dbl(q) for q in pts] + [ident]
    for op in (TPR_DBL, TPR_DBL_X4):
        assert [norm(r) for r in _point_raw(curve, op, D, D)] == dwant, op
    # mixed addition: the record holds q, or -q with neg = 1
    MA, MB, MN, mwant = [], [], [], []
    for i, a in enumerate(pts):
        b = pts[(i + 1) % len(pts)]
        for q in (b, a, neg_pt(a)):
            for ng in (0, 1):
                MA.append(acc(a)); MB.append(rec(neg_pt(q) if ng else q)); MN.append(ng); mwant.append(add(a, q))
        MA.append(acc(ident)); MB.append(rec(b)); MN.append(0); mwant.append(b)
        if not te:
            MA.append(acc(a)); MB.append(rec(ident)); MN.append(1); mwant.append(a)
    assert [norm(r) for r in _point_raw(curve, TPR_MADD, MA, MB, MN)] == mwant
    if not te:
        recs = [rec(q) for q in pts for _ in (0, 1)]
        negs = [k & 1 for k in range(len(recs))]
        recs = [rec(neg_pt(pts[k // 2])) if negs[k] else recs[k] for k in range(len(recs))]
        assert [norm(r) for r in _point_raw(curve, TPR_MDBL, [zero_rec] * len(recs), recs, negs)] == \
            [dbl(pts[k // 2]) for k in range(len(recs))]
    # register chains: r <- r + b, r <- 2r alternately, never stored
    CA = [acc(pts[i]) for i in range(4)]
    CB = [acc(pts[i + 1]) for i in range(4)]
    cwant = [_chain_ref(add, dbl, pts[i], pts[i + 1], CHAIN_L) for i in range(4)]
    for op in (TPR_CHAIN, TPR_CHAIN_X4):
        assert [norm(r) for r in _point_raw(curve, op, CA, CB, L=CHAIN_L)] == cwant, op


@pytest.mark.parametrize("label", CURVES)
def test_point_madd_hook(ctxs, label):
    """msmz_test_point MADD: the second operand is stored as an input record and folded in by the policy's mixed
    addition (it used to fall through to the full addition)"""
    from msm_zprize_amd import _native
    curve = ctxs(label)
    fb = curve.fe_bytes
    rng = random.Random(41)
    c = _curve_ref(label)
    te = isinstance(c, B.TwistedEdwards)
    pts = [c.scale(rng.randrange(1, c.q), c.one) for _ in range(6)]
    pts = [c.to_affine(q) if te else q for q in pts]
    pairs = []
    for i, a in enumerate(pts):
        b = pts[(i + 1) % len(pts)]
        pairs += [(a, b), (a, a)] + ([(a, c.negate(a)), (a, c.zero), (c.zero, a)] if not te else [(a, (0, 1))])
    enc = lambda q: (q[0].to_bytes(fb, "little") + q[1].to_bytes(fb, "little")) if te or not q[2] else bytes(2 * fb)
    inf = lambda q: bytes([0 if te or not q[2] else 1])
    a_xy = b"".join(enc(p) for p, _ in pairs)
    b_xy = b"".join(enc(q) for _, q in pairs)
    ai = None if te else b"".join(inf(p) for p, _ in pairs)
    bi = None if te else b"".join(inf(q) for _, q in pairs)
    out = C.create_string_buffer(2 * fb * len(pairs))
    assert _native.lib().msmz_test_point(curve._ctx, TP_MADD, a_xy, ai, b_xy, bi, len(pairs), out) == 0
    for k, (p, q) in enumerate(pairs):
        x = int.from_bytes(out.raw[2 * fb * k:2 * fb * k + fb], "little")
        y = int.from_bytes(out.raw[2 * fb * k + fb:2 * fb * (k + 1)], "little")
        if te:
            assert (x, y) == c.to_affine(c.add(c.from_affine(p), c.from_affine(q))), k
        else:
            assert (c.zero if (x, y) == (0, 0) else (x, y, False)) == c.add(p, q), k


def _curve_ref(label):
    params = P.CURVES[label]
    return B.TwistedEdwards(params) if params["kind"] == "twisted-edwards" else B.AffineWeierstrass(params)

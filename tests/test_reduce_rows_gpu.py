"""The row-form levels of the bucket reduction (k_reduce_rows: one wave per addition, a field element per DPP row)
through msmz_test_reduce, with rows_max forcing them on (2^20: every level down to one entry) and off (1: levels of a
single group only, so that k_reduce_quad16 and k_reduce_tail do the work), crossed with the tail thresholds 1 / 4 / 32 /
4096.  Inputs,
oracle and failure messages are those of tests/test_reduce_gpu.py; every result is bit-exact against
oracle/bigint_ref.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import bigint_ref as BR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_reduce_gpu as TR  # noqa: E402

pytestmark = pytest.mark.gpu

ctxs = TR.ctxs
ROWS = [1 << 20, 1]
TAILS = [1, 4, 32, 4096]
N_INS = [1, 2, 3, 4, 5, 7, 16, 17, 31, 33, 64, 100, 256, 4096]
KINDS = ["generic", "all_neutral", "all_equal", "alternating"]


def call(curve, rows_max, **kw):
    """TR.call with the appended rows_max field"""
    from msm_zprize_amd import _native
    a = _native.MsmzTestReduceArgs()
    keep = []

    def buf(x):
        if x is None:
            return None
        b = x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()
        keep.append(b)
        return b

    fb = kw["fb"]
    for name in ("mode", "c", "nsets", "n_in", "nc", "tail_n", "quad16_max", "pairsum_x4_max", "n_points", "n_slots"):
        setattr(a, name, int(kw.get(name, 0)))
    a.rows_max = rows_max
    for name in ("points_xy", "scale"):
        setattr(a, name, buf(kw.get(name)))
    cscan = kw.get("cscan")
    if cscan is not None:
        cscan = np.ascontiguousarray(cscan, dtype=np.uint32)
        a.cscan = cscan.ctypes.data
    n_res, n_lines = kw["n_res"], kw.get("n_lines", 0)
    out = np.full((n_res, 2 * fb), 0xEE, dtype=np.uint8)
    lines = np.full((max(n_lines, 1), 2 * fb), 0xEE, dtype=np.uint8)
    a.out_xy = out.ctypes.data
    a.lines_xy = lines.ctypes.data if n_lines else None
    st = TR._lib().msmz_test_reduce(curve._ctx, C.byref(a))
    return st, out, lines[:n_lines]


def level_inputs(n_in, nprob, kind):
    if kind == "generic":
        rng = np.random.default_rng(n_in * 64 + nprob)
        rows = rng.integers(-1000, 1001, size=(nprob, n_in))
        cs = rng.integers(-1000, 1001, size=(nprob, n_in))
        rows[:, n_in // 2] = 0
        return rows, cs
    return TR.degenerate_levels(n_in, nprob, kind)


def run_levels(ctxs, label, rows, cs, rows_max, tail, what, lam):
    pl = TR.pool(label)
    rows, cs = np.asarray(rows, dtype=np.int64), np.asarray(cs, dtype=np.int64)
    nprob, n_in = rows.shape
    vals = np.concatenate([rows.reshape(-1), cs.reshape(-1)])
    kw = dict(points_xy=pl.take(vals), n_points=len(vals))
    if lam:
        kw["scale"] = TR.scales(pl, len(vals), lam)
    st, out, _ = call(ctxs(label), rows_max, fb=pl.fb, mode=TR.LEVELS, nsets=nprob, n_in=n_in, tail_n=tail, n_res=nprob, **kw)
    tag = f"{label} levels n_in={n_in} nprob={nprob} tail_n={tail} rows_max={rows_max} [{what}; lambda={lam}]"
    assert st == 0, f"{tag}: status {st}"
    e = np.arange(n_in, dtype=object)
    want = [int((cs[j].astype(object) + e * rows[j].astype(object)).sum()) % pl.q for j in range(nprob)]
    bad = np.nonzero((pl.enc_many(want) != out).any(axis=1))[0]
    if len(bad):
        j = int(bad[0])
        pytest.fail(f"{tag}: problem {j}: expected {want[j]} G; problems {bad.tolist()} differ")


@pytest.mark.parametrize("nprob", [1, 3, 64])
@pytest.mark.parametrize("label", TR.ALL)
def test_levels_rows(ctxs, label, nprob):
    """short last groups, a single group, groups that do not fill the tail's workgroup, a tail that does every level
    or only copies C; generic entries, all neutral, all equal (every step a doubling), alternating P / -P, with the
    entries of a problem in one representation and each in its own (lambda)"""
    for n_in in N_INS:
        for kind in KINDS:
            rows, cs = level_inputs(n_in, nprob, kind)
            for rows_max in ROWS:
                for tail in TAILS:
                    if n_in == 4096 and kind != "generic" and (rows_max, tail) != (ROWS[0], 32):
                        continue   # the largest shape: degenerate entries on the row kernels with the default tail only
                    run_levels(ctxs, label, rows, cs, rows_max, tail, kind, lam=n_in if tail == 4 else 0)


def run_2d(ctxs, label, c, nsets, m, rows_max, tail, what, lam):
    """TR.run_2d in the accumulator mode with rows_max: every line sum, then every weighted sum"""
    pl = TR.pool(label)
    L, H, D = TR.split(c)
    m = np.asarray(m, dtype=np.int64).reshape(nsets, L).copy()
    cnt = TR.counts(nsets * L, L, "one")
    kw = TR.encode_accs(pl, m.reshape(-1), cnt, lam)
    st, out, lines = call(ctxs(label), rows_max, fb=pl.fb, mode=TR.ACCS, c=c, nsets=nsets, tail_n=tail, n_res=2 * nsets,
                          n_lines=2 * nsets * H, **kw)
    tag = f"{label} accs c={c} (L={L} H={H} D={D}) sets={nsets} tail_n={tail} rows_max={rows_max} [{what}; lambda={lam}]"
    assert st == 0, f"{tag}: status {st}"
    want_lines, want_res = [], []
    for s in range(nsets):
        rows, cols, rr, cr = BR.reduce_multiples_2d([int(v) for v in m[s]], c, pl.q)
        want_lines += rows + cols
        want_res += [rr, cr]
    bad = np.nonzero((pl.enc_many(want_lines) != lines).any(axis=1))[0]
    if len(bad):
        prob, line = divmod(int(bad[0]), H)
        pytest.fail(f"{tag}: LINE SUM wrong in problem {prob}, line {line}; {len(bad)} of {len(lines)} differ")
    bad = np.nonzero((pl.enc_many(want_res) != out).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        pytest.fail(f"{tag}: WEIGHTED SUM wrong (all line sums right) in problem {i}: expected {want_res[i]} G; "
                    f"problems {bad.tolist()} differ")


@pytest.mark.parametrize("c", [2, 3, 5, 8, 9, 16])
@pytest.mark.parametrize("label", TR.ALL)
def test_2d_rows(ctxs, label, c):
    """H = 2, odd and even splits of the window, the largest window: line sums and weighted sums checked separately"""
    nsets = 1 if c == 16 else 3
    for kind, lam in (("random", 0), ("same", 5), ("alternating_lines", 0)):
        if c == 16 and kind != "random":
            continue
        m = TR.contents(c, nsets, kind, 3)
        for rows_max in ROWS:
            for tail in TAILS:
                run_2d(ctxs, label, c, nsets, m, rows_max, tail, kind, lam)

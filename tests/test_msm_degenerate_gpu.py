"""Safe MSMs whose tree rounds are large enough for B = 2 .. 16 pairs per thread AND full of degenerate pairs.

Half of the 3 * 2^17 inputs come from a pool of three points, their negatives and the point at infinity, with four
distinct scalars: every window's buckets then hold many copies of the same point (DBL pairs), a point and its negative
(sums at infinity) and infinity operands (TAKE pairs), in rounds of 2^18 .. 2^21 pairs and more.  The other half are distinct
random points with random scalars.  Points are a_i G with known a_i (randomPointsFast), so the expected MSM is
(sum_i s_i m_i mod q) G with m_i = a_i, q - a_i for a negated point and 0 for infinity (test_msm_gpu_large.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle
from oracle import params as P
from oracle import prng

pytestmark = pytest.mark.gpu

N = 3 << 17   # without GLV > 2^22 entries: a first round of > 2^21 pairs (B = 16), then B = 8, 4, 2
HALF = N // 2
PSEED, SSEED = 71, 72
# one round of each size: 2^21 (B = 16), 2^20 (B = 8), 2^19 (B = 4), 2^18 (B = 2) pairs at the least
MIN_PAIRS = (1 << 21) + (1 << 20) + (1 << 19) + (1 << 18)


@pytest.fixture(scope="module")
def mod():
    import msm_zprize_amd as m
    m.startThreads()
    return m


def _strip(p):
    return {"x": p["x"], "y": p["y"], "isZero": bool(p.get("isZero", False))}


def _point(c, t):
    gen = {"x": c["generator"]["x"], "y": c["generator"]["y"], "isZero": False}
    r = c_oracle.scale(c, t, gen)
    return {"x": r["x"], "y": r["y"], "isZero": bool(r.get("isZero", False))}


class Inputs:
    """pooled half: entry i < HALF is value (i // 3) % 7 of the pool -- base 0, 1, 2, their negatives, infinity -- with
    scalar (i // 5) % 4 of four fixed ones; distinct half: the random points and scalars of the seeds"""

    def __init__(self, curve, label):
        from msm_zprize_amd._native import check, lib
        c = P.CURVES[label]
        self.c, q, p, fb = c, c["order"], c["modulus"], c["fe_bytes"]
        rand = curve.Parallel.randomPointsFast(N, PSEED)
        raw = C.create_string_buffer(2 * fb * N)
        inf = C.create_string_buffer(N)
        check(lib().msmz_download_points(curve._ctx, rand.handle, 0, N, raw, inf), "msmz_download_points")
        rand.free()
        rows = np.frombuffer(raw.raw, dtype=np.uint8).reshape(N, 2 * fb).copy()
        a = prng.multipliers_np(PSEED, N)
        base = [int(v) for v in a[:3]]
        pool_rows = [rows[k].copy() for k in range(3)]
        for k in range(3):
            y = int.from_bytes(pool_rows[k][fb:].tobytes(), "little")
            neg = pool_rows[k].copy()
            neg[fb:] = np.frombuffer(((p - y) % p).to_bytes(fb, "little"), dtype=np.uint8)
            pool_rows.append(neg)
        pool_rows.append(np.zeros(2 * fb, dtype=np.uint8))
        pool_mult = base + [q - m for m in base] + [0]
        i = np.arange(HALF)
        self.val = (i // 3) % 7
        self.sidx = (i // 5) % 4
        rows[:HALF] = np.stack(pool_rows)[self.val]
        is_inf = np.zeros(N, dtype=np.uint8)
        is_inf[:HALF] = self.val == 6
        self.pts = curve.Parallel.pointsFromBytes(rows.tobytes(), N, is_inf.tobytes())
        self.pool_mult = pool_mult
        self.a = a
        self.q = q

    def scalars(self, seed, fixed):
        """scalar words (N, 4) and the expected MSM: fixed[j] on the pooled half, scalars_np(seed) on the other"""
        s = prng.scalars_np(seed, N, self.q)
        for j, v in enumerate(fixed):
            s[:HALF][self.sidx == j] = [(v >> (64 * w)) & (2 ** 64 - 1) for w in range(4)]
        counts = np.zeros((len(fixed), 7), dtype=np.int64)
        np.add.at(counts, (self.sidx, self.val), 1)
        t = sum(int(counts[j, v]) * fixed[j] * self.pool_mult[v] for j in range(len(fixed)) for v in range(7))
        t += prng.sum_of_products_mod(s[HALF:], self.a[HALF:], self.q)
        return s.astype("<u8").tobytes(), _point(self.c, t % self.q)


_inputs = {}


def inputs(mod, label):
    if label not in _inputs:
        curve = mod.Weierstrass.create(mod.curves.BY_LABEL[label])
        _inputs[label] = (curve, Inputs(curve, label))
    return _inputs[label]


def fixed_scalars(q, k):
    return [(0x1234567 + 0x9E3779B97F4A7C15 * (j + 1) * (k + 3)) ** 3 % q for j in range(4)]


@pytest.mark.parametrize("label", ["bls12-377", "pallas", "bls12-381"])
def test_safe_msm_with_degenerate_buckets_at_large_batch(mod, label):
    curve, inp = inputs(mod, label)
    sc, want = inp.scalars(SSEED, fixed_scalars(inp.q, 0))
    for glv in (0, 1):
        out = curve.Parallel.msm(sc, inp.pts, N, False, {"glv": glv})
        assert _strip(out["result"]) == want, f"glv={glv}"
        st = out["stats"]
        print(f"{label} glv={glv}: c={st.c} K={st.K} rounds={st.rounds} n_entries={st.n_entries} n_pairs={st.n_pairs}")
        # rounds large enough for every B > 1 (a later planner change must not shrink them below B = 2)
        assert st.n_entries >= (1 << 22) + (1 << 20)
        assert st.n_pairs >= MIN_PAIRS


@pytest.mark.parametrize("label", ["bls12-377", "pallas", "bls12-381"])
def test_safe_batch_and_precomputed_with_degenerate_buckets(mod, label):
    curve, inp = inputs(mod, label)
    try:
        s0, w0 = inp.scalars(SSEED, fixed_scalars(inp.q, 0))
        s1, w1 = inp.scalars(SSEED + 1, fixed_scalars(inp.q, 1))
        got = curve.Parallel.msmBatch([s0, s1], inp.pts, N)
        assert [_strip(r) for r in got] == [w0, w1]
        log = curve.Parallel.lastBatchLog
        print(f"{label} batch: c={log.c} K={log.K} n_entries={log.n_entries} n_pairs={log.n_pairs}")
        assert log.n_pairs >= 2 * MIN_PAIRS
        pre = curve.Parallel.precomputePoints(inp.pts, N, {}, 0)
        out = curve.Parallel.msm(s0, pre, N)
        st = out["stats"]
        print(f"{label} precomputed: c={st.c} K={st.K} n_entries={st.n_entries} n_pairs={st.n_pairs}")
        assert _strip(out["result"]) == w0
        assert st.n_pairs >= MIN_PAIRS
        pre.free()
    finally:
        inp.pts.free()
        curve.close()
        _inputs.pop(label, None)

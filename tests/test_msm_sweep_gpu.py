"""The MSM option space on the GPU against the closed form (tests/msm_sweep_util.py makes the cases).

Every case of cases(SEED) runs once: curve x entry point x shape (one MSM, batch, segments, precomputed set) x GLV x
window size x scalar bit bound x reduceAffine x scalar source x scalar and point distribution x engines x lowered limits
x size class, a covering of all pairs and of three triples under the rule table of the util module.  Points are m_i G
with known m_i, so the expected result of a problem is [sum s_i m_i mod q] G (c_oracle.scale); the comparison is
bit-exact on x, y and the infinity flag.  Every case also asserts that the call reports the window size, window count
and GLV choice tests/native/sweep_regimes.cpp predicted for it from csrc/plan.h alone, so a case runs the plan it was
chosen for, and a failure names the case, the predicted regime and what the call reported.  The last test asserts that
the engine-side regimes (index-range passes, sub-batches, a batch run problem by problem, msmBasic with and without
k_bucket_sums, a grown msmBasic chunk, the GLV redo) were seen.

Checked against seven one-line mutations, each on a scratch copy of csrc/ built as a variant library and run through
MSMZ_LIB, none committed.  All change value arithmetic only -- a sign bit, a Horner weight on the host, which of the
copies or images inside a set a reference names -- never an index, offset, count, loop bound or barrier.  The sweep
failed under every one; the first failing case and its predicted regime:
  1. host64.h window_terms: the rows of a FOLDED top window get their weight (`if (!fold || k < K - 1)` -> `if (true)`)
     -> bls12-377 msmUnsafe, n = 98304 on two engines in passes, c = 16, glv = 1, scalarBits = 16: fold_shift = 7, K = 2
  2. host64.h window_terms: the weight of a precomputed bucket set (`c *= F` -> `c = c * F + 1`)
     -> bls12-377 pre2 (two windows per set), c = 20, scalarBits = 127, n = 16385: F = 2, Keff = 4
  3. host64.h window_terms: a SPREAD sub-window's weight in the one-dimensional reduction (`{c * k, kw}` ->
     `{c * k + (kw > k), kw}`) -> bls12-377 msmBatch(5) run problem by problem, reduceAffine = 1, c = 12, scalarBits = 127,
     pooled points: spread = 3
  4. plan.h make_plan: endo_delta of a GLV prefix of a longer point set (`pts_n - pl.n` -> 0: the second halves name base
     points of the set instead of images) -> bls12-377 msmSegments, glv = 1, c = 17, n = 8191 of the shared set
  5. sort_kernels.h k_coarse: the sign of a spread top-window digit (`ng ^= spread > 0` after bucket_index)
     -> the same segmented case: spread = 3, top_split
  6. sort_kernels.h DigitStream::load: the sign of the second GLV half (`n0 | (n1 << 1)` -> `n0 | (n0 << 1)`)
     -> the same segmented case: glv = 1
  7. sort_kernels.h k_coarse: the copy window k of a precomputed set references (`k % F` -> `(k + 1) % F`)
     -> the pre2 case of 2.
Not mutated: the carry into the top window under a scalar bound.  It changes a digit, and a digit is a bucket number:
the histogram and the scatter must agree on it and the planner sizes the top window's bins for it, so no variant of it is
value-only.  tests/test_scalar_bits_gpu.py and tests/test_sort_gpu.py cover that carry on the sort's own output.
"""
import pytest

import msm_sweep_util as U

pytestmark = pytest.mark.gpu

SEED = 1
BLOCK = 40   # cases per test function
SWEEP = U.Sweep(SEED)


def _blocks():
    out = []
    for label in U.DIMS["curve"]:
        ids = [c["id"] for c in SWEEP.cases if c["curve"] == label]
        out += [pytest.param(ids[k:k + BLOCK], id=f"{label}-{k // BLOCK}") for k in range(0, len(ids), BLOCK)]
    return out


@pytest.fixture(scope="module")
def sweep():
    import msm_zprize_amd as m
    m.startThreads()
    yield SWEEP
    SWEEP.close()


@pytest.mark.parametrize("ids", _blocks())
def test_sweep(sweep, ids):
    for i in ids:
        sweep.run(sweep.cases[i])


def test_engine_side_regimes_were_observed(sweep):
    """(after the whole module) the sweep saw: two index-range passes, two sub-batches, a batch run problem by problem,
    msmBasic with and without k_bucket_sums, a bucket above 1024 entries that grows the msmBasic chunk, the GLV redo"""
    seen = sweep.observed
    print(f"sweep: {seen['cases']} cases in {seen['seconds']:.1f} s; observed {seen}")
    assert seen["cases"] == len(sweep.cases), "run the whole module: the sweep's cases are its coverage"
    for key in ("range_passes", "sub_batches", "per_problem", "basic_summed", "basic_plain", "chunk_grown", "glv_redo"):
        assert seen[key] >= 1, (key, seen)

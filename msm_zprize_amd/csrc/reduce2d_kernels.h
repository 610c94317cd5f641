// Two-dimensional bucket reduction.  Included by kernels.h.
//
// The reference's running-sum reduction (msm-batched-affine.ts:544-571) walks a window's L buckets as ONE chain; the
// grouped form of round 1-2 (a first level over all L buckets + quad levels) still left a dependency chain of 2 point
// additions per bit of the bucket index: 13 bits above the first level = 0.55 ms of latency at 2^20, and a first level
// that holds two XYZZ accumulators (256 VGPRs).  Here the bucket weight j in [0, L) is split into a high and a low half,
//     j = h * D + d,   h in [0, H), d in [0, D),   H = 2^ceil((c-1)/2), D = L / H,
//     sum_j j E_j = D * sum_h h R_h + sum_d d C_d,     R_h = sum_d E[h D + d],   C_d = sum_h E[h D + d]:
// the 2 L plain (unweighted) sums R, C are embarrassingly parallel -- any grouping, one accumulator per thread, mixed
// additions only -- and what is left are two weighted sums over H (<= 512) entries per bucket set instead of one over
// L: the chain is half as deep.  The host's Horner pass adds the row result at bit position c k + log2 D and the column
// result at c k (host64.h window_terms) -- no extra doublings.  The bucket of weight L = H D is added twice
// into row H/2, as before.
//
//   k_reduce2d_partial   thread = (problem, line, chunk): folds D / NC buckets of a row (or H / NC buckets of a column)
//                        into one XYZZ partial sum; problems 2 kw (rows) and 2 kw + 1 (columns) of
//                        bucket set kw, H lines each (the column problem's lines >= D are infinity), NC chunks per line
//   k_pairsum(_x4)       out[i] = in[2 i] + in[2 i + 1]: log2 NC launches turn the chunks of a line into its sum; the
//                        small late levels with one DPP quad per addition (xyzz_add_x4)
//   then the existing upper levels (k_reduce_quad16 / k_reduce_tail) run on 2 Keff problems of H entries with
//   rows = line sums, C = infinity.
#pragma once
#include "plan.h"   // R2Geom

namespace msmz {

// What thread t of the partial-sum kernels does: chunk `chunk` of line `line` of problem `prob` (bucket set kw, rows or
// columns), i.e. the buckets of weights j0, j0 + step, ... (count of them); fold: and the single bucket of weight
// L = H D, folded in as 2 * (H/2) * D by the first chunk of row H/2.  A plain sum may group buckets any way, so
// the chunks of a ROW are interleaved (chunk q = buckets q, q + NC, q + 2 NC, ... of the row) and those of a COLUMN are
// dealt so that neighbouring lanes hold neighbouring columns: either way the lanes of a wave read neighbouring buckets
// in the same step (coalesced final-location words, neighbouring records).
struct R2Chunk {
  uint32_t prob, kw, line, chunk, j0, step, count;
  bool fold;
};
__device__ __forceinline__ R2Chunk r2_chunk(const R2Geom& g, uint32_t t) {
  R2Chunk c;
  const uint32_t per_prob = g.H * g.NC;
  c.prob = t / per_prob;
  const uint32_t u = t - c.prob * per_prob;
  c.kw = c.prob >> 1;
  const bool col = (c.prob & 1u) != 0;
  c.j0 = c.step = c.count = 0;
  if (!col) {
    c.line = u / g.NC;
    c.chunk = u - c.line * g.NC;
    c.j0 = c.line * g.D + c.chunk;
    c.step = g.NC;
    c.count = g.chr;
  } else if (u < g.D * g.NC) {
    c.chunk = u / g.D;
    c.line = u - c.chunk * g.D;
    c.j0 = c.chunk * g.chc * g.D + c.line;
    c.step = g.D;
    c.count = g.chc;
  } else {
    // lines D .. H-1 of the column problem do not exist: infinity, so that both problems have H entries
    const uint32_t v = u - g.D * g.NC;
    c.line = g.D + v / g.NC;
    c.chunk = v - (v / g.NC) * g.NC;
  }
  c.fold = !col && c.line == g.H / 2 && c.chunk == 0;
  return c;
}

// acc += accs[q0 .. q1), accumulator records in the policy's memory format
template <class P>
__device__ __forceinline__ void add_accs(typename P::Acc& acc, const uint32_t* accs, uint32_t q0, uint32_t q1) {
  typename P::Acc tmp, p;
  for (uint32_t q = q0; q < q1; q++) {
    P::load(p, accs + (size_t)q * P::ACC_WORDS);
    P::add(tmp, acc, p);
    acc = tmp;
  }
}

template <class F>
__global__ void __launch_bounds__(128, MSMZ_REDUCE_OCC) k_reduce2d_partial(uint32_t* part, const uint32_t* slots,
                                                                           const uint32_t* points, const uint4* bfin,
                                                                           R2Geom g, uint32_t total) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const R2Chunk c = r2_chunk(g, t);
  Xyzz<F> acc;
  xyzz_set_inf(acc);
  // (A software pipeline -- final-location word two buckets ahead, record one bucket ahead -- measured no faster than
  // this plain loop once the chunks were interleaved: the kernel is bound by the multiplier at 2 waves per SIMD, and the
  // other wave covers the two dependent loads of a bucket.)
#pragma unroll 1
  for (uint32_t i = 0; i < c.count; i++) {
    const uint32_t j = c.j0 + i * c.step;
    if (j >= 1) add_bucket<F>(acc, c.kw * g.L + (j - 1), slots, points, bfin);
  }
  if (c.fold) {
    for (int twice = 0; twice < 2; twice++) add_bucket<F>(acc, c.kw * g.L + (g.L - 1), slots, points, bfin);
  }
  WeierPolicy<F>::store(part + ((size_t)(c.prob * g.H + c.line) * g.NC + c.chunk) * 4 * F::NW, acc);
}

// The same partial sums for the msmBasic path (msm-basic.ts:106-128 buckets in XYZZ / extended coordinates): bucket g is
// the sum of the partial accumulators accs[cscan[g] .. cscan[g+1]) that k_bucket_accumulate left of it (cscan == nullptr:
// accs holds ONE accumulator per bucket, in bucket order -- the sums k_bucket_sums formed).
template <class P>
__global__ void __launch_bounds__(128, MSMZ_REDUCE_OCC) k_reduce2d_partial_acc(uint32_t* part, const uint32_t* accs,
                                                                               const uint32_t* cscan, R2Geom g,
                                                                               uint32_t total) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const R2Chunk c = r2_chunk(g, t);
  typename P::Acc acc;
  P::set_identity(acc);
  // [a, b) = the accumulators of the bucket of weight j of this set (none for weight 0)
  auto range = [&](uint32_t j, uint32_t& a, uint32_t& b) {
    a = b = 0;
    if (j >= 1) {
      const size_t gb = (size_t)c.kw * g.L + (j - 1);
      a = cscan ? cscan[gb] : (uint32_t)gb;
      b = cscan ? cscan[gb + 1] : (uint32_t)gb + 1u;
    }
  };
  // the chunk ranges of the next bucket are requested one step ahead
  uint32_t qa = 0, qb = 0;
  if (c.count) range(c.j0, qa, qb);
#pragma unroll 1
  for (uint32_t i = 0; i < c.count; i++) {
    uint32_t na = 0, nb = 0;
    if (i + 1 < c.count) range(c.j0 + (i + 1) * c.step, na, nb);
    add_accs<P>(acc, accs, qa, qb);
    qa = na;
    qb = nb;
  }
  if (c.fold) {
    range(g.L, qa, qb);
    for (int twice = 0; twice < 2; twice++) add_accs<P>(acc, accs, qa, qb);
  }
  P::store(part + ((size_t)(c.prob * g.H + c.line) * g.NC + c.chunk) * P::ACC_WORDS, acc);
}

// Buckets of several partial accumulators (large msmBasic inputs): one accumulator per bucket, in bucket order, so that
// the two visits of the two-dimensional reduction read each bucket ONCE each instead of all its chunks twice.
template <class P>
__global__ void __launch_bounds__(128, MSMZ_REDUCE_OCC) k_bucket_sums(uint32_t* out, const uint32_t* accs, const uint32_t* cscan,
                                                                      uint32_t nb) {
  constexpr int XW = P::ACC_WORDS;
  const uint32_t gb = blockIdx.x * blockDim.x + threadIdx.x;
  if (gb >= nb) return;
  typename P::Acc acc, tmp, p;
  P::set_identity(acc);
  const uint32_t q0 = cscan[gb], q1 = cscan[gb + 1];
  if (q1 > q0) {
    P::load(acc, accs + (size_t)q0 * XW);
    for (uint32_t q = q0 + 1; q < q1; q++) {
      P::load(p, accs + (size_t)q * XW);
      P::add(tmp, acc, p);
      acc = tmp;
    }
  }
  P::store(out + (size_t)gb * XW, acc);
}

// n neutral accumulators (the C inputs of the first weighted level).  Not a memset: the twisted-Edwards identity is
// (0, 1, 1, 0), only the XYZZ infinity is an all-zero record.
template <class P>
__global__ void __launch_bounds__(256) k_fill_neutral(uint32_t* out, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  typename P::Acc z;
  P::set_identity(z);
  P::store(out + (size_t)t * P::ACC_WORDS, z);
}

// out[i] = in[2 i] + in[2 i + 1], one thread per addition
template <class P>
__global__ void __launch_bounds__(128, MSMZ_REDUCE_OCC) k_pairsum(uint32_t* out, const uint32_t* in, uint32_t n_out) {
  constexpr int XW = P::ACC_WORDS;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_out) return;
  typename P::Acc a, b, r;
  P::load(a, in + (size_t)(2 * t) * XW);
  P::load(b, in + (size_t)(2 * t + 1) * XW);
  P::add(r, a, b);
  P::store(out + (size_t)t * XW, r);
}

// the same with one DPP quad per addition (4 dependent field products instead of 14: the small, latency-bound levels)
template <class P>
__global__ void __launch_bounds__(64, MSMZ_Q16_OCC) k_pairsum_x4(uint32_t* out, const uint32_t* in, uint32_t n_out) {
  constexpr int XW = P::ACC_WORDS;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = t >> 2;
  const int s = (int)(t & 3);
  const bool live = i < n_out;
  typename P::Acc a, b, r;
  P::set_identity(a);
  P::set_identity(b);
  if (live) {
    P::load(a, in + (size_t)(2 * i) * XW);
    P::load(b, in + (size_t)(2 * i + 1) * XW);
  }
  P::add_x4(r, a, b, s, false);
  if (live && s == 0) P::store(out + (size_t)i * XW, r);
}

}  // namespace msmz

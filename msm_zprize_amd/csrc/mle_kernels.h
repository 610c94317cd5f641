// Multilinear polynomials over resident scalar sets (msmz_scalars_eq_table / _mle_eval / _mle_bind / _sumcheck_round /
// _sumcheck_step, include/msmz.h; DESIGN.md sections 24 and 30).  A polynomial in v variables is a range of 2^v records, entry i =
// f(b_0, .., b_(v-1)) with i = sum b_j 2^j: variable 0 is the lowest index bit.
//     eq_table:        out_i = scale eq(r, i),   eq(r, i) = prod_j (b_j r_j + (1 - b_j)(1 - r_j))
//     mle_eval:        sum_i f_i eq(r, i)        (the table is generated, never stored)
//     mle_bind:        out_i = lo + r (hi - lo)  over pairs (i, i + h) or (2i, 2i + 1)
//     sumcheck_round:  g(t) = sum_i sum_T c_T prod_(j in T) (lo_j + t (hi_j - lo_j)),  t = 0 .. d
//     sumcheck_step:   mle_bind of every table, and sumcheck_round over what it wrote, in one pass
// all mod q with the F_q functions of fr.h, on canonical 8-word records.  The first part of this file is host/device
// code: the geometry, the run of eq values one thread owns, the bind of one pair and the round body of one pair index,
// which tests/native/mle_test.cpp runs on the CPU.  The kernels follow, for the device compiler only.
#pragma once
#include "scalar_kernels.h"
#include "sqrt.h"   // static_for

namespace msmz {

constexpr int MLE_MAX_VARS = 31;                 // a set has fewer than 2^32 entries
// eq: consecutive entries one thread owns, the three low variables expanded in registers
constexpr int MLE_RUN = 8;
// mle_eval: the tile of k_scalars_dot, but a thread's elements are ONE run of consecutive entries
constexpr int MLE_TILE = SDOT_THREADS * MLE_RUN;
// sumcheck_round: pair indices per thread and per workgroup (the tile geometry of k_scalars_dot)
constexpr int MSC_E = SDOT_E;
constexpr int MSC_TILE = SDOT_THREADS * MSC_E;
constexpr int MSC_MAX_TABLES = 6;
constexpr int MSC_MAX_DEGREE = 4;
constexpr int MSC_MAX_TERMS = 8;
// sumcheck_step: the table counts k_scalars_sumcheck_step is instantiated for.  With more tables the compiler has no
// allocation of it without scratch, and the host queues the bind and round kernels instead.
constexpr int MSC_STEP_FUSED_TABLES = 5;
// the head of the result buffer of a round: MSC_MAX_DEGREE + 1 values, then the error word
constexpr int MSC_ERR_WORD = (MSC_MAX_DEGREE + 1) * 8;
constexpr int MSC_HEAD_BYTES = 256;
static_assert(MLE_RUN == 8, "fr_eq_run expands exactly three variables in registers");
static_assert((MSC_ERR_WORD + 1) * 4 <= MSC_HEAD_BYTES, "the values and the error word fit the head");

// the point of an eq table: r_j 2^256 mod q, so that a canonical value times r_j is one product and canonical again
struct FrEqPoint {
  uint32_t r[MLE_MAX_VARS][8];
};

// One thread's run of an eq table: e[k] = scale eq(r, g + k), k < min(MLE_RUN, 2^n_vars); g is a multiple of MLE_RUN
// (0 when n_vars < 3) and scale is canonical, as everything in e.  The high variables first: the running value takes
// the factor r_j or 1 - r_j its index bit selects, as t = acc r_j and then t or acc - t (one product per variable; `j`
// is the same in every lane and indexes the point in the argument segment, not a register array).  Then the low three
// variables 1 -> 2 -> 4 -> 8: child1 = parent r_j, child0 = parent - child1, one product per two children, every index
// a constant after unrolling.  At most n_vars - 3 + 7 products.
template <class Fr>
MSMZ_HD void fr_eq_split(uint32_t* c0, uint32_t* c1, const uint32_t* rj) {   // parent in c0 -> children (c0, c1)
  fr_mont_mul<Fr>(c1, c0, rj);
  fr_sub<Fr>(c0, c0, c1);
}

template <class Fr>
MSMZ_HD void fr_eq_run(uint32_t (&e)[MLE_RUN][8], const uint32_t* scale, const FrEqPoint& pt, uint32_t n_vars, uint32_t g) {
#pragma unroll
  for (int w = 0; w < 8; w++) e[0][w] = scale[w];
#pragma unroll 1
  for (uint32_t j = 3; j < n_vars; j++) {
    uint32_t t[8];
    fr_mont_mul<Fr>(t, e[0], pt.r[j]);
    if ((g >> j) & 1u) {
#pragma unroll
      for (int w = 0; w < 8; w++) e[0][w] = t[w];
    } else {
      fr_sub<Fr>(e[0], e[0], t);
    }
  }
  // (written out: seven splits, each guarded by the variables there are, so a partial run touches no entry it lacks)
  const bool v1 = n_vars > 0, v2 = n_vars > 1, v3 = n_vars > 2;
  if (v3) fr_eq_split<Fr>(e[0], e[4], pt.r[2]);
  if (v2) {
    fr_eq_split<Fr>(e[0], e[2], pt.r[1]);
    if (v3) fr_eq_split<Fr>(e[4], e[6], pt.r[1]);
  }
  if (v1) {
    fr_eq_split<Fr>(e[0], e[1], pt.r[0]);
    if (v2) fr_eq_split<Fr>(e[2], e[3], pt.r[0]);
    if (v3) {
      fr_eq_split<Fr>(e[4], e[5], pt.r[0]);
      fr_eq_split<Fr>(e[6], e[7], pt.r[0]);
    }
  }
}

// out = lo + r (hi - lo): the bind of one pair, r in Montgomery form; one product
template <class Fr>
MSMZ_HD void fr_bind(uint32_t* out, const uint32_t* lo, const uint32_t* hi, const uint32_t* r_mont) {
  uint32_t d[8];
  fr_sub<Fr>(d, hi, lo);
  fr_mont_mul<Fr>(d, r_mont, d);
  fr_add<Fr>(out, lo, d);
}

// The terms of a round as the kernel takes them: term k multiplies the tables of mask[k] and the coefficient, which
// the host has brought to c 2^(256 f) mod q for a term of f factors -- f products through fr_mont_mul then leave
// c prod f_j, canonical, whatever f is, and terms of different degree add up as they are.
struct FrScTerms {
  uint32_t coeff[MSC_MAX_TERMS][8];
  uint32_t mask[MSC_MAX_TERMS];
  uint32_t n_terms;
  uint32_t degree;   // the largest popcount of a mask: the round writes degree + 1 values
};

// c -> c 2^(256 factors) mod q (host: once per term and call)
template <class Fr>
MSMZ_HD void fr_sc_coeff(uint32_t* out, const uint32_t* c, int factors) {
#pragma unroll
  for (int w = 0; w < 8; w++) out[w] = c[w];
  for (int f = 0; f < factors; f++) fr_to_mont<Fr>(out, out);
}

// The round body of one pair index: acc[t] += sum_T c_T prod_(j in T) (lo_j + t (hi_j - lo_j)), t = 0 .. degree.
// cur holds the NT tables' lo on entry and hi their hi; both are used up (hi becomes the difference, cur walks t by
// ADDING it: no product outside the terms).  Masks, coefficients and the loop bounds are the same in every lane; every
// index into cur, hi and acc is a constant after unrolling.
template <class Fr, int NT>
MSMZ_HD void fr_sc_pair(uint32_t (&acc)[MSC_MAX_DEGREE + 1][8], uint32_t (&cur)[NT][8], uint32_t (&hi)[NT][8],
                        const FrScTerms& T) {
  static_for<0, NT>([&](auto J) { fr_sub<Fr>(hi[J], hi[J], cur[J]); });
  static_for<0, MSC_MAX_DEGREE + 1>([&](auto Tt) {   // (unrolled by the language: loops of products inside)
    constexpr int t = decltype(Tt)::value;
    if ((uint32_t)t <= T.degree) {
      if (t) static_for<0, NT>([&](auto J) { fr_add<Fr>(cur[J], cur[J], hi[J]); });
#pragma unroll 1
      for (uint32_t k = 0; k < T.n_terms; k++) {
        const uint32_t m = T.mask[k];
        uint32_t p[8];
#pragma unroll
        for (int w = 0; w < 8; w++) p[w] = T.coeff[k][w];
        static_for<0, NT>([&](auto J) {
          if ((m >> J) & 1u) fr_mont_mul<Fr>(p, p, cur[J]);
        });
        fr_add<Fr>(acc[t], acc[t], p);
      }
    }
  });
}

// The step body of one NEW pair index: the two entries of every bound table that make the pair (lo, hi) of the next
// round are bound from their source pairs, stored, and go into fr_sc_pair as they are -- two fr_bind per table, then the
// round body.  load(J, K, dst) brings source record K of table J (0, 1: lo and hi of the pair that binds into the new
// lo; 2, 3: of the one that binds into the new hi) and returns whether it was >= q; store(J, K, src) takes the bound
// entry K (0: the new lo, 1: the new hi); J and K are integral constants.  A table's first pair is loaded, bound and
// stored before its second is loaded: with the temporary, three records of a table are live at most, and once the loop
// is through the live set is that of the round (cur, hi, acc).  Returns whether any record was >= q.
template <class Fr, int NT, class Load, class Store>
MSMZ_HD bool fr_sc_step(uint32_t (&acc)[MSC_MAX_DEGREE + 1][8], const FrScTerms& T, const uint32_t* r_mont, Load load,
                        Store store) {
  uint32_t cur[NT][8], hi[NT][8];
  bool bad = false;
  static_for<0, NT>([&](auto J) {
    uint32_t t[8];
    bad |= load(J, std::integral_constant<int, 0>{}, cur[J]);
    bad |= load(J, std::integral_constant<int, 1>{}, t);
    fr_bind<Fr>(cur[J], cur[J], t, r_mont);
    store(J, std::integral_constant<int, 0>{}, cur[J]);
    bad |= load(J, std::integral_constant<int, 2>{}, hi[J]);
    bad |= load(J, std::integral_constant<int, 3>{}, t);
    fr_bind<Fr>(hi[J], hi[J], t, r_mont);
    store(J, std::integral_constant<int, 1>{}, hi[J]);
  });
  fr_sc_pair<Fr, NT>(acc, cur, hi, T);
  return bad;
}

// The last step, source tables of ONE variable: every table has one bound entry and no variable is left to sum.  The
// value is the round body on a pair with hi = lo and degree 0 (fr_sc_step with both source pairs the same and
// T.degree == 0; tests/native/sumcheck_step_test.cpp holds the two against each other): acc += sum_T c_T prod_(j in T)
// bound_j, the products in the order of fr_sc_pair.  One pair of loops over tables and terms with nothing indexed in
// registers, so one function serves every table count: load(j, k, dst) brings source record k (0, 1) of table j and
// returns whether it was >= q, store(j, src) takes the bound entry, bound(j, dst) brings it back.
template <class Fr, class Load, class Store, class Bound>
MSMZ_HD bool fr_sc_last(uint32_t* acc, const FrScTerms& T, uint32_t n_tables, const uint32_t* r_mont, Load load, Store store,
                        Bound bound) {
  bool bad = false;
  for (uint32_t j = 0; j < n_tables; j++) {
    uint32_t lo[8], hi[8];
    bad |= load(j, 0, lo);
    bad |= load(j, 1, hi);
    fr_bind<Fr>(lo, lo, hi, r_mont);
    store(j, lo);
  }
  for (uint32_t k = 0; k < T.n_terms; k++) {
    uint32_t p[8];
#pragma unroll
    for (int w = 0; w < 8; w++) p[w] = T.coeff[k][w];
    for (uint32_t j = 0; j < n_tables; j++) {
      if ((T.mask[k] >> j) & 1u) {
        uint32_t v[8];
        bound(j, v);
        fr_mont_mul<Fr>(p, p, v);
      }
    }
    fr_add<Fr>(acc, acc, p);
  }
  return bad;
}

}  // namespace msmz

#if defined(__HIPCC__)
namespace msmz {

static_assert((1 << MULTI_BLOCK_SHIFT) % MLE_RUN == 0, "a run of eq values stays inside one block of set indices");

// out_i = scale eq(r, i), i < 2^n_vars.  Thread t owns entries [t MLE_RUN, (t + 1) MLE_RUN) (fr_eq_run); with fewer
// than three variables thread 0 owns the whole table.  The point is an argument: the `j` of the high variables is
// uniform and reads it from the argument segment.
template <class Fr>
__global__ void __launch_bounds__(256) k_scalars_eq_table(uint32_t* out, FrConst scale, FrEqPoint pt, uint32_t n_vars) {
  const uint64_t n = 1ull << n_vars;
  const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * MLE_RUN;
  if (first >= n) return;
  uint32_t e[MLE_RUN][8];
  fr_eq_run<Fr>(e, scale.w, pt, n_vars, (uint32_t)first);
#pragma unroll
  for (int k = 0; k < MLE_RUN; k++) {
    if (first + k < n) fr_store(out, first + k, e[k]);
  }
}

// partial[tile] = sum over the tile's entries of x_i eq(r, i) 2^-256: k_scalars_dot with its second operand generated.
// Thread t of a tile takes the run of MLE_RUN consecutive entries at tile MLE_TILE + t MLE_RUN: it reads 256 bytes in
// a row, 16 at a time, and the eq values of exactly those entries come from one fr_eq_run.  Folded by
// k_scalars_dot_fold with to_canon.  A record >= q raises bit 2 of *err.
template <class Fr>
__global__ void __launch_bounds__(SDOT_THREADS) k_scalars_mle_eval(uint32_t* partial, const uint32_t* x, FrEqPoint pt,
                                                                   uint32_t n_vars, uint32_t* err) {
  const uint64_t n = 1ull << n_vars;
  const uint64_t first = (uint64_t)blockIdx.x * MLE_TILE + (uint64_t)threadIdx.x * MLE_RUN;
  uint32_t acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0;
  bool bad = false;
  if (first < n) {
    uint32_t one[8];
#pragma unroll
    for (int j = 0; j < 8; j++) one[j] = j == 0 ? 1u : 0u;
    uint32_t e[MLE_RUN][8];
    fr_eq_run<Fr>(e, one, pt, n_vars, (uint32_t)first);
    static_for<0, MLE_RUN>([&](auto K) {
      if (first + K < n) {
        uint32_t a[8];
        const bool b = fr_load<Fr>(a, x, first + K);
        bad |= b;
        fr_mont_mul<Fr>(a, e[K], a);   // (e[K] < q: the product ends below q whatever the record is)
        if (!b) fr_add<Fr>(acc, acc, a);
      }
    });
  }
  if (bad) atomicOr(err, 4u);
  fr_block_sum<Fr>(acc);
  if (threadIdx.x == 0) fr_store(partial, blockIdx.x, acc);
}

// out_i = lo + r (hi - lo), one thread per output, i < count 2^(n_vars - 1); `in` is the first record of table 0 and
// table k follows table k - 1, in the source and in the destination.  High variable: (lo, hi) = entries (i', i' + h)
// of the thread's table, h = 2^(n_vars - 1).  low: entries (2i, 2i + 1), 64 contiguous bytes.  A thread reads its two
// records and then writes its one, so with ONE table and the high variable `out` may be the table's low half; the host
// refuses every other overlap.  A record >= q raises bit 2 of *err.
template <class Fr>
__global__ void __launch_bounds__(256) k_scalars_mle_bind(uint32_t* out, const uint32_t* in, FrConst r_mont, uint32_t n_vars,
                                                          uint32_t total, int low, uint32_t* err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint32_t hbits = n_vars - 1, h = 1u << hbits;
  const uint64_t lo_at = low ? 2ull * i : ((uint64_t)(i >> hbits) << n_vars) + (i & (h - 1));
  const uint64_t hi_at = low ? lo_at + 1 : lo_at + h;
  uint32_t lo[8], hi[8];
  bool bad = fr_load<Fr>(lo, in, lo_at);
  bad |= fr_load<Fr>(hi, in, hi_at);
  if (bad) atomicOr(err, 4u);
  fr_bind<Fr>(lo, lo, hi, r_mont.w);
  fr_store(out, i, lo);
}

// the tables of a round: the first record of each range
struct ScTables {
  const uint32_t* p[MSC_MAX_TABLES];
};

// partial[t tiles + tile] = the tile's share of g(t), t = 0 .. degree (fr_sc_pair over the tile's pair indices; thread
// t takes indices tile MSC_TILE + e SDOT_THREADS + t as k_scalars_dot does).  half = 2^(n_vars - 1) pair indices;
// (lo, hi) = entries (i, i + half), or with `low` (2i, 2i + 1).  NT, the number of tables, is the template parameter:
// every register array is indexed by constants.  One block sum per value; k_scalars_dot_fold, one workgroup per value,
// adds the tiles (the values are canonical already: no conversion).  A record >= q raises bit 2 of *err.
template <class Fr, int NT>
__global__ void __launch_bounds__(SDOT_THREADS) k_scalars_sumcheck_round(uint32_t* partial, ScTables tab, FrScTerms T,
                                                                         uint32_t half, int low, uint32_t* err) {
  const uint64_t base = (uint64_t)blockIdx.x * MSC_TILE + threadIdx.x;
  uint32_t acc[MSC_MAX_DEGREE + 1][8];
#pragma unroll
  for (int t = 0; t <= MSC_MAX_DEGREE; t++) {
#pragma unroll
    for (int w = 0; w < 8; w++) acc[t][w] = 0;
  }
  bool bad = false;
#pragma unroll 1
  for (int e = 0; e < MSC_E; e++) {
    const uint64_t i = base + (uint64_t)e * SDOT_THREADS;
    if (i < half) {
      const uint64_t lo_at = low ? 2 * i : i, hi_at = low ? 2 * i + 1 : i + half;
      uint32_t cur[NT][8], hi[NT][8];
      static_for<0, NT>([&](auto J) {
        bad |= fr_load<Fr>(cur[J], tab.p[J], lo_at);
        bad |= fr_load<Fr>(hi[J], tab.p[J], hi_at);
      });
      fr_sc_pair<Fr, NT>(acc, cur, hi, T);
    }
  }
  if (bad) atomicOr(err, 4u);
  static_for<0, MSC_MAX_DEGREE + 1>([&](auto Tt) {
    constexpr int t = decltype(Tt)::value;
    if ((uint32_t)t <= T.degree) {   // (uniform: every thread of the workgroup reaches the same block sums)
      fr_block_sum<Fr>(acc[t]);
      if (threadIdx.x == 0) fr_store(partial, (uint64_t)t * gridDim.x + blockIdx.x, acc[t]);
      __syncthreads();   // (fr_block_sum's LDS words are free for the next value)
    }
  });
}

// the destinations of a step: the first record of each range
struct ScOuts {
  uint32_t* p[MSC_MAX_TABLES];
};

// msmz_scalars_sumcheck_step: binds every table to r and leaves the partial sums of the NEXT round, the one over the
// bound tables, where k_scalars_sumcheck_round leaves them (the same tiles, the same fold).  quarter = 2^(n_vars - 2) new
// pair indices, thread and tile geometry of the round over them; h = 2 quarter entries per bound table.  New pair index
// i reads the source records `at` and writes the bound entries `to`:
//     high variable:  at = (i, i + h, i + quarter, i + quarter + h), to = (i, i + quarter)
//     low:            at = (4i, 4i + 1, 4i + 2, 4i + 3),             to = (2i, 2i + 1)
// each of them i times a uniform factor plus a uniform offset, formed where it is used (a source table has at most 2^31
// entries: 32 bits hold every index).  A destination may be its own table's low half in the high order: the records a
// thread writes, i and i + quarter, are among the four it reads and among no other thread's, and each is read before it
// is written (fr_sc_step).  n_vars >= 2: the last step is k_scalars_sumcheck_last.  A record >= q raises bit 2 of *err.
template <class Fr, int NT>
__global__ void __launch_bounds__(SDOT_THREADS) k_scalars_sumcheck_step(uint32_t* partial, ScOuts out, ScTables tab,
                                                                        FrScTerms T, FrConst r_mont, uint32_t quarter,
                                                                        int low, uint32_t* err) {
  const uint32_t base = blockIdx.x * MSC_TILE + threadIdx.x;
  const uint32_t h = 2 * quarter;
  const uint32_t at_mul = low ? 4u : 1u, to_mul = low ? 2u : 1u;
  const uint32_t at1 = low ? 1u : h, at2 = low ? 2u : quarter, at3 = low ? 3u : quarter + h, to1 = low ? 1u : quarter;
  uint32_t acc[MSC_MAX_DEGREE + 1][8];
#pragma unroll
  for (int t = 0; t <= MSC_MAX_DEGREE; t++) {
#pragma unroll
    for (int w = 0; w < 8; w++) acc[t][w] = 0;
  }
  bool bad = false;
#pragma unroll 1
  for (int e = 0; e < MSC_E; e++) {
    const uint32_t i = base + (uint32_t)e * SDOT_THREADS;
    if (i < quarter) {
      bad |= fr_sc_step<Fr, NT>(
          acc, T, r_mont.w,
          [&](auto J, auto K, uint32_t* dst) {
            constexpr int k = decltype(K)::value;
            return fr_load<Fr>(dst, tab.p[J], i * at_mul + (k == 0 ? 0u : k == 1 ? at1 : k == 2 ? at2 : at3));
          },
          [&](auto J, auto K, const uint32_t* src) {
            fr_store(out.p[J], i * to_mul + (decltype(K)::value ? to1 : 0u), src);
          });
    }
  }
  if (bad) atomicOr(err, 4u);
  static_for<0, MSC_MAX_DEGREE + 1>([&](auto Tt) {
    constexpr int t = decltype(Tt)::value;
    if ((uint32_t)t <= T.degree) {   // (uniform: every thread of the workgroup reaches the same block sums)
      fr_block_sum<Fr>(acc[t]);
      if (threadIdx.x == 0) fr_store(partial, (uint64_t)t * gridDim.x + blockIdx.x, acc[t]);
      __syncthreads();   // (fr_block_sum's LDS words are free for the next value)
    }
  });
}

// The last step of msmz_scalars_sumcheck_step (n_vars == 1): ONE thread binds entries (0, 1) of every table into entry 0
// of its destination and leaves the terms over the bound entries in partial record 0 (fr_sc_last); the tables and the
// terms are read with uniform indices from the argument segment.  A destination is apart from every other table's
// source and from every other destination, so table j's bind reads the source as it was, in place too, and the bound
// entries read back are the thread's own writes.  Folded like a round of one tile and one value.
template <class Fr>
__global__ void __launch_bounds__(64) k_scalars_sumcheck_last(uint32_t* partial, ScOuts out, ScTables tab, FrScTerms T,
                                                              FrConst r_mont, uint32_t n_tables, uint32_t* err) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t acc[8];
#pragma unroll
  for (int w = 0; w < 8; w++) acc[w] = 0;
  const bool bad = fr_sc_last<Fr>(
      acc, T, n_tables, r_mont.w, [&](uint32_t j, int k, uint32_t* dst) { return fr_load<Fr>(dst, tab.p[j], k); },
      [&](uint32_t j, const uint32_t* src) { fr_store(out.p[j], 0, src); },
      [&](uint32_t j, uint32_t* dst) { load_scalar(dst, out.p[j], 0); });
  if (bad) atomicOr(err, 4u);
  fr_store(partial, 0, acc);
}

}  // namespace msmz
#endif

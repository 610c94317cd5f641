// Stage-level test hooks: kernels that run ONE device routine on caller-supplied inputs and return the raw
// outputs, so that tests/ can check every stage in isolation -- the build's version of the
// reference's per-operation checks (src/field.test.ts:159-211, src/curve-projective.test.ts:77-209,
// src/glv/glv-test.ts:83-125, src/testing/equivalent-wasm.ts:97-147).  Exposed through include/msmz_test.h; they
// never take part in an MSM.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "test_ops.h"

namespace msmz {

enum {   // field ops (msmz_test_field)
  TF_MUL = 0, TF_SQR = 1, TF_ADD = 2, TF_SUB = 3, TF_INVERSE = 4, TF_INVERSE_WAVE = 5, TF_ROUNDTRIP = 6,
  TF_IS_ZERO = 7, TF_SLOT_ROUNDTRIP = 8
};
enum {   // point ops (msmz_test_point)
  TP_ADD = 0, TP_ADD_X4 = 1, TP_MADD = 2, TP_DBL = 3, TP_DBL_X4 = 4
};
enum {   // point ops on memory-format operands (msmz_test_point_raw)
  TPR_ADD = 0, TPR_ADD_X4 = 1, TPR_MADD = 2, TPR_DBL = 3, TPR_DBL_X4 = 4, TPR_MDBL = 5, TPR_CHAIN = 6, TPR_CHAIN_X4 = 7,
  TPR_ADD_ROWS = 8, TPR_DBL_ROWS = 9, TPR_CHAIN_ROWS = 10, TPR_COUNT = 11
};

// Operands / results are NW memory words per element (little endian).  Inputs are lazy Montgomery residues: any
// value in [0, 4p) for the field ops (the kernels write [0, 3p), see fp.h).  Results are the CANONICAL representative of the routine's output residue:
//   MUL a*b/R, SQR a*a/R, ADD, SUB, INVERSE(_WAVE)  R^2/a  (0 for a = 0 mod p), ROUNDTRIP a (store -> load),
//   IS_ZERO  1 / 0 in word 0, SLOT_ROUNDTRIP a through the slot-record format of the tree rounds.
template <class F>
__global__ void __launch_bounds__(64) k_test_field(uint32_t* out, const uint32_t* a_in, const uint32_t* b_in,
                                                   uint32_t n, int op, uint32_t* scratch) {
  constexpr int NW = F::NW;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  // whole waves stay alive: fe_inverse_wave spreads one value over the lanes of a wave
  const uint32_t ii = i < n ? i : n - 1;
  Fe<F> a, b, r;
  fe_unpack<F>(a, a_in + (size_t)ii * NW);
  fe_unpack<F>(b, b_in + (size_t)ii * NW);
  fe_zero(r);
  switch (op) {
    case TF_MUL: fe_mul(r, a, b); break;
    case TF_SQR: fe_sqr(r, a); break;
    case TF_ADD: fe_add(r, a, b); break;
    case TF_SUB: fe_sub(r, a, b); break;
    case TF_INVERSE: fe_inverse(r, a); break;
    case TF_INVERSE_WAVE: {
      // the routine inverts ONE wave-uniform value: feed it lane 0's element, then lane 1's, ...
      for (int l = 0; l < 64; l++) {
        Fe<F> x, y;
#pragma unroll
        for (int j = 0; j < F::N; j++) x.l[j] = __shfl(a.l[j], l, 64);
        fe_inverse_wave(y, x);
        if ((int)(threadIdx.x & 63) == l) r = y;
      }
      break;
    }
    case TF_ROUNDTRIP: {
      uint32_t w[NW];
      fe_store<F>(w, a);
      fe_unpack<F>(r, w);
      break;
    }
    case TF_IS_ZERO: {
      Fe<F> d;
      fe_sub(d, a, b);
      r.l[0] = fe_is_zero(d) ? 1 : 0;
      break;
    }
    case TF_SLOT_ROUNDTRIP: {
      // record i of a chunk-interleaved slot array: (a, b) stored as a point, a also as a parked product
      Affine<F> p, q;
      p.x = a;
      p.y = b;
      slot_store_point<F>(scratch + slot_offset<F>(ii), p, false);
      slot_load_point<F, false>(q, scratch + slot_offset<F>(ii));
      fe_add(r, q.x, q.y);   // a + b
      break;
    }
    default: break;
  }
  if (i >= n) return;
  uint32_t w[NW];
  if (op == TF_IS_ZERO) {
#pragma unroll
    for (int j = 0; j < NW; j++) w[j] = j == 0 ? (uint32_t)r.l[0] : 0u;
  } else {
    fe_to_canon_words<F>(w, r);
  }
#pragma unroll
  for (int j = 0; j < NW; j++) out[(size_t)i * NW + j] = w[j];
}

// field routines on raw register limbs (msmz_test_field_limbs): the ops of field_limbs_op (test_ops.h, the code the
// host contract driver runs too) plus the device-only ones.  a, b, raw: N int32 limbs per element; canon: NW words.
template <class F>
__global__ void __launch_bounds__(64) k_test_field_limbs(int32_t* raw, uint32_t* canon, const int32_t* a_in,
                                                         const int32_t* b_in, uint32_t n, int op, uint32_t* scratch) {
  constexpr int N = F::N, NW = F::NW;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  // whole waves stay alive: fe_inverse_wave spreads one value over the lanes of a wave
  const uint32_t ii = i < n ? i : n - 1;
  Fe<F> a, b, r;
#pragma unroll
  for (int j = 0; j < N; j++) {
    a.l[j] = a_in[(size_t)ii * N + j];
    b.l[j] = b_in[(size_t)ii * N + j];
  }
  int32_t rl[N];
  uint32_t cw[NW];
  if (!field_limbs_op<F>(op, a, b, rl, cw)) {
    fe_zero(r);
    switch (op) {
      case TFL_INVERSE_WAVE:
        for (int l = 0; l < 64; l++) {
          Fe<F> x, y;
#pragma unroll
          for (int j = 0; j < N; j++) x.l[j] = __shfl(a.l[j], l, 64);
          fe_inverse_wave(y, x);
          if ((int)(threadIdx.x & 63) == l) r = y;
        }
        break;
      case TFL_SLOT_MULOUT:
        slot_store_mulout<F>(scratch + slot_offset<F>(ii), a);
        slot_load_fe<F>(r, scratch + slot_offset<F>(ii));
        break;
      case TFL_SLOT_POINT: {
        Affine<F> p, q;
        p.x = a;
        p.y = b;
        slot_store_point<F>(scratch + slot_offset<F>(ii), p, false);
        slot_load_point<F, false>(q, scratch + slot_offset<F>(ii));
        r = q.y;
        fe_to_canon_words<F>(cw, q.x);
        break;
      }
      default: break;
    }
#pragma unroll
    for (int j = 0; j < N; j++) rl[j] = r.l[j];
    if (op != TFL_SLOT_POINT) fe_to_canon_words<F>(cw, r);
  }
  if (i >= n) return;
#pragma unroll
  for (int j = 0; j < N; j++) raw[(size_t)i * N + j] = rl[j];
#pragma unroll
  for (int j = 0; j < NW; j++) canon[(size_t)i * NW + j] = cw[j];
}

// row-form field routines (fp_rows.h) on raw limbs (msmz_test_field_rows): one element per DPP row, lane j = limb j.
// A wave takes as many elements as live_rows has bits, one in each row whose bit is set; the other rows run on zero
// operands.  a, b, raw: N int32 per element (ROUNDTRIP: the NW memory words in the first NW of them); canon: NW words.
enum { TFR_MUL = 0, TFR_ROUNDTRIP = 1, TFR_IS_ZERO = 2, TFR_COUNT = 3 };
template <class F>
__global__ void __launch_bounds__(64) k_test_field_rows(int32_t* raw, uint32_t* canon, const int32_t* a_in,
                                                        const int32_t* b_in, uint32_t n, int op, uint32_t live_rows) {
  constexpr int N = F::N, NW = F::NW;
  __shared__ uint32_t sw[4][NW];
  const RowLane<F> rk = row_lane<F>();
  const uint32_t row = threadIdx.x >> 4;
  const uint32_t i = blockIdx.x * (uint32_t)__popc(live_rows) + (uint32_t)__popc(live_rows & ((1u << row) - 1u));
  const bool live = ((live_rows >> row) & 1u) != 0 && i < n;
  const size_t at = (size_t)(live ? i : 0) * N;   // all 64 lanes stay active: the row routines need whole waves
  int32_t a = 0, b = 0, r = 0;
  if (live && rk.j < N) {
    a = a_in[at + rk.j];
    b = b_in[at + rk.j];
  }
  switch (op) {
    case TFR_MUL:
      r = fe_mul_row<F>(a, b, rk);
      fe_store_row<F>(sw[row], r, rk);
      break;
    case TFR_ROUNDTRIP: {
      const int32_t x = fe_load_row<F>(reinterpret_cast<const uint32_t*>(a_in + at), rk);
      fe_store_row<F>(sw[row], live ? x : 0, rk);
      break;
    }
    default: {
      const bool z = fe_is_zero_row<F>(a, rk);
      r = (rk.j == 0 && z) ? 1 : 0;
      if (rk.j < NW) sw[row][rk.j] = 0;
      break;
    }
  }
  __syncthreads();
  if (!live) return;
  if (op == TFR_ROUNDTRIP) r = rk.j < NW ? (int32_t)sw[row][rk.j] : 0;
  if (rk.j < N) raw[at + rk.j] = r;
  if (rk.j == 0) {
    uint32_t w[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) w[j] = sw[row][j];
    if (op != TFR_IS_ZERO) words_canon<F>(w);
#pragma unroll
    for (int j = 0; j < NW; j++) canon[(size_t)i * NW + j] = w[j];
  }
}

// GLV decomposition of n scalars: out0/out1 = |s0|, |s1| (4 words each), neg[2i], neg[2i+1] = their signs
template <class Fr>
__global__ void __launch_bounds__(256) k_test_glv(uint32_t* s0, uint32_t* s1, uint8_t* neg, const uint32_t* scalars,
                                                  uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (Fr::HAS_GLV) {
    uint32_t s[8], h0[4], h1[4], n0, n1;
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = scalars[(size_t)i * 8 + j];
    glv_decompose<Fr>(h0, h1, n0, n1, s);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      s0[(size_t)i * 4 + j] = h0[j];
      s1[(size_t)i * 4 + j] = h1[j];
    }
    neg[2 * i] = (uint8_t)n0;
    neg[2 * i + 1] = (uint8_t)n1;
  }
}

// signed digits of n scalars as the sort kernels slice them: digits[(h * n + i) * K + k] = l | (negate << 31)
template <class Fr, bool GLV>
__global__ void __launch_bounds__(256) k_test_digits(uint32_t* digits, const uint32_t* scalars, uint32_t n, int c, int K) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int HALVES = GLV ? 2 : 1;
  const uint32_t L = 1u << (c - 1);
  DigitStream<Fr, GLV> ds;
  ds.load(scalars, i, 256);
  for (int k = 0; k < K; k++) {
#pragma unroll
    for (int h = 0; h < HALVES; h++) {
      uint32_t ng;
      const uint32_t l = ds.next(h, k, c, L, ng);
      digits[((size_t)h * n + i) * K + k] = l | (ng << 31);
    }
  }
}

// point operations on pairs of canonical-affine inputs converted to the accumulator type of policy P:
//   out[i] = canonical affine (x | y) of op(a_i, b_i); all-zero = infinity (Weierstrass)
template <class P>
__global__ void __launch_bounds__(64) k_test_point(uint32_t* out, const uint32_t* a_in, const uint32_t* b_in,
                                                   const uint8_t* a_inf, const uint8_t* b_inf, uint32_t n, int op) {
  using F = typename P::F;
  using Acc = typename P::Acc;
  constexpr int NW = F::NW;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool x4 = op == TP_ADD_X4 || op == TP_DBL_X4;
  const uint32_t i = x4 ? t >> 2 : t;   // a DPP quad per pair for the 4-lane addition
  const uint32_t ii = i < n ? i : n - 1;
  auto load = [&](Acc& p, const uint32_t* in, const uint8_t* inf) {
    Fe<F> x, y, xm, ym;
    fe_unpack<F>(x, in + (size_t)ii * 2 * NW);
    fe_unpack<F>(y, in + (size_t)ii * 2 * NW + NW);
    fe_to_mont(xm, x);
    fe_to_mont(ym, y);
    if (!P::TE && inf != nullptr && inf[ii]) P::set_identity(p); else P::from_affine(p, xm, ym);
  };
  Acc a, b, r;
  load(a, a_in, a_inf);
  load(b, b_in, b_inf);
  switch (op) {
    case TP_ADD: P::add(r, a, b); break;
    case TP_ADD_X4: P::add_x4(r, a, b, (int)(threadIdx.x & 3), false); break;
    case TP_DBL_X4: {   // 2 (a + b): the doubling on a general accumulator (ZZ != 1)
      Acc sum;
      P::add_x4(sum, a, b, (int)(threadIdx.x & 3), false);
      P::add_x4(r, sum, sum, (int)(threadIdx.x & 3), true);
      break;
    }
    case TP_DBL: P::dbl(r, a); break;
    case TP_MADD: {   // a + b with b as the input record of the bucket accumulation (affine / Niels, memory format)
      alignas(16) uint32_t rec[4 * NW];   // load_words reads it as 16-byte vectors
      if constexpr (P::TE) {
        Fe<F> ym, yp, kt, k;
        fe_sub(ym, b.Y, b.X);
        fe_add(yp, b.Y, b.X);
        fe_set_const<F>(k, F::K2D);
        fe_mul(kt, b.T, k);
        fe_store<F>(rec, ym);
        fe_store<F>(rec + NW, yp);
        fe_store<F>(rec + 2 * NW, kt);
      } else {
        const bool binf = b_inf != nullptr && b_inf[ii];
        fe_store<F>(rec, b.X);
        fe_store<F>(rec + NW, b.Y);
        if (binf) {
#pragma unroll
          for (int j = 0; j < 2 * NW; j++) rec[j] = 0;
        }
      }
#pragma unroll
      for (int j = 3 * NW; j < 4 * NW; j++) rec[j] = 0;
      P::madd(r, a, rec, 0);
      break;
    }
    default: P::add(r, a, b); break;
  }
  if (i >= n || (x4 && (threadIdx.x & 3) != 0)) return;
  uint32_t w[2 * NW];
  (void)P::to_affine_canon(w, r);
#pragma unroll
  for (int j = 0; j < 2 * NW; j++) out[(size_t)i * 2 * NW + j] = w[j];
}

// point operations on operands in the kernels' own form: every coordinate a lazy memory-format Montgomery residue,
// loaded with fe_unpack as the kernels load it (no conversion).  a[i]: accumulator (X, Y, ZZ, ZZZ) / (X, Y, Z, T),
// 4*NW words.  b[i]: 4*NW words -- an accumulator (ADD, CHAIN), an affine record [x | y | 0 | 0] (MADD, MDBL; all-zero =
// infinity) or a Niels record [y-x | y+x | 2dxy | 0] (TE MADD).  neg[i] (nullable): negate the MADD / MDBL record as the
// bucket accumulation does.  CHAIN: L steps r <- r + b (even steps), r <- 2r (odd steps) in registers, from r = a,
// with the scalar or the 4-lane formulas.  out[i] = canonical affine (x | y) of the result; all-zero = infinity.
// The *_ROWS ops run the row form (add_rows of the policy): one wave per element, launched as one workgroup each.
template <class P>
__global__ void __launch_bounds__(64) k_test_point_raw(uint32_t* out, const uint32_t* a_in, const uint32_t* b_in,
                                                       const uint8_t* neg, uint32_t n, int op, int L) {
  using F = typename P::F;
  using Acc = typename P::Acc;
  constexpr int NW = F::NW;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool x4 = op == TPR_ADD_X4 || op == TPR_DBL_X4 || op == TPR_CHAIN_X4;
  const int s = (int)(threadIdx.x & 3);
  const uint32_t i = x4 ? t >> 2 : t;   // a DPP quad per element for the 4-lane formulas
  const uint32_t ii = i < n ? i : n - 1;
  const uint32_t* arec = a_in + (size_t)ii * 4 * NW;
  const uint32_t* brec = b_in + (size_t)ii * 4 * NW;
  const uint32_t ng = neg != nullptr ? (uint32_t)neg[ii] & 1u : 0u;
  auto load = [&](Acc& p, const uint32_t* rec) {
    Fe<F>* c = reinterpret_cast<Fe<F>*>(&p);
#pragma unroll
    for (int k = 0; k < 4; k++) fe_unpack<F>(c[k], rec + k * NW);
  };
  Acc a, b, r;
  if (op >= TPR_ADD_ROWS) {   // uniform over the launch
    __shared__ uint32_t rec[4 * NW];
    const RowLane<F> rk = row_lane<F>();
    typename P::Row ra, rb, rr;
    acc_load_row<F>(ra, a_in + (size_t)blockIdx.x * 4 * NW, rk);
    acc_load_row<F>(rb, b_in + (size_t)blockIdx.x * 4 * NW, rk);
    if (op == TPR_ADD_ROWS) {
      P::add_rows(rr, ra, rb, false, rk);
    } else if (op == TPR_DBL_ROWS) {
      P::add_rows(rr, ra, ra, true, rk);
    } else {
      rr = ra;
#pragma unroll 1
      for (int k = 0; k < L; k++) {
        typename P::Row u;
        if (k & 1) P::add_rows(u, rr, rr, true, rk); else P::add_rows(u, rr, rb, false, rk);
        rr = u;
      }
    }
    acc_store_row<F>(rec, rr, rk);
    __syncthreads();
    if (threadIdx.x != 0) return;
    load(r, rec);
    uint32_t w[2 * NW];
    (void)P::to_affine_canon(w, r);
#pragma unroll
    for (int j = 0; j < 2 * NW; j++) out[(size_t)blockIdx.x * 2 * NW + j] = w[j];
    return;
  }
  load(a, arec);
  switch (op) {
    case TPR_ADD: load(b, brec); P::add(r, a, b); break;
    case TPR_ADD_X4: load(b, brec); P::add_x4(r, a, b, s, false); break;
    case TPR_DBL: P::dbl(r, a); break;
    case TPR_DBL_X4: P::add_x4(r, a, a, s, true); break;
    case TPR_MADD: P::madd(r, a, brec, ng); break;
    case TPR_MDBL:
      if constexpr (!P::TE) {
        Affine<F> q;
        load_affine<F>(q, brec, ng);
        xyzz_mdbl(r, q);
      } else {
        r = a;
      }
      break;
    case TPR_CHAIN:
    case TPR_CHAIN_X4: {
      load(b, brec);
      r = a;
#pragma unroll 1
      for (int k = 0; k < L; k++) {
        Acc u;
        if (op == TPR_CHAIN) {
          if (k & 1) P::dbl(u, r); else P::add(u, r, b);
        } else {
          if (k & 1) P::add_x4(u, r, r, s, true); else P::add_x4(u, r, b, s, false);
        }
        r = u;
      }
      break;
    }
    default: r = a; break;
  }
  if (i >= n || (x4 && s != 0)) return;
  uint32_t w[2 * NW];
  (void)P::to_affine_canon(w, r);
#pragma unroll
  for (int j = 0; j < 2 * NW; j++) out[(size_t)i * 2 * NW + j] = w[j];
}

// input slot records of msmz_test_batch_add: canonical affine (x | y, 2*NW words) + infinity flags (nullable) ->
// slot records 0 .. n-1 in the tree rounds' format; a coordinate >= p raises err bit 2 (as k_points_to_resident)
template <class F>
__global__ void __launch_bounds__(256) k_test_slots_in(uint32_t* slots, const uint32_t* in, const uint8_t* is_inf,
                                                       uint32_t n, uint32_t* err) {
  constexpr int NW = F::NW;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* w = in + (size_t)i * 2 * NW;
  if (words_geq<NW>(w, F::PW) || words_geq<NW>(w + NW, F::PW)) atomicOr(err, 4u);
  Fe<F> x, y;
  Affine<F> m;
  fe_unpack<F>(x, w);
  fe_unpack<F>(y, w + NW);
  fe_to_mont(m.x, x);
  fe_to_mont(m.y, y);
  slot_store_point<F>(slots + slot_offset<F>(i), m, is_inf != nullptr && is_inf[i] != 0);
}

// results of msmz_test_batch_add: slot records first .. first+n-1 -> canonical affine, all-zero = infinity
template <class F>
__global__ void __launch_bounds__(256) k_test_slots_out(uint32_t* out, const uint32_t* slots, uint32_t first,
                                                        uint32_t n) {
  constexpr int NW = F::NW;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<F> p;
  const bool inf = slot_load_point<F, true>(p, slots + slot_offset<F>(first + i));
  uint32_t w[2 * NW];
  if (inf) {
#pragma unroll
    for (int j = 0; j < 2 * NW; j++) w[j] = 0;
  } else {
    Fe<F> t;
    fe_from_mont(t, p.x);
    fe_to_canon_words<F>(w, t);
    fe_from_mont(t, p.y);
    fe_to_canon_words<F>(w + NW, t);
  }
#pragma unroll
  for (int j = 0; j < 2 * NW; j++) out[(size_t)i * 2 * NW + j] = w[j];
}

// accumulator records of msmz_test_reduce: canonical affine (x | y) + infinity flags (nullable; Weierstrass: an
// all-zero record is infinity too) + scales lambda (nullable, canonical, != 0) -> records 0 .. n-1 as the policy
// stores them: XYZZ (l^2 x, l^3 y, l^2, l^3), extended twisted Edwards (l x, l y, l, l x y).  err bit 2: a coordinate
// or scale >= p; bit 3: a zero scale.
template <class P>
__global__ void __launch_bounds__(256) k_test_accs_in(uint32_t* accs, const uint32_t* in, const uint8_t* is_inf,
                                                      const uint32_t* scale, uint32_t n, uint32_t* err) {
  using F = typename P::F;
  constexpr int NW = F::NW;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* w = in + (size_t)i * 2 * NW;
  if (words_geq<NW>(w, F::PW) || words_geq<NW>(w + NW, F::PW)) atomicOr(err, 4u);
  uint32_t o = 0;
#pragma unroll
  for (int j = 0; j < 2 * NW; j++) o |= w[j];
  Fe<F> x, y, xm, ym, l, l2, l3;
  fe_unpack<F>(x, w);
  fe_unpack<F>(y, w + NW);
  fe_to_mont(xm, x);
  fe_to_mont(ym, y);
  if (scale != nullptr) {
    const uint32_t* sw = scale + (size_t)i * NW;
    if (words_geq<NW>(sw, F::PW)) atomicOr(err, 4u);
    uint32_t so = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) so |= sw[j];
    if (so == 0) atomicOr(err, 8u);
    fe_unpack<F>(x, sw);
    fe_to_mont(l, x);
  } else {
    fe_set_const<F>(l, F::ONE);
  }
  typename P::Acc a;
  if constexpr (P::TE) {
    Fe<F> t;
    fe_mul(a.X, xm, l);
    fe_mul(a.Y, ym, l);
    a.Z = l;
    fe_mul(t, xm, ym);
    fe_mul(a.T, t, l);
  } else {
    if (o == 0 || (is_inf != nullptr && is_inf[i] != 0)) {
      xyzz_set_inf(a);
    } else {
      fe_sqr(l2, l);
      fe_mul(l3, l2, l);
      fe_mul(a.X, xm, l2);
      fe_mul(a.Y, ym, l3);
      a.ZZ = l2;
      a.ZZZ = l3;
    }
  }
  P::store(accs + (size_t)i * P::ACC_WORDS, a);
}

// results of msmz_test_reduce: accumulator records 0 .. n-1 -> canonical affine (Weierstrass: all-zero = infinity)
template <class P>
__global__ void __launch_bounds__(64) k_test_accs_out(uint32_t* out, const uint32_t* accs, uint32_t n) {
  using F = typename P::F;
  constexpr int NW = F::NW;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typename P::Acc a;
  P::load(a, accs + (size_t)i * P::ACC_WORDS);
  uint32_t w[2 * NW];
  (void)P::to_affine_canon(w, a);
#pragma unroll
  for (int j = 0; j < 2 * NW; j++) out[(size_t)i * 2 * NW + j] = w[j];
}

}  // namespace msmz

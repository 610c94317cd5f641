// Fixed-base multiplication (msmz_points_fixed_base, include/msmz.h):
//     out_i = [s_i] B,   i = 0 .. n-1
// a point set made from a resident scalar set and ONE base -- a KZG SRS [tau^i]G, Pedersen vectors, a test SRS with known
// discrete logs -- by a window table of multiples of B instead of a double-and-add chain per point.
//
// This file is the part that needs no device: the digit rule, the shape of the table, the planner with its cost model,
// and the MSMZ_HD steps that the kernels (fixed_kernels.h) and the CPU driver (tests/native/fixed_base_test.cpp) share.
//
// Digits.  A scalar below 2^bits is written in K = ceil((bits + 1) / c) signed digits of width c,
//     s = sum_k d_k 2^(ck),   d_k in [-2^(c-1), 2^(c-1)],
// from the bottom: raw = (window k) + carry; raw > 2^(c-1) gives d_k = raw - 2^c and a carry into window k + 1.  The
// one spare bit of K windows (cK >= bits + 1) keeps the top window's raw value at or below 2^(c-1), so nothing is carried
// out of it.  A scalar ABOVE the bound has more bits than the K windows take: every window is masked to c bits before
// the rule is applied, so its digits are in range all the same (and the carry out of the top is dropped) -- the table
// is never indexed outside, and the caller's error word says that the result is not to be used.
//
// Table.  T_k[w] = w 2^(ck) B for w = 1 .. 2^(c-1): entry k 2^(c-1) + (w - 1), an affine [x | y] record of 2 NW
// Montgomery words like a resident Weierstrass record (the all-zero record: the point at infinity, which a base of
// small order reaches).  A negative digit negates the entry as it is read: y on the Weierstrass curves, x on the
// twisted Edwards curve.
#pragma once
#include <cstdint>

#include "curve.h"

namespace msmz {

constexpr int FIXED_C_MIN = 4, FIXED_C_MAX = 16;
constexpr int FIXED_MAX_WINDOWS = (256 + FIXED_C_MIN) / FIXED_C_MIN;   // c = 4 and no bound on a 256-bit order: 65
constexpr uint64_t FIXED_TABLE_CAP = 64ull << 20;   // bytes of one table (what the cap costs)

// the bound a call's digits are cut for: the caller's (0 = none), at most the bit length of the group order
constexpr int fixed_base_bits(int scalar_bits, int fr_bits) {
  return scalar_bits <= 0 || scalar_bits >= fr_bits ? fr_bits : scalar_bits;
}
constexpr int fixed_base_windows(int bits, int c) { return (bits + c) / c; }   // ceil((bits + 1) / c)
constexpr uint64_t fixed_base_entries(int c, int K) { return (uint64_t)K << (c - 1); }

// ------------------------------------------------------------------------------------------------ digits
// The scalar in a shift register: a digit is cut off the bottom word and the eight words move down c bits, all with
// CONSTANT register indices (the reason scalar_take_top_word, mul_kernels.h, gives for walking from the top).
struct FixedDigits {
  uint32_t r[8];
  uint32_t carry;
};

MSMZ_HD void fixed_digits_begin(FixedDigits& d, const uint32_t* s) {
#pragma unroll
  for (int j = 0; j < 8; j++) d.r[j] = s[j];
  d.carry = 0;
}

// the next digit from the bottom, c in [FIXED_C_MIN, FIXED_C_MAX]: in [-2^(c-1) + 1, 2^(c-1)] for ANY register contents
MSMZ_HD int32_t fixed_digits_next(FixedDigits& d, int c) {
  const uint32_t raw = (d.r[0] & ((1u << c) - 1u)) + d.carry;
#pragma unroll
  for (int j = 0; j < 7; j++) d.r[j] = (d.r[j] >> c) | (d.r[j + 1] << (32 - c));
  d.r[7] >>= c;
  d.carry = raw > (1u << (c - 1)) ? 1u : 0u;
  return (int32_t)raw - (int32_t)(d.carry << c);
}

// the table entry of digit d != 0 of window k
MSMZ_HD uint32_t fixed_entry_index(int k, int32_t d, int c) {
  return ((uint32_t)k << (c - 1)) + (uint32_t)(d < 0 ? -d : d) - 1u;
}

// ------------------------------------------------------------------------------------------------ group steps
// acc = [w] base, w below 2^c: MSB-first double-and-add from the identity with the complete formulas -- one table entry
// from the base 2^(ck) B of its window (k_fixed_table; the CPU driver builds the entries it reads the same way)
template <class G>
MSMZ_HD void fixed_table_multiple(typename G::Acc& acc, const typename G::Base& base, uint32_t w, int c) {
  typename G::Acc t;
  G::set_identity(acc);
#pragma unroll 1
  for (int b = c - 1; b >= 0; b--) {
    G::dbl(t, acc);
    acc = t;
    if ((w >> b) & 1u) {
      G::madd(t, acc, base);
      acc = t;
    }
  }
}

// a table entry (x, y as unpacked from its record, `inf`: the all-zero record) as the base of the complete mixed
// addition, negated if `neg`.  Twisted Edwards: the Niels form of (-x, y), its two sums carried as te_add carries them
template <class G>
MSMZ_HD void fixed_entry_base(typename G::Base& b, const Fe<typename G::F>& x, const Fe<typename G::F>& y, bool inf,
                              uint32_t neg) {
  Fe<typename G::F> s;
  if constexpr (G::TE) {
    fe_cneg(s, x, neg);
    G::base_from_affine(b, s, y, false);
    fe_carry(b.ym);
    fe_carry(b.yp);
  } else {
    fe_cneg(s, y, neg);
    G::base_from_affine(b, x, s, inf);
  }
}

// acc += (+-) the entry: the addition k_points_mul uses, so acc = -entry, acc = entry and either side at infinity are
// covered and a base outside the subgroup gives what the group law gives
template <class G>
MSMZ_HD void fixed_add_entry(typename G::Acc& acc, const Fe<typename G::F>& x, const Fe<typename G::F>& y, bool inf,
                             uint32_t neg) {
  typename G::Base b;
  typename G::Acc t;
  fixed_entry_base<G>(b, x, y, inf, neg);
  G::madd(t, acc, b);
  acc = t;
}

// ------------------------------------------------------------------------------------------------ planner
// The cost MODEL of a call in field products, squarings counted as products (the conventions of points_mul_products,
// mul_kernels.h):
//   one table entry   the chain of fixed_table_multiple over c bits with a multiplier of weight c / 2, and the
//                     wave-wide normalisation (12 + 2 for the scans and the lane's inverse, the affine coordinates)
//   one output point  K mixed additions from affine entries (Weierstrass 8M + 2S; twisted Edwards 7M and the 2M of
//                     the Niels form), and the normalisation with the endomorphism image / the Niels record
// The one fe_inverse_wave per 64 entries or points is in neither, as in points_mul_products.
constexpr int fixed_add_products(bool te) { return te ? 7 + 2 : 10; }
constexpr int fixed_entry_products(bool te, int c) {
  return c * 9 + (c / 2) * (te ? 7 : 10) + 12 + 2 + (te ? 2 : 4);
}
constexpr int fixed_point_products(bool te, int K) {
  return K * fixed_add_products(te) + 12 + 2 + (te ? 2 + 2 : 4 + 1);
}

struct FixedPlan {
  int c, K;
  uint64_t entries;
};

constexpr uint32_t FIXED_CACHE = 4;   // window tables an engine keeps (PointOps::fixed_table, point_ops.h)

// the table of n points with scalars below 2^bits (bits as fixed_base_bits gives it): the c in [4, 16] with the fewest
// products for table and points together, among those whose table fits FIXED_TABLE_CAP; the smaller c on a tie.  For
// fixed bits c does not fall as n grows: a wider window has no more additions per point and a larger table.
static inline FixedPlan fixed_base_plan(uint64_t n, int bits, bool te, int record_bytes) {
  FixedPlan best{0, 0, 0};
  uint64_t best_cost = 0;
  for (int c = FIXED_C_MIN; c <= FIXED_C_MAX; c++) {
    const int K = fixed_base_windows(bits, c);
    const uint64_t entries = fixed_base_entries(c, K);
    if (entries * (uint64_t)record_bytes > FIXED_TABLE_CAP) continue;
    const uint64_t cost = entries * (uint64_t)fixed_entry_products(te, c) + n * (uint64_t)fixed_point_products(te, K);
    if (best.c == 0 || cost < best_cost) {
      best = FixedPlan{c, K, entries};
      best_cost = cost;
    }
  }
  return best;
}

// the plan with c forced (msmz_test_set_fixed_base_window); c outside [4, 16] or a table beyond the cap: c = 0
static inline FixedPlan fixed_base_plan_forced(int c, int bits, int record_bytes) {
  if (c < FIXED_C_MIN || c > FIXED_C_MAX) return FixedPlan{0, 0, 0};
  const int K = fixed_base_windows(bits, c);
  const uint64_t entries = fixed_base_entries(c, K);
  if (entries * (uint64_t)record_bytes > FIXED_TABLE_CAP) return FixedPlan{0, 0, 0};
  return FixedPlan{c, K, entries};
}

}  // namespace msmz

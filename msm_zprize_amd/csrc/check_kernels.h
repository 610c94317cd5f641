// Point-set validation (msmz_check_points, include/msmz.h): is every resident record a point of
// the curve, and does it lie in the subgroup of prime order q?  The reference's isOnCurve / isInSubgroup
// (src/curve-affine.ts:193, src/curve-projective.ts:291-303 and the twisted-Edwards pair), run over a resident set.
//
// The first part of this file is host/device code (MSMZ_HD): the curve equations and the chain [q]P, which
// tests/native/check_points_test.cpp compiles for the CPU.  The kernels follow, for the device compiler only.
#pragma once
#if defined(__HIPCC__)
#include "gen_kernels.h"
#include "kernels.h"
#endif
#include "curve.h"

namespace msmz {

// verdict bits of one point (msmz_check_points): bit 1 is only ever set on a point that passed bit 0's test
constexpr uint8_t CHECK_OFF_CURVE = 1, CHECK_OFF_SUBGROUP = 2;

// y^2 = x^3 + b for a finite affine point in the lazy Montgomery form of the resident records     [1M + 2S]
template <class F>
MSMZ_HD bool weier_on_curve(const Affine<F>& a) {
  Fe<F> yy, xx, xxx, b, t;
  fe_sqr(yy, a.y);
  fe_sqr(xx, a.x);
  fe_mul(xxx, xx, a.x);
  fe_set_const<F>(b, F::B);
  fe_sub(t, yy, xxx);
  fe_sub(t, t, b);
  fe_carry(t);
  return fe_is_zero(t);
}

// -x^2 + y^2 = 1 + d x^2 y^2                                                                       [2M + 2S]
template <class F>
MSMZ_HD bool te_on_curve(const Fe<F>& x, const Fe<F>& y) {
  Fe<F> xx, yy, xy, d, t, one;
  fe_sqr(xx, x);
  fe_sqr(yy, y);
  fe_mul(xy, xx, yy);
  fe_set_const<F>(d, F::D);
  fe_mul(t, xy, d);
  fe_set_const<F>(one, F::ONE);
  fe_sub(yy, yy, xx);
  fe_sub(yy, yy, one);
  fe_sub(yy, yy, t);
  fe_carry(yy);
  return fe_is_zero(yy);
}

// bit i of the group order: the index is the same in every lane, so on the device this is a scalar load from the
// constant Fr::Q and a scalar shift -- no per-lane register holds a bit of q
template <class Fr>
MSMZ_HD uint32_t order_bit(int i) {
  return (Fr::Q[i >> 5] >> (i & 31)) & 1u;
}

// [q]P == O for a finite point P of a short Weierstrass curve (a = 0), q = the order of the curve parameters.
// Plain MSB-first double-and-add from the point at infinity: Fr::BITS doublings, one mixed addition per set bit of q.
// Every lane runs the same doublings and additions; the branches inside xyzz_dbl / xyzz_madd (accumulator at infinity,
// equal to P, equal to -P) are the only divergence, and small-order points do take them: [2](x, 0) = O, and a point of
// order 3 meets acc = -P at the second step.
template <class F, class Fr>
MSMZ_HD bool point_times_order_is_zero(const Affine<F>& base) {
  Xyzz<F> acc, t;
  xyzz_set_inf(acc);
#pragma unroll 1
  for (int i = Fr::BITS - 1; i >= 0; i--) {
    xyzz_dbl(t, acc);
    acc = t;
    if (order_bit<Fr>(i)) {
      xyzz_madd(t, acc, base, false);
      acc = t;
    }
  }
  return xyzz_is_inf(acc);
}

// [q]P == (0, 1) for a point P of the twisted Edwards curve (a = -1), given as its Niels record.  The doubling is the
// unified te_add(acc, acc): a = -1 is a square mod p and d is not, so the addition law has no exceptional pair on this
// curve (Hisil-Wong-Carter-Dawson 2008, section 3) -- the 2- and 4-torsion points included -- and Z never vanishes.
template <class F, class Fr>
MSMZ_HD bool te_point_times_order_is_zero(const TeNiels<F>& base) {
  TeExt<F> acc, t;
  te_set_zero(acc);
#pragma unroll 1
  for (int i = Fr::BITS - 1; i >= 0; i--) {
    te_add(t, acc, acc);
    acc = t;
    if (order_bit<Fr>(i)) {
      te_madd(t, acc, base, 0);
      acc = t;
    }
  }
  Fe<F> d;
  fe_sub(d, acc.Y, acc.Z);
  fe_carry(d);
  return fe_is_zero(acc.X) && fe_is_zero(d);   // X = 0 alone also holds for (0, -1): the identity has Y = Z
}

// field products of one chain, squarings counted as products (the cost model of DESIGN.md section 15 and
// tools/check_points_report.py): 9 per xyzz_dbl, 10 per xyzz_madd; 9 per te_add, 7 per te_madd
template <class Fr>
constexpr int order_weight() {
  int w = 0;
  for (int i = 0; i < Fr::BITS; i++) w += (Fr::Q[i >> 5] >> (i & 31)) & 1u;
  return w;
}

}  // namespace msmz

#if defined(__HIPCC__)
namespace msmz {

// the result record of one msmz_check_points call on one engine, in device memory
struct CheckResult {
  uint32_t off_curve;      // points with CHECK_OFF_CURVE
  uint32_t off_subgroup;   // points with CHECK_OFF_SUBGROUP
  uint32_t first_bad;      // smallest set index with a non-zero verdict; 0xffffffff = none
  uint32_t pad;
};

__device__ __forceinline__ void check_report(CheckResult* res, uint32_t* count, uint32_t index) {
  atomicAdd(count, 1u);
  atomicMin(&res->first_bad, index);   // the minimum, not the last writer: the same answer on every run
}

// verdicts[i] = CHECK_OFF_CURVE or 0 for records [0, n) at `recs` (set indices first .. first + n).  The all-zero record
// is the point at infinity (a flagged input, whatever its coordinates were): on the curve.  One thread per point, a
// streaming kernel: one record read, one byte written.
template <class F>
__global__ void __launch_bounds__(256) k_check_curve(uint8_t* verdicts, CheckResult* res, const uint32_t* recs,
                                                     uint32_t n, uint32_t first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<F> a;
  const bool inf = load_affine<F>(a, recs + (size_t)i * PointFmt<F>::STRIDE, 0);
  const bool bad = !inf && !weier_on_curve<F>(a);
  verdicts[i] = bad ? CHECK_OFF_CURVE : 0;
  if (bad) check_report(res, &res->off_curve, first + i);
}

// twisted Edwards: x and y = (y - x) + x of the Niels record (y - x, y + x, k t, x), as k_te_points_from_niels
template <class F>
__global__ void __launch_bounds__(256) k_te_check_curve(uint8_t* verdicts, CheckResult* res, const uint32_t* recs,
                                                        uint32_t n, uint32_t first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<F> ym, yp, kt, x, y;
  load_fe4<F>(ym, yp, kt, x, recs + (size_t)i * 4 * F::NW);
  fe_add(y, ym, x);
  fe_carry(y);
  const bool bad = !te_on_curve<F>(x, y);
  verdicts[i] = bad ? CHECK_OFF_CURVE : 0;
  if (bad) check_report(res, &res->off_curve, first + i);
}

// after k_check_curve: verdicts[i] |= CHECK_OFF_SUBGROUP where [q]P != O.  Off-curve points and the point at infinity
// are skipped (the group law means nothing for the former).  One thread per point; the accumulator and the base stay in
// registers for the whole chain, no LDS, no scratch.
template <class F, class Fr>
__global__ void __launch_bounds__(256) k_check_subgroup(uint8_t* verdicts, CheckResult* res, const uint32_t* recs,
                                                        uint32_t n, uint32_t first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (verdicts[i] != 0) return;
  Affine<F> a;
  if (load_affine<F>(a, recs + (size_t)i * PointFmt<F>::STRIDE, 0)) return;
  if (point_times_order_is_zero<F, Fr>(a)) return;
  verdicts[i] = CHECK_OFF_SUBGROUP;
  check_report(res, &res->off_subgroup, first + i);
}

template <class F, class Fr>
__global__ void __launch_bounds__(256) k_te_check_subgroup(uint8_t* verdicts, CheckResult* res, const uint32_t* recs,
                                                           uint32_t n, uint32_t first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (verdicts[i] != 0) return;
  TeNiels<F> b;
  Fe<F> x;
  load_fe4<F>(b.ym, b.yp, b.kt, x, recs + (size_t)i * 4 * F::NW);
  if (te_point_times_order_is_zero<F, Fr>(b)) return;
  verdicts[i] = CHECK_OFF_SUBGROUP;
  check_report(res, &res->off_subgroup, first + i);
}

}  // namespace msmz
#endif

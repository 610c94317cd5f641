// Point-set validation (msmz_check_points, include/msmz.h): is every resident record a point of
// the curve, and does it lie in the subgroup of prime order q?  The reference's isOnCurve / isInSubgroup
// (src/curve-affine.ts:193, src/curve-projective.ts:291-303 and the twisted-Edwards pair), run over a resident set.
//
// The first part of this file is host/device code (MSMZ_HD): the chain [q]P over a group of curve.h, which
// tests/native/check_points_test.cpp compiles for the CPU.  The kernels follow, for the device compiler only.
#pragma once
#if defined(__HIPCC__)
#include "kernels.h"
#endif
#include "curve.h"

namespace msmz {

// verdict bits of one point (msmz_check_points): bit 1 is only ever set on a point that passed bit 0's test
constexpr uint8_t CHECK_OFF_CURVE = 1, CHECK_OFF_SUBGROUP = 2;

// bit i of the group order: the index is the same in every lane, so on the device this is a scalar load from the
// constant Fr::Q and a scalar shift -- no per-lane register holds a bit of q
template <class Fr>
MSMZ_HD uint32_t order_bit(int i) {
  return (Fr::Q[i >> 5] >> (i & 31)) & 1u;
}

// [q]P == O for a point P of the curve, q = the order of the curve parameters.  Plain MSB-first double-and-add from
// the identity: Fr::BITS doublings, one mixed addition per set bit of q.  Every lane runs the same doublings and
// additions.  Short Weierstrass (P finite): the branches inside xyzz_dbl / xyzz_madd (accumulator at infinity, equal to
// P, equal to -P) are the only divergence, and small-order points do take them: [2](x, 0) = O, and a point of order 3
// meets acc = -P at the second step.  Twisted Edwards: the unified addition has nothing to branch on (TeGroup, curve.h).
template <class G, class Fr>
MSMZ_HD bool group_times_order_is_zero(const typename G::Base& base) {
  typename G::Acc acc, t;
  G::set_identity(acc);
#pragma unroll 1
  for (int i = Fr::BITS - 1; i >= 0; i--) {
    G::dbl(t, acc);
    acc = t;
    if (order_bit<Fr>(i)) {
      G::madd(t, acc, base);
      acc = t;
    }
  }
  return G::is_identity(acc);
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
// of a Weierstrass set is the point at infinity (a flagged input, whatever its coordinates were): on the curve.  One
// thread per point, a streaming kernel: one record read, one byte written.
template <class P>
__global__ void __launch_bounds__(256) k_check_curve(uint8_t* verdicts, CheckResult* res, const uint32_t* recs,
                                                     uint32_t n, uint32_t first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<typename P::F> x, y;
  const bool inf = P::load_resident_affine(x, y, recs + (size_t)i * P::IN_WORDS);
  const bool bad = !inf && !P::on_curve(x, y);
  verdicts[i] = bad ? CHECK_OFF_CURVE : 0;
  if (bad) check_report(res, &res->off_curve, first + i);
}

// after k_check_curve: verdicts[i] |= CHECK_OFF_SUBGROUP where [q]P != O.  Off-curve points and the point at infinity
// are skipped (the group law means nothing for the former).  One thread per point; the accumulator and the base stay in
// registers for the whole chain, no LDS, no scratch.
template <class P, class Fr>
__global__ void __launch_bounds__(256) k_check_subgroup(uint8_t* verdicts, CheckResult* res, const uint32_t* recs,
                                                        uint32_t n, uint32_t first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (verdicts[i] != 0) return;
  typename P::Base b;
  if (P::load_base(b, recs + (size_t)i * P::IN_WORDS)) return;
  if (group_times_order_is_zero<P, Fr>(b)) return;
  verdicts[i] = CHECK_OFF_SUBGROUP;
  check_report(res, &res->off_subgroup, first + i);
}

}  // namespace msmz
#endif

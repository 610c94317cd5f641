// Per-point scalar multiplication of a resident point set (msmz_points_mul, include/msmz.h):
//     out_i = [s_i] P_i (+ Q_i),   i = 0 .. n-1
// a NEW point set made from resident ones -- IPA generator folding, SRS re-randomisation, fixed-base vectors.
//
// The first part of this file is host/device code (MSMZ_HD): the chain [s]P and the final addition, which
// tests/native/points_mul_test.cpp compiles for the CPU.  The kernels follow, for the device compiler only.
#pragma once
#if defined(__HIPCC__)
#include "gen_kernels.h"
#include "kernels.h"
#endif
#include "curve.h"

namespace msmz {

// The scalar words are walked from the top by a shift register: the top word is taken and the others move up one place,
// all with CONSTANT register indices.  (s[w] with a run-time w is a dynamic index into a register array -- scratch, or an
// array the compiler moves to LDS -- and a chain of selects on constant indices is folded back into exactly that.)
MSMZ_HD uint32_t scalar_take_top_word(uint32_t* r) {
  const uint32_t top = r[7];
#pragma unroll
  for (int j = 7; j > 0; j--) r[j] = r[j - 1];
  return top;
}

// acc = [s] base on a short Weierstrass curve (a = 0); s: 8 words little-endian, below the group order (bits from
// Fr::BITS up are not read).  Plain MSB-first double-and-add from the point at infinity: Fr::BITS doublings and one
// mixed addition per set bit.  The loop indices (word, bit) are the same in every lane and the words come off a shift
// register (scalar_take_top_word); what differs between lanes is whether the addition runs.  The branches inside
// xyzz_dbl / xyzz_madd make the chain complete: a base at infinity, a base of small order ([2](x, 0) = O, acc = -P at
// an odd multiple) and leading zero bits all come out right.
template <class F, class Fr>
MSMZ_HD void point_times_scalar(Xyzz<F>& acc, const Affine<F>& base, bool base_inf, const uint32_t* s) {
  Xyzz<F> t;
  xyzz_set_inf(acc);
  static_assert(((Fr::BITS - 1) >> 5) == 7, "the walk starts in the top word of the 8");
  uint32_t r[8];
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = s[j];
#pragma unroll 1
  for (int w = 7; w >= 0; w--) {
    const uint32_t word = scalar_take_top_word(r);
#pragma unroll 1
    for (int b = (w == 7) ? ((Fr::BITS - 1) & 31) : 31; b >= 0; b--) {
      xyzz_dbl(t, acc);
      acc = t;
      if ((word >> b) & 1u) {
        xyzz_madd(t, acc, base, base_inf);
        acc = t;
      }
    }
  }
}

// r = [s] base + q: the chain, then one complete mixed addition (q at infinity, q = [s] base: a doubling, q = -[s] base)
template <class F, class Fr>
MSMZ_HD void point_times_scalar_plus(Xyzz<F>& r, const Affine<F>& base, bool base_inf, const uint32_t* s,
                                     const Affine<F>& q, bool q_inf) {
  Xyzz<F> acc;
  point_times_scalar<F, Fr>(acc, base, base_inf, s);
  xyzz_madd(r, acc, q, q_inf);
}

// the twisted Edwards curve (a = -1): extended coordinates from the identity (0, 1); the doubling is the unified
// te_add(acc, acc), which has no exceptional pair on this curve (check_kernels.h), so there is nothing to branch on
template <class F, class Fr>
MSMZ_HD void te_point_times_scalar(TeExt<F>& acc, const TeNiels<F>& base, const uint32_t* s) {
  TeExt<F> t;
  te_set_zero(acc);
  static_assert(((Fr::BITS - 1) >> 5) == 7, "the walk starts in the top word of the 8");
  uint32_t r[8];
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = s[j];
#pragma unroll 1
  for (int w = 7; w >= 0; w--) {
    const uint32_t word = scalar_take_top_word(r);
#pragma unroll 1
    for (int b = (w == 7) ? ((Fr::BITS - 1) & 31) : 31; b >= 0; b--) {
      te_add(t, acc, acc);
      acc = t;
      if ((word >> b) & 1u) {
        te_madd(t, acc, base, 0);
        acc = t;
      }
    }
  }
}

template <class F, class Fr>
MSMZ_HD void te_point_times_scalar_plus(TeExt<F>& r, const TeNiels<F>& base, const uint32_t* s, const TeNiels<F>& q) {
  TeExt<F> acc;
  te_point_times_scalar<F, Fr>(acc, base, s);
  te_madd(r, acc, q, 0);
}

// The cost MODEL of one output point in field products, squarings counted as products (DESIGN.md section 16,
// tools/points_mul_report.py): the chain with a scalar of Hamming weight BITS / 2, the addend, and the wave-wide
// normalisation (12 for the prefix and suffix products, the lane's own inverse, the affine coordinates and the
// endomorphism image / the Niels record); the one fe_inverse_wave per 64 points is not in it.
template <class Fr>
constexpr int points_mul_products(bool te, bool addend) {
  return te ? Fr::BITS * 9 + (Fr::BITS / 2) * 7 + (addend ? 7 : 0) + 12 + 2 + 2 + 2
            : Fr::BITS * 9 + (Fr::BITS / 2) * 10 + (addend ? 10 : 0) + 12 + 2 + 4 + 1;
}

}  // namespace msmz

#if defined(__HIPCC__)
namespace msmz {

// the broadcast scalar of a call, passed by value (it arrives in scalar registers)
struct MulScalar {
  uint32_t w[8];
};

// lane's scalar: record i of `scalars`, or the broadcast one; a value >= q raises bit 2 of *err (as k_check_scalars)
template <class Fr>
__device__ __forceinline__ void mul_load_scalar(uint32_t* s, const uint32_t* scalars, const MulScalar& bc, uint32_t i,
                                                uint32_t* err) {
  if (scalars) {
    const uint4* p4 = reinterpret_cast<const uint4*>(scalars + (size_t)i * 8);
    const uint4 a = p4[0], b = p4[1];
    s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
    s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    if (words_geq<8>(s, Fr::Q)) atomicOr(err, 4u);
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = bc.w[j];   // (checked on the host)
  }
}

// inv = 1 / d in every lane of a whole wave, d != 0 mod p: Montgomery's trick across the lanes as in k_precompute_copy
// (exclusive prefix and suffix products by shuffles, ONE fe_inverse_wave of the wave's product).  12 products a lane
// for the scans, 2 for its own inverse.  All 64 lanes must be here.
template <class F>
__device__ __forceinline__ void wave_batch_inverse(Fe<F>& inv_d, const Fe<F>& d) {
  const int lane = (int)(threadIdx.x & 63u);
  Fe<F> inc = d, suf = d, t, u;
#pragma unroll 1
  for (int s = 1; s < 64; s <<= 1) {
    fe_shfl_up(t, inc, s);
    fe_shfl_down(u, suf, s);
    Fe<F> a, b;
    fe_mul(a, inc, t);
    fe_mul(b, suf, u);
    if (lane >= s) inc = a;
    if (lane + s < 64) suf = b;
  }
  Fe<F> pre, total, inv;
  fe_shfl_up(pre, inc, 1);
  if (lane == 0) fe_set_const<F>(pre, F::ONE);
  fe_shfl_down(t, suf, 1);
  if (lane == 63) fe_set_const<F>(t, F::ONE);
#pragma unroll
  for (int j = 0; j < F::N; j++) total.l[j] = __shfl(inc.l[j], 63, 64);
  fe_inverse_wave(inv, total);
  fe_mul(u, inv, pre);
  fe_mul(inv_d, u, t);
}

// out record i = [s_i] P_i (+ Q_i) as an affine record, and (endo) record n + i = its endomorphism image (beta x, y).
// pts / addend / scalars point at the first record of their ranges; scalars == nullptr: the broadcast scalar bc;
// addend == nullptr: none.  One thread per point; the accumulator, the base and the scalar stay in registers for the
// whole chain.  Whole waves stay alive to the inversion (the grid is whole blocks): lanes past n carry the identity.
template <class F, class Fr>
__global__ void __launch_bounds__(256) k_points_mul(uint32_t* out, const uint32_t* pts, const uint32_t* scalars,
                                                    MulScalar bc, const uint32_t* addend, uint32_t n, int endo,
                                                    uint32_t* err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool inf = true;
  Xyzz<F> p;
  xyzz_set_inf(p);
  if (i < n) {
    uint32_t s[8];
    mul_load_scalar<Fr>(s, scalars, bc, i, err);
    Affine<F> a;
    const bool a_inf = load_affine<F>(a, pts + (size_t)i * PointFmt<F>::STRIDE, 0);
    point_times_scalar<F, Fr>(p, a, a_inf, s);
    if (addend) {
      Xyzz<F> t;
      const bool q_inf = load_affine<F>(a, addend + (size_t)i * PointFmt<F>::STRIDE, 0);
      xyzz_madd(t, p, a, q_inf);
      p = t;
    }
    inf = fe_is_zero_mod_p(p.ZZZ);
  }
  Fe<F> d, zi3;
  if (inf) fe_set_const<F>(d, F::ONE); else d = p.ZZZ;
  wave_batch_inverse(zi3, d);   // 1 / ZZZ
  if (i >= n) return;
  Affine<F> m;
  fe_zero(m.x);
  fe_zero(m.y);
  if (!inf) {
    Fe<F> t, zi2;
    fe_mul(t, zi3, p.ZZ);         // 1 / Z
    fe_sqr(zi2, t);               // 1 / ZZ
    fe_mul(m.x, p.X, zi2);
    fe_mul(m.y, p.Y, zi3);
  }
  store_affine<F>(out + (size_t)i * PointFmt<F>::STRIDE, m, inf);
  if (endo) {
    if (!inf) {
      Fe<F> beta, bx;
      fe_set_const<F>(beta, F::BETA);
      fe_mul(bx, m.x, beta);
      m.x = bx;
    }
    store_affine<F>(out + ((size_t)n + i) * PointFmt<F>::STRIDE, m, inf);
  }
}

// the twisted Edwards twin: Niels records (y - x, y + x, k t, x) in and out, the denominator is Z.  Z != 0 for every
// multiple of a point of the curve; a record that is no point of the curve may reach Z = 0, and then the identity is
// stored rather than the wave's product spoiled.
template <class F, class Fr>
__global__ void __launch_bounds__(256) k_te_points_mul(uint32_t* out, const uint32_t* pts, const uint32_t* scalars,
                                                       MulScalar bc, const uint32_t* addend, uint32_t n,
                                                       uint32_t* err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool dead = true;
  TeExt<F> p;
  te_set_zero(p);
  if (i < n) {
    uint32_t s[8];
    mul_load_scalar<Fr>(s, scalars, bc, i, err);
    TeNiels<F> b;
    Fe<F> x;
    load_fe4<F>(b.ym, b.yp, b.kt, x, pts + (size_t)i * 4 * F::NW);
    te_point_times_scalar<F, Fr>(p, b, s);
    if (addend) {
      TeExt<F> t;
      load_fe4<F>(b.ym, b.yp, b.kt, x, addend + (size_t)i * 4 * F::NW);
      te_madd(t, p, b, 0);
      p = t;
    }
    dead = fe_is_zero_mod_p(p.Z);
  }
  Fe<F> d, zi;
  if (dead) fe_set_const<F>(d, F::ONE); else d = p.Z;
  wave_batch_inverse(zi, d);   // 1 / Z
  if (i >= n) return;
  Fe<F> x, y;
  if (dead) {
    fe_zero(x);
    fe_set_const<F>(y, F::ONE);
  } else {
    fe_mul(x, p.X, zi);
    fe_mul(y, p.Y, zi);
  }
  te_store_niels<F>(out + (size_t)i * 4 * F::NW, x, y);
}

}  // namespace msmz
#endif

// Per-point scalar multiplication of a resident point set (msmz_points_mul, include/msmz.h):
//     out_i = [s_i] P_i (+ Q_i),   i = 0 .. n-1
// a NEW point set made from resident ones -- IPA generator folding, SRS re-randomisation, fixed-base vectors.
//
// The first part of this file is host/device code (MSMZ_HD): the chain [s]P and the final addition, which
// tests/native/points_mul_test.cpp compiles for the CPU.  The kernels follow, for the device compiler only.
#pragma once
#if defined(__HIPCC__)
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

// acc = [s] base over a group of curve.h; s: 8 words little-endian, below the group order (bits from Fr::BITS up are
// not read).  Plain MSB-first double-and-add from the identity: Fr::BITS doublings and one mixed addition per set bit.
// The loop indices (word, bit) are the same in every lane and the words come off a shift register
// (scalar_take_top_word); what differs between lanes is whether the addition runs.  Short Weierstrass: the branches
// inside xyzz_dbl / xyzz_madd make the chain complete: a base at infinity, a base of small order ([2](x, 0) = O,
// acc = -P at an odd multiple) and leading zero bits all come out right.  Twisted Edwards: nothing to branch on.
template <class G, class Fr>
MSMZ_HD void group_times_scalar(typename G::Acc& acc, const typename G::Base& base, const uint32_t* s) {
  typename G::Acc t;
  G::set_identity(acc);
  static_assert(((Fr::BITS - 1) >> 5) == 7, "the walk starts in the top word of the 8");
  uint32_t r[8];
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = s[j];
#pragma unroll 1
  for (int w = 7; w >= 0; w--) {
    const uint32_t word = scalar_take_top_word(r);
#pragma unroll 1
    for (int b = (w == 7) ? ((Fr::BITS - 1) & 31) : 31; b >= 0; b--) {
      G::dbl(t, acc);
      acc = t;
      if ((word >> b) & 1u) {
        G::madd(t, acc, base);
        acc = t;
      }
    }
  }
}

// r = [s] base + q: the chain, then one complete mixed addition (q at infinity, q = [s] base: a doubling, q = -[s] base)
template <class G, class Fr>
MSMZ_HD void group_times_scalar_plus(typename G::Acc& r, const typename G::Base& base, const uint32_t* s,
                                     const typename G::Base& q) {
  typename G::Acc acc;
  group_times_scalar<G, Fr>(acc, base, s);
  G::madd(r, acc, q);
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
    load_scalar(s, scalars, i);
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

// out record i = [s_i] P_i (+ Q_i) as a resident record, and (endo) record n + i = its endomorphism image (beta x, y).
// pts / addend / scalars point at the first record of their ranges; scalars == nullptr: the broadcast scalar bc;
// addend == nullptr: none.  One thread per point; the accumulator, the base and the scalar stay in registers for the
// whole chain.  Whole waves stay alive to the inversion (the grid is whole blocks): lanes past n carry the identity.
// `dead`: the denominator is 0 and the identity is stored rather than the wave's product spoiled -- the point at
// infinity (Weierstrass); on the twisted Edwards curve Z != 0 for every multiple of a point of the curve, and only a
// record that is no point of the curve may reach Z = 0.
template <class P, class Fr>
__global__ void __launch_bounds__(256) k_points_mul(uint32_t* out, const uint32_t* pts, const uint32_t* scalars,
                                                    MulScalar bc, const uint32_t* addend, uint32_t n, int endo,
                                                    uint32_t* err) {
  using F = typename P::F;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool dead = true;
  typename P::Acc p;
  P::set_identity(p);
  if (i < n) {
    uint32_t s[8];
    mul_load_scalar<Fr>(s, scalars, bc, i, err);
    typename P::Base b;
    P::load_base(b, pts + (size_t)i * P::IN_WORDS);
    group_times_scalar<P, Fr>(p, b, s);
    if (addend) {
      typename P::Acc t;
      P::load_base(b, addend + (size_t)i * P::IN_WORDS);
      P::madd(t, p, b);
      p = t;
    }
    dead = fe_is_zero_mod_p(P::denominator(p));
  }
  Fe<F> d, inv;
  if (dead) fe_set_const<F>(d, F::ONE); else d = P::denominator(p);
  wave_batch_inverse(inv, d);
  if (i >= n) return;
  P::store_normalised(out, i, n, p, inv, dead, endo);
}

}  // namespace msmz
#endif

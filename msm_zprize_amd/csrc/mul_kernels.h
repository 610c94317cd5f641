// Per-point scalar multiplication of a resident point set (msmz_points_mul, msmz_points_mul_opts, include/msmz.h;
// DESIGN.md section 16):
//     out_i = [s_i] P_i (+ Q_i),   i = 0 .. n-1
// a NEW point set made from resident ones -- IPA generator folding, SRS re-randomisation.  (Fixed-base vectors [s_i]B
// for one base B: fixed_kernels.h, a window table instead of a chain per point.)
//
// The first part of this file is host/device code (MSMZ_HD): the chain [s]P over all or the low `bits` bits, the GLV
// table and joint chain, the final addition, the choice of chain and the cost models, which
// tests/native/points_mul_test.cpp and points_mul_opts_test.cpp compile for the CPU.  The kernels follow, for the
// device compiler only.
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

// acc = [s] base over a group of curve.h; s: 8 words little-endian, below 2^bits (bits from `bits` up are not read);
// `bits` in [1, Fr::BITS], the same in every lane.  Plain MSB-first double-and-add from the identity: `bits` doublings
// and one mixed addition per set bit.  The loop indices (word, bit) are the same in every lane and the words come off a
// shift register (scalar_take_top_word): the words above the top word of the walk are taken and dropped first, so the
// register indices stay constant whatever `bits` is.  What differs between lanes is whether the addition runs.  Short
// Weierstrass: the branches inside xyzz_dbl / xyzz_madd make the chain complete: a base at infinity, a base of small
// order ([2](x, 0) = O, acc = -P at an odd multiple) and leading zero bits all come out right.  Twisted Edwards:
// nothing to branch on.
template <class G, class Fr>
MSMZ_HD void group_times_scalar(typename G::Acc& acc, const typename G::Base& base, const uint32_t* s, int bits) {
  typename G::Acc t;
  G::set_identity(acc);
  static_assert(((Fr::BITS - 1) >> 5) == 7, "an unbounded walk starts in the top word of the 8");
  uint32_t r[8];
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = s[j];
  const int top = (bits - 1) >> 5;
#pragma unroll 1
  for (int w = 7; w > top; w--) (void)scalar_take_top_word(r);
#pragma unroll 1
  for (int w = top; w >= 0; w--) {
    const uint32_t word = scalar_take_top_word(r);
#pragma unroll 1
    for (int b = (w == top) ? ((bits - 1) & 31) : 31; b >= 0; b--) {
      G::dbl(t, acc);
      acc = t;
      if ((word >> b) & 1u) {
        G::madd(t, acc, base);
        acc = t;
      }
    }
  }
}

// all Fr::BITS bits: any s below the group order
template <class G, class Fr>
MSMZ_HD void group_times_scalar(typename G::Acc& acc, const typename G::Base& base, const uint32_t* s) {
  group_times_scalar<G, Fr>(acc, base, s, Fr::BITS);
}

// r = [s] base + q: the chain, then one complete mixed addition (q at infinity, q = [s] base: a doubling, q = -[s] base)
template <class G, class Fr>
MSMZ_HD void group_times_scalar_plus(typename G::Acc& r, const typename G::Base& base, const uint32_t* s,
                                     const typename G::Base& q, int bits = Fr::BITS) {
  typename G::Acc acc;
  group_times_scalar<G, Fr>(acc, base, s, bits);
  G::madd(r, acc, q);
}

// ------------------------------------------------------------------------------------------------ the GLV chain
// For a point P of the prime-order subgroup of a short Weierstrass curve with the endomorphism phi(x, y) = (beta x, y)
// = [lambda]P, and s = (+-)k0 + (+-)k1 lambda mod q (glv_decompose, scalar.h: k0, k1 < 2^GLV_PROVEN_BITS for every s):
//     [s]P = [k0]A + [k1]B,   A = (+-)P,  B = (+-)phi P
// walked jointly: GLV_PROVEN_BITS doublings and one mixed addition of A, B or T = A + B wherever either half has a bit.
// The table is five field elements in a store of the caller's, read by slot: the x of A, B and T and the y of A and T
// (the y of B is that of A, negated when the signs differ: `flip`).  The CPU driver keeps them in an array
// (GlvSlotsRegs); the kernel keeps them in LDS (GlvSlotsLds), so that the chain holds no more registers than the plain
// one: the accumulator, the entry of the step and the formulas' temporaries.
// A point outside the subgroup gives SOME point of the curve or infinity (phi P = [lambda]P does not hold there), never
// a fault: every entry is a point of the curve or flagged as infinity.
enum { GLV_X = 0, GLV_BX = 1, GLV_TX = 2, GLV_YA = 3, GLV_TY = 4, GLV_SLOTS = 5 };
struct GlvFlags {
  bool flip;    // B = (beta x, -ya)
  bool inf;     // P at infinity: every entry is
  bool t_inf;   // T at infinity
};

template <class F>
struct GlvSlotsRegs {
  Fe<F> e[GLV_SLOTS];
  MSMZ_HD void put(int slot, const Fe<F>& a) { e[slot] = a; }
  MSMZ_HD void get(int slot, Fe<F>& a) const { a = e[slot]; }
};

// First half of the table: A, beta x (one product), and d = (beta - 1) x, the denominator of T = A + B when the signs
// differ.  t_inf then says that d must not be inverted: P at infinity, or x = 0 mod p, where B = -A and T = O.
template <class G, class Slots>
MSMZ_HD void glv_table_begin(GlvFlags& t, Slots& slots, Fe<typename G::F>& d, const typename G::Base& base, uint32_t neg0,
                             uint32_t neg1) {
  using F = typename G::F;
  static_assert(!G::TE, "the endomorphism is that of the short Weierstrass curves");
  Fe<F> beta, bx, ya;
  t.inf = base.inf;
  t.flip = ((neg0 ^ neg1) & 1u) != 0;
  fe_cneg(ya, base.a.y, neg0);
  fe_set_const<F>(beta, F::BETA);
  fe_mul(bx, base.a.x, beta);
  fe_sub(d, bx, base.a.x);
  fe_carry(d);
  t.t_inf = t.inf || (t.flip && fe_is_zero(d));
  slots.put(GLV_X, base.a.x);
  slots.put(GLV_YA, ya);
  slots.put(GLV_BX, bx);
}

// Second half: T.  Equal signs: A + B = (+-)(P + phi P) = (+-)(-x - beta x, -y) = (beta^2 x, -ya) for EVERY point of the
// curve (1 + beta + beta^2 = 0), no inverse read.  Unequal signs: the affine addition with inv = 1 / d; not read when
// t_inf (the slots then hold zeros, which no step reads).
template <class G, class Slots>
MSMZ_HD void glv_table_finish(const GlvFlags& t, Slots& slots, const Fe<typename G::F>& inv) {
  using F = typename G::F;
  Affine<F> a, b, r;
  slots.get(GLV_X, a.x);
  slots.get(GLV_YA, a.y);
  slots.get(GLV_BX, b.x);
  if (!t.flip) {
    Fe<F> u;
    fe_add(u, a.x, b.x);
    fe_neg(r.x, u);
    fe_neg(r.y, a.y);
  } else if (!t.t_inf) {
    fe_neg(b.y, a.y);
    affine_add_with_inv(r, a, b, inv);
  } else {
    fe_zero(r.x);
    fe_zero(r.y);
  }
  fe_carry(r.x);
  fe_carry(r.y);
  slots.put(GLV_TX, r.x);
  slots.put(GLV_TY, r.y);
}

// the top word of a 4-word half, the others moving up (as scalar_take_top_word)
MSMZ_HD uint32_t half_take_top_word(uint32_t* r) {
  const uint32_t top = r[3];
#pragma unroll
  for (int j = 3; j > 0; j--) r[j] = r[j - 1];
  return top;
}

// acc = [k0]A + [k1]B from the identity; k0, k1: 4 words each, below 2^GLV_PROVEN_BITS.  The entry of a step is read
// from its slots; xyzz_madd's own branches keep the chain complete when acc = (+-) the entry.
template <class G, class Fr, class Slots>
MSMZ_HD void group_times_glv(typename G::Acc& acc, const GlvFlags& tb, const Slots& slots, const uint32_t* k0,
                             const uint32_t* k1) {
  using F = typename G::F;
  static_assert(GLV_X == 0 && GLV_BX == 1 && GLV_TX == 2, "slot sel - 1 is the x of entry sel");
  constexpr int H = Fr::GLV_PROVEN_BITS;
  static_assert(Fr::HAS_GLV && H > 96 && H <= 128, "the walk starts in the top word of the 4");
  typename G::Acc t;
  G::set_identity(acc);
  uint32_t r0[4], r1[4];
#pragma unroll
  for (int j = 0; j < 4; j++) r0[j] = k0[j], r1[j] = k1[j];
#pragma unroll 1
  for (int w = 3; w >= 0; w--) {
    const uint32_t w0 = half_take_top_word(r0), w1 = half_take_top_word(r1);
#pragma unroll 1
    for (int b = (w == 3) ? ((H - 1) & 31) : 31; b >= 0; b--) {
      G::dbl(t, acc);
      acc = t;
      const uint32_t sel = ((w0 >> b) & 1u) | (((w1 >> b) & 1u) << 1);
      if (sel) {
        typename G::Base e;
        Fe<F> y;
        slots.get((int)sel - 1, e.a.x);   // GLV_X, GLV_BX, GLV_TX
        slots.get(sel == 3u ? GLV_TY : GLV_YA, y);
        fe_cneg(e.a.y, y, (sel == 2u && tb.flip) ? 1u : 0u);
        e.inf = tb.inf || (sel == 3u && tb.t_inf);
        G::madd(t, acc, e);
        acc = t;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ which chain
// msmz_points_mul_opts (include/msmz.h): the chain of a call and its number of doublings, from the caller's vouch
// (`subgroup`: MSMZ_MUL_SUBGROUP) and bound (scalar_bits; 0 = none).  Host only.
enum MulChainKind { MUL_CHAIN_PLAIN = 0, MUL_CHAIN_GLV = 1 };
struct MulChain {
  int kind;
  int steps;
};
template <class Fr>
constexpr MulChain points_mul_chain(bool subgroup, int scalar_bits) {
  const int b = (scalar_bits <= 0 || scalar_bits >= Fr::BITS) ? Fr::BITS : scalar_bits;
  if (b < Fr::BITS && b <= Fr::GLV_PROVEN_BITS) return MulChain{MUL_CHAIN_PLAIN, b};   // no longer than the halves
  if (subgroup && Fr::HAS_GLV) return MulChain{MUL_CHAIN_GLV, Fr::GLV_PROVEN_BITS};   // the proven bound: no retry
  return MulChain{MUL_CHAIN_PLAIN, b};
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

// the plain chain over `bits` bits (a scalar of Hamming weight bits / 2): points_mul_products with that chain length
template <class Fr>
constexpr int points_mul_products_bounded(bool te, bool addend, int bits) {
  return te ? bits * 9 + (bits / 2) * 7 + (addend ? 7 : 0) + 12 + 2 + 2 + 2
            : bits * 9 + (bits / 2) * 10 + (addend ? 10 : 0) + 12 + 2 + 4 + 1;
}

// the GLV chain: h = GLV_PROVEN_BITS doublings, an addition at three steps of four, beta x, the lane's share of the
// table's batch inversion (12 + 2), the affine addition of T, the addend, and the normalisation as above
template <class Fr>
constexpr int points_mul_products_glv(bool addend) {
  return Fr::GLV_PROVEN_BITS * 9 + (3 * Fr::GLV_PROVEN_BITS / 4) * 10 + 1 + 14 + 3 + (addend ? 10 : 0) + 12 + 2 + 4 + 1;
}

}  // namespace msmz

#if defined(__HIPCC__)
namespace msmz {

// the broadcast scalar of a call, passed by value (it arrives in scalar registers)
struct MulScalar {
  uint32_t w[8];
};

// lane's scalar: record i of `scalars`, or the broadcast one; a resident value >= q or (BOUNDED) >= 2^bits (the caller's
// bound, the same in every lane) raises bit 2 of *err (as k_check_scalars)
template <class Fr, bool BOUNDED>
__device__ __forceinline__ void mul_load_scalar(uint32_t* s, const uint32_t* scalars, const MulScalar& bc, uint32_t i,
                                                int bits, uint32_t* err) {
  if (scalars) {
    load_scalar(s, scalars, i);
    if (words_geq<8>(s, Fr::Q) || (BOUNDED && words_geq_pow2(s, bits))) atomicOr(err, 4u);
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
// addend == nullptr: none.  BOUNDED: the chain walks `bits` bits and every scalar is below 2^bits; otherwise `bits` is not
// read and the chain walks Fr::BITS, with compile-time loop bounds: the instance of a call without a bound, kept apart
// because run-time bounds changed its schedule (2 to 3 % at 2^16 points on two curves).  One
// thread per point; the accumulator, the base and the scalar stay in registers for the whole chain.  Whole waves stay
// alive to the inversion (the grid is whole blocks): lanes past n carry the identity.
// `dead`: the denominator is 0 and the identity is stored rather than the wave's product spoiled -- the point at
// infinity (Weierstrass); on the twisted Edwards curve Z != 0 for every multiple of a point of the curve, and only a
// record that is no point of the curve may reach Z = 0.
template <class P, class Fr, bool BOUNDED>
__global__ void __launch_bounds__(256) k_points_mul(uint32_t* out, const uint32_t* pts, const uint32_t* scalars,
                                                    MulScalar bc, const uint32_t* addend, uint32_t n, int endo,
                                                    int bits, uint32_t* err) {
  using F = typename P::F;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int walk = BOUNDED ? bits : Fr::BITS;
  bool dead = true;
  typename P::Acc p;
  P::set_identity(p);
  if (i < n) {
    uint32_t s[8];
    mul_load_scalar<Fr, BOUNDED>(s, scalars, bc, i, walk, err);
    typename P::Base b;
    P::load_base(b, pts + (size_t)i * P::IN_WORDS);
    group_times_scalar<P, Fr>(p, b, s, walk);
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

// the broadcast scalar of a GLV call, decomposed on the host (glv_decompose), passed by value
struct MulGlvScalar {
  uint32_t k0[4], k1[4];
  uint32_t neg0, neg1;
};

// The table of a block in LDS: slot s of thread t is the column t of rows [s N, (s + 1) N) of a [5 N][256] array --
// limb j of a thread 256 words after limb j - 1, so a wave's access is 64 consecutive words and no bank conflicts with
// another; nothing is shared between threads, so there is no barrier.  45 KB (255-bit field) / 70 KB (377 / 381 bits) a
// block: three / two blocks a CU, the 3 / 2 waves per SIMD of k_points_mul.  With the table in registers the kernel
// needed 254 (BLS12-377) and 183 (Pallas: a wave less than k_points_mul) and spilled when held to 168.
template <class F>
struct GlvSlotsLds {
  int32_t* col;   // this thread's column
  __device__ __forceinline__ void put(int slot, const Fe<F>& a) {
#pragma unroll
    for (int j = 0; j < F::N; j++) col[(slot * F::N + j) * 256] = a.l[j];
  }
  __device__ __forceinline__ void get(int slot, Fe<F>& a) const {
#pragma unroll
    for (int j = 0; j < F::N; j++) a.l[j] = col[(slot * F::N + j) * 256];
  }
};

// k_points_mul by the GLV chain (group_times_glv) for points the caller vouches to lie in the subgroup; Weierstrass
// only.  A resident scalar is checked (< q, < 2^bits) and decomposed by its lane; bits only bounds, the chain has
// GLV_PROVEN_BITS steps.  The table's T = A + B needs 1 / ((beta - 1) x) where the signs of the halves differ: ONE more
// wave_batch_inverse, all 64 lanes present, and lanes past n, lanes with P at infinity or x = 0 and lanes with equal
// signs feed it a 1.  With a broadcast scalar the signs are the same in every lane, and equal signs skip the inversion.
template <class P, class Fr>
__global__ void __launch_bounds__(256) k_points_mul_glv(uint32_t* out, const uint32_t* pts, const uint32_t* scalars,
                                                        MulGlvScalar bc, const uint32_t* addend, uint32_t n, int endo,
                                                        int bits, uint32_t* err) {
  using F = typename P::F;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  uint32_t k0[4], k1[4], neg0 = bc.neg0, neg1 = bc.neg1;
#pragma unroll
  for (int j = 0; j < 4; j++) k0[j] = bc.k0[j], k1[j] = bc.k1[j];
  if (live && scalars) {
    uint32_t s[8];
    load_scalar(s, scalars, i);
    if (words_geq<8>(s, Fr::Q) || words_geq_pow2(s, bits)) atomicOr(err, 4u);
    glv_decompose<Fr>(k0, k1, neg0, neg1, s);
  }
  __shared__ int32_t table[GLV_SLOTS * F::N * 256];
  GlvSlotsLds<F> slots{table + threadIdx.x};
  GlvFlags tb;
  Fe<F> d, inv;
  tb.inf = tb.t_inf = true;
  tb.flip = false;
  if (live) {
    typename P::Base b;
    P::load_base(b, pts + (size_t)i * P::IN_WORDS);
    glv_table_begin<P>(tb, slots, d, b, neg0, neg1);
  }
  fe_set_const<F>(inv, F::ONE);
  if (scalars || ((bc.neg0 ^ bc.neg1) & 1u)) {   // (the same in every lane)
    if (!tb.flip || tb.t_inf) fe_set_const<F>(d, F::ONE);
    wave_batch_inverse(inv, d);
  }
  bool dead = true;
  typename P::Acc p;
  P::set_identity(p);
  if (live) {
    glv_table_finish<P>(tb, slots, inv);
    group_times_glv<P, Fr>(p, tb, slots, k0, k1);
    if (addend) {
      typename P::Acc t;
      typename P::Base b;
      P::load_base(b, addend + (size_t)i * P::IN_WORDS);
      P::madd(t, p, b);
      p = t;
    }
    dead = fe_is_zero_mod_p(P::denominator(p));
  }
  if (dead) fe_set_const<F>(d, F::ONE); else d = P::denominator(p);
  wave_batch_inverse(inv, d);
  if (!live) return;
  P::store_normalised(out, i, n, p, inv, dead, endo);
}

}  // namespace msmz
#endif

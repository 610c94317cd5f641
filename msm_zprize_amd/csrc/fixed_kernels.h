// The kernels of msmz_points_fixed_base (fixed_base.h: digits, table shape, planner): the window
// table of one base, and the points [s_i]B as K gathers from it and K complete mixed additions each.
#pragma once
#include <hip/hip_runtime.h>

#include "fixed_base.h"
#include "kernels.h"
#include "mul_kernels.h"

namespace msmz {

// table[k 2^(c-1) + w - 1] = w base_k as an affine [x | y] record, base_k = 2^(ck) B from the host (record k of
// `bases`, the all-zero record: the point at infinity).  One thread per entry; the normalisation is wave-wide (one
// fe_inverse_wave per 64 entries, where k_gen_table pays one fe_inverse per thread), so the grid is whole blocks and no
// lane leaves before it: lanes past the end and entries at infinity (a base of small order, a base at infinity) feed
// it a 1.  An entry at infinity is the all-zero record (Weierstrass) / the identity (0, 1) (twisted Edwards).
template <class P>
__global__ void __launch_bounds__(256) k_fixed_table(uint32_t* table, const uint32_t* bases, uint32_t entries, int c) {
  using F = typename P::F;
  constexpr int RW = 2 * F::NW;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  bool dead = true;
  typename P::Acc acc;
  P::set_identity(acc);
  if (t < entries) {
    const uint32_t k = t >> (c - 1), w = (t & ((1u << (c - 1)) - 1u)) + 1u;
    Affine<F> a;
    const bool inf = load_affine<F>(a, bases + (size_t)k * RW, 0);
    typename P::Base b;
    fixed_entry_base<P>(b, a.x, a.y, inf, 0);
    fixed_table_multiple<P>(acc, b, w, c);
    dead = fe_is_zero_mod_p(P::denominator(acc));
  }
  Fe<F> d, inv;
  if (dead) fe_set_const<F>(d, F::ONE); else d = P::denominator(acc);
  wave_batch_inverse(inv, d);
  if (t >= entries) return;
  Affine<F> r;
  fe_zero(r.x);
  if (P::TE) fe_set_const<F>(r.y, F::ONE); else fe_zero(r.y);
  if (!dead) P::affine_from_inverse(r.x, r.y, acc, inv);
  store_affine<F>(table + (size_t)t * RW, r, dead && !P::TE);
}

// the record of digit d of window k into w, issued and not waited for; d == 0: no entry, nothing is read
template <class F>
__device__ __forceinline__ void fixed_gather(uint32_t* w, const uint32_t* table, int k, int32_t d, int c) {
  if (d != 0) load_words<F>(w, table + (size_t)fixed_entry_index(k, d, c) * (2 * F::NW));
}

// out record i = [s_i] B as a resident record, and (endo) record n + i = its endomorphism image; s_i = record i of
// `scalars` (the first of the call's range), `table` as k_fixed_table leaves it for (c, K).  One thread per scalar:
// the scalar is checked (>= q, or BOUNDED and >= 2^bits: bit 2 of *err, as k_points_mul), cut into K signed digits
// from the bottom (fixed_digits_next: in range whatever the scalar, so the table is never indexed outside), and every
// non-zero digit is one gather and one complete mixed addition.  The gather of window k + 1 is issued before the
// addition of window k: an entry is a dependent read of a table that lives in L2 or the Infinity Cache, and the
// addition's ~10 products are what there is to hide it behind.  Registers: the accumulator, two raw records, the
// formulas' temporaries.  Whole waves stay alive to the inversion (the grid is whole blocks): lanes past n carry the
// identity.  `dead` as in k_points_mul.
template <class P, class Fr, bool BOUNDED>
__global__ void __launch_bounds__(256) k_fixed_mul(uint32_t* out, const uint32_t* table, const uint32_t* scalars,
                                                   uint32_t n, int endo, int c, int K, int bits, uint32_t* err) {
  using F = typename P::F;
  constexpr int RW = 2 * F::NW;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t s[8];
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = 0;   // (a lane past n: every digit 0, no gather, no addition)
  if (i < n) {
    load_scalar(s, scalars, i);
    if (words_geq<8>(s, Fr::Q) || (BOUNDED && words_geq_pow2(s, bits))) atomicOr(err, 4u);
  }
  FixedDigits dg;
  fixed_digits_begin(dg, s);
  typename P::Acc p;
  P::set_identity(p);
  uint32_t cur[RW], nxt[RW];
#pragma unroll
  for (int j = 0; j < RW; j++) cur[j] = nxt[j] = 0;
  int32_t d = fixed_digits_next(dg, c);
  fixed_gather<F>(cur, table, 0, d, c);
#pragma unroll 1
  for (int k = 0; k < K; k++) {
    int32_t dn = 0;
    if (k + 1 < K) {
      dn = fixed_digits_next(dg, c);
      fixed_gather<F>(nxt, table, k + 1, dn, c);
    }
    if (d != 0) {
      uint32_t o = 0;
#pragma unroll
      for (int j = 0; j < RW; j++) o |= cur[j];
      Fe<F> x, y;
      fe_unpack<F>(x, cur);
      fe_unpack<F>(y, cur + F::NW);
      fixed_add_entry<P>(p, x, y, o == 0, d < 0 ? 1u : 0u);
    }
    d = dn;
#pragma unroll
    for (int j = 0; j < RW; j++) cur[j] = nxt[j];
  }
  const bool dead = i >= n || fe_is_zero_mod_p(P::denominator(p));
  Fe<F> den, inv;
  if (dead) fe_set_const<F>(den, F::ONE); else den = P::denominator(p);
  wave_batch_inverse(inv, den);
  if (i >= n) return;
  P::store_normalised(out, i, n, p, inv, dead, endo);
}

}  // namespace msmz

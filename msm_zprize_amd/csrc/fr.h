// Arithmetic in the scalar field F_q on 8 saturated 32-bit words, little endian -- the format of a resident scalar set
// (msmz_scalars_combine / _dot / _powers and msmz_scalars_recurrence / _inverse, include/msmz.h; DESIGN.md sections 18
// and 19).  Operands and results are canonical (< q) unless a comment says otherwise, so whatever these functions write
// is what an upload would have left.
//
// Saturated words, not the lazy limbs of fp.h: the kernels built on this file (scalar_kernels.h) move 64 to 160 bytes
// per Montgomery product and sit at the memory bound, the values have to be canonical in memory anyway (a lazy form
// would need a normalisation on every load and store), and q < 2^255 on all four curves, so a sum of two operands fits
// the 8 words without a ninth.  fp_cios.h shows the schedule; this is its 8-word instance over Fr::Q / Fr::QINV32.
//
// Host and device (MSMZ_HD); tests/native/scalar_ops_test.cpp and scalar_scan_test.cpp compile it for the CPU.  Every
// loop over words is fully unrolled and every array index is a constant after unrolling: nothing here indexes a
// register array dynamically.
#pragma once
#include <cstdint>
#include "fp.h"

namespace msmz {

// r = a + b mod q.  a, b < q < 2^255: the plain sum fits 8 words.  r may alias a or b.
template <class Fr>
MSMZ_HD void fr_add(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  static_assert(Fr::BITS <= 255, "a + b must fit 8 words");
  uint32_t t[8], d[8];
  words_add<8>(t, a, b);
  const uint32_t borrow = words_sub<8>(d, t, Fr::Q);
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = borrow ? t[j] : d[j];
}

// r = a - b mod q.  r may alias a or b.
template <class Fr>
MSMZ_HD void fr_sub(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  uint32_t t[8], d[8];
  const uint32_t borrow = words_sub<8>(t, a, b);
  words_add<8>(d, t, Fr::Q);   // (mod 2^256: t = a - b + 2^256, so d = a - b + q)
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = borrow ? d[j] : t[j];
}

// r = a b 2^-256 mod q (CIOS: one row of a[i] * b, one reduction step, eight times).  With a, b < q the running value
// stays below 2 q, so one conditional subtraction ends below q; with a < q and ANY b < 2^256 it still ends below q
// (t < q + b q / 2^256 < 2 q), which is what a kernel relies on for a resident operand it has flagged as >= q.
// r may alias a or b.
template <class Fr>
MSMZ_HD void fr_mont_mul(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  uint32_t t[10];
#pragma unroll
  for (int j = 0; j < 10; j++) t[j] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t x = (uint64_t)a[i] * b[j] + t[j] + c;
      t[j] = (uint32_t)x;
      c = x >> 32;
    }
    uint64_t x = (uint64_t)t[8] + c;
    t[8] = (uint32_t)x;
    t[9] = (uint32_t)(x >> 32);
    const uint32_t m = t[0] * Fr::QINV32;
    c = ((uint64_t)m * Fr::Q[0] + t[0]) >> 32;   // (the low word is 0 by the choice of m)
#pragma unroll
    for (int j = 1; j < 8; j++) {
      const uint64_t y = (uint64_t)m * Fr::Q[j] + t[j] + c;
      t[j - 1] = (uint32_t)y;
      c = y >> 32;
    }
    x = (uint64_t)t[8] + c;
    t[7] = (uint32_t)x;
    t[8] = t[9] + (uint32_t)(x >> 32);
  }
  uint32_t d[8];
  const uint32_t borrow = words_sub<8>(d, t, Fr::Q);
  const bool keep = borrow && !t[8];
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = keep ? t[j] : d[j];
}

// a -> a 2^256 mod q, the form of a broadcast coefficient: fr_mont_mul(that, x) = a x, canonical, in ONE product
template <class Fr>
MSMZ_HD void fr_to_mont(uint32_t* r, const uint32_t* a) {
  fr_mont_mul<Fr>(r, a, Fr::R2);
}

// r = a b mod q: two Montgomery products, (a b 2^-256) (2^512) 2^-256
template <class Fr>
MSMZ_HD void fr_mul(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  uint32_t t[8];
  fr_mont_mul<Fr>(t, a, b);
  fr_mont_mul<Fr>(r, t, Fr::R2);
}

// ---------------------------------------------------------------------------------------------- inversion
// word w of q - 2, the exponent of Fermat's inversion: a constant of Fr (the borrow of "- 2" runs up from word 0)
template <class Fr>
MSMZ_HD constexpr uint32_t fr_qm2_word(int w) {
  uint32_t borrow = 2, r = 0;
  for (int j = 0; j <= w; j++) {
    r = Fr::Q[j] - borrow;
    borrow = Fr::Q[j] < borrow ? 1u : 0u;
  }
  return r;
}

// r = x^-1 mod q = x^(q - 2); 0 -> 0.  Operand canonical, result CANONICAL: x goes to Montgomery form (one product),
// 256 squarings and one product per set bit of q - 2 follow (about 380 products in all), and a product with the plain 1
// leaves Montgomery form.  The exponent is a constant of Fr (its words come from Fr::Q in constant memory, one per 32
// steps), so every lane of a kernel takes the same path whatever x is.  r may alias x.
template <class Fr>
MSMZ_HD void fr_inv(uint32_t* r, const uint32_t* x) {
  uint32_t xm[8], acc[8], one[8];
  fr_to_mont<Fr>(xm, x);
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = Fr::ONE[j], one[j] = j == 0 ? 1u : 0u;
#pragma unroll 1
  for (int w = 7; w >= 0; w--) {
    const uint32_t e = fr_qm2_word<Fr>(w);
#pragma unroll 1
    for (int k = 31; k >= 0; k--) {
      fr_mont_mul<Fr>(acc, acc, acc);
      if ((e >> k) & 1u) fr_mont_mul<Fr>(acc, acc, xm);
    }
  }
  fr_mont_mul<Fr>(r, acc, one);
}

// ---------------------------------------------------------------------------------------------- affine maps
// y -> A y + B over F_q, the element of a first-order linear recurrence (msmz_scalars_recurrence; scan_kernels.h).
// Forms: A is kept in MONTGOMERY form (A 2^256 mod q), B and every y are canonical.  Then
//     apply:    A (.) y = fr_mont_mul(A, y)   is canonical,                                        one product
//     compose:  A2 (.) A1                     is again in Montgomery form,  A2 (.) B1 is canonical: two products
// and no conversion ever happens between maps.  HA = false: A is 1 for every map in play (a running sum) and the field
// is neither read nor written; HB = false: B is 0 (a running product).
struct FrMap {
  uint32_t A[8];
  uint32_t B[8];
};

template <class Fr, bool HA, bool HB>
MSMZ_HD void fr_map_identity(FrMap& m) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (HA) m.A[j] = Fr::ONE[j];
    if (HB) m.B[j] = 0;
  }
}

// r = g o f, f applied first: (A_g, B_g) o (A_f, B_f) = (A_g A_f, A_g B_f + B_g).  r may alias g or f.
template <class Fr, bool HA, bool HB>
MSMZ_HD void fr_map_compose(FrMap& r, const FrMap& g, const FrMap& f) {
  if (HB) {
    uint32_t t[8];
    if (HA) {
      fr_mont_mul<Fr>(t, g.A, f.B);
      fr_add<Fr>(r.B, t, g.B);
    } else {
      fr_add<Fr>(r.B, f.B, g.B);
    }
  }
  if (HA) fr_mont_mul<Fr>(r.A, g.A, f.A);
}

// y = m(y) = A y + B
template <class Fr, bool HA, bool HB>
MSMZ_HD void fr_map_apply(uint32_t* y, const FrMap& m) {
  if (HA) fr_mont_mul<Fr>(y, m.A, y);
  if (HB) fr_add<Fr>(y, y, m.B);
}

// ---------------------------------------------------------------------------------------------- powers of one ratio
// msmz_scalars_powers: out_i = base ratio^i.  The table holds ratio^(2^k) 2^256 mod q, k < 32; a run of consecutive
// indices starts at base ratio^g, reached by one product per set bit of g, and goes on by one product with entry 0 per
// index.  The running value is canonical throughout (canonical times Montgomery form is canonical), so it is stored as
// it is.  The host builds the table (Engine::scalars_powers) and the kernel receives it as an argument.
constexpr int FR_POW_BITS = 32;   // indices below 2^32, as the entry count of a set

struct FrPowTable {
  uint32_t w[FR_POW_BITS][8];
};

template <class Fr>
MSMZ_HD void fr_pow_table(FrPowTable& t, const uint32_t* ratio) {
  fr_to_mont<Fr>(t.w[0], ratio);
  for (int k = 1; k < FR_POW_BITS; k++) fr_mont_mul<Fr>(t.w[k], t.w[k - 1], t.w[k - 1]);
}

// acc = base ratio^g, g < 2^32: at most 32 products.  `k` is the same in every lane of a kernel and indexes the table
// in memory (the kernel's argument segment), not a register array.
template <class Fr>
MSMZ_HD void fr_pow_start(uint32_t* acc, const uint32_t* base, const FrPowTable& t, uint32_t g) {
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = base[j];
#pragma unroll 1
  for (int k = 0; k < FR_POW_BITS; k++) {
    if ((g >> k) & 1u) fr_mont_mul<Fr>(acc, acc, t.w[k]);
  }
}

// acc = acc ratio: the step from one index to the next
template <class Fr>
MSMZ_HD void fr_pow_step(uint32_t* acc, const FrPowTable& t) {
  fr_mont_mul<Fr>(acc, acc, t.w[0]);
}

}  // namespace msmz

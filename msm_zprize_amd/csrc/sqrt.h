// Square roots in the base fields: what decompression of a point needs (curve.h `decompress`,
// import_kernels.h).  The job of the reference's src/field-sqrt.ts, restated so that every lane of a wave runs the same
// instructions: Tonelli-Shanks with the discrete logarithm taken by fixed C-bit digits (Bernstein, "Faster square roots
// in annoying finite fields"), never the textbook `while` loop whose trip count depends on the value.
//
// p - 1 = 2^S t, t odd; w = g^t generates the 2^S-th roots of unity (g a non-residue).  For a != 0:
//   u = a^((t-1)/2)            one fixed exponent: a sliding-window schedule from the generator, the same in every lane
//   r = u a,  v = u r = a^t    r^2 = v a, and v = w^e for one e in [0, 2^S)
//   e is odd  <=>  a is a non-residue;  otherwise  sqrt(a) = r w^(-e/2).
// The logarithm: N = ceil(S / C) digits.  e is kept as E = e << DELTA, DELTA = C N - S, so every digit E_i of E is C bits
// wide and the short digit (S is no multiple of C for 46 and 47) is the bottom one, its low DELTA bits zero.  With
// x_i = v^(2^(C (N-1-i))) (one chain of squarings from v) and zeta = w^(2^(S-C)), the primitive 2^C-th root,
//   x_i * prod_{j<i} INV[i-j][E_j] = zeta^(E_i),      INV[k][d] = w^-((d << C (N-1-k)) >> DELTA)
// -- the lower digits are peeled off with one table product each, N (N-1) / 2 in all -- and which power of zeta it is
// is read from the low word of its canonical residue (SQRT_KEY: 2^C distinct non-zero words, asserted by
// tools/gen_constants.py, so a match is an identification, not a hash hit).  The same table gives the last step:
//   w^(-e/2) = prod_j INV[N-1-j][H_j],   H = E >> 1.
// S = 1 (BLS12-381) is the same code with C = 1, N = 1: no squarings, no peeling, r = a^((p+1)/4) * 1.
// The x_i are kept in registers, so they are computed in two halves (digits [0, N/2), then [N/2, N)): half the
// registers for C (N - N/2) squarings run twice.  Product counts per field: F::SQRT_PRODUCTS (from these loop bounds).
//
// Host/device code (MSMZ_HD): tests/native/sqrt_test.cpp compiles this very template for the CPU.
#pragma once
#include <type_traits>
#include "fp.h"

namespace msmz {

// fn(integral_constant<int, I>) for I = BEGIN .. END-1, unrolled by the language: the register arrays below are indexed
// by constants whatever the optimizer thinks of a loop with loops inside
template <int BEGIN, int END, class Fn>
MSMZ_HD void static_for(Fn&& fn) {
  if constexpr (BEGIN < END) {
    fn(std::integral_constant<int, BEGIN>{});
    static_for<BEGIN + 1, END>(fn);
  }
}

template <class F>
MSMZ_HD void fe_select(Fe<F>& r, bool c, const Fe<F>& a, const Fe<F>& b) {   // r = c ? a : b
#pragma unroll
  for (int j = 0; j < F::N; j++) r.l[j] = c ? a.l[j] : b.l[j];
}

// u = a^((t-1)/2) by the schedule F::SQRT_SCHED over the odd powers a, a^3, a^5, a^7.  The schedule is a constant of
// the field: squaring counts and table picks are the same in every lane (scalar control flow).
template <class F>
MSMZ_HD void sqrt_pow(Fe<F>& u, const Fe<F>& a) {
  Fe<F> a2, a3, a5, a7, m, t;
  fe_sqr(a2, a);
  fe_mul(a3, a2, a);
  fe_mul(a5, a3, a2);
  fe_mul(a7, a5, a2);
  u = a;
#pragma unroll 1
  for (int s = 0; s < F::SQRT_SCHED_LEN; s++) {
    const int nsq = F::SQRT_SCHED[2 * s], idx = F::SQRT_SCHED[2 * s + 1];
    fe_select(m, (idx & 1) != 0, a3, a);
    fe_select(t, (idx & 1) != 0, a7, a5);
    fe_select(m, (idx & 2) != 0, t, m);
    if (s == 0) {   // the leading window starts the accumulator
      u = m;
      continue;
    }
#pragma unroll 1
    for (int k = 0; k < nsq; k++) {
      fe_sqr(t, u);
      u = t;
    }
    if (idx < 4) {
      fe_mul(t, u, m);
      u = t;
    }
  }
}

// which power of zeta is y?  false if none (cannot happen for y = a power of zeta; 0 matches nothing)
template <class F>
MSMZ_HD bool sqrt_digit(uint32_t& d, const Fe<F>& y) {
  uint32_t w[F::NW];
  fe_to_canon_words<F>(w, y);
  bool found = false;
  d = 0;
#pragma unroll
  for (uint32_t k = 0; k < (1u << F::SQRT_C); k++) {
    const bool hit = w[0] == F::SQRT_KEY[k];
    d = hit ? k : d;
    found = found || hit;
  }
  return found;
}

// digits [LO, HI) of E, given the digits below LO
template <class F, int LO, int HI>
MSMZ_HD bool sqrt_dlog_range(uint64_t& E, const Fe<F>& v) {
  constexpr int C = F::SQRT_C, N = F::SQRT_N;
  bool ok = true;
  if constexpr (HI > LO) {
    Fe<F> xs[HI - LO], y, t;
    y = v;
#pragma unroll 1
    for (int k = 0; k < C * (N - HI); k++) {
      fe_sqr(t, y);
      y = t;
    }
    xs[HI - 1 - LO] = y;   // x_(HI-1) = v^(2^(C (N-HI)))
    static_for<0, HI - 1 - LO>([&](auto K) {   // x_i = x_(i+1)^(2^C), i = HI-2 .. LO
#pragma unroll 1
      for (int k = 0; k < C; k++) {
        fe_sqr(t, y);
        y = t;
      }
      xs[HI - 2 - LO - decltype(K)::value] = y;
    });
    static_for<LO, HI>([&](auto I) {
      constexpr int i = decltype(I)::value;
      y = xs[i - LO];
#pragma unroll 1
      for (int j = 0; j < i; j++) {
        const uint32_t d = (uint32_t)(E >> (C * j)) & ((1u << C) - 1u);
        Fe<F> f;
        fe_set_const<F>(f, F::SQRT_INV[((i - j) << C) + d]);
        fe_mul(t, y, f);
        y = t;
      }
      uint32_t d;
      ok = sqrt_digit<F>(d, y) && ok;
      E |= (uint64_t)d << (C * i);
    });
  }
  return ok;
}

// r = a square root of the Montgomery residue a (any lazy value a product takes), as a product output; false when a is
// a non-residue (r is then unspecified).  a = 0 gives 0.  Which of the two roots comes back is not specified: callers
// that care pick by sign (curve.h fe_choose_root).
template <class F>
MSMZ_HD bool fe_sqrt(Fe<F>& r, const Fe<F>& a) {
  constexpr int C = F::SQRT_C, N = F::SQRT_N;
  static_assert(C * N - F::SQRT_S == F::SQRT_DELTA && C * N <= 64, "the shifted logarithm fits 64 bits");
  Fe<F> u, v, t;
  sqrt_pow<F>(u, a);
  fe_mul(r, u, a);   // a^((t+1)/2)
  fe_mul(v, u, r);   // a^t
  uint64_t E = 0;
  bool ok = sqrt_dlog_range<F, 0, N / 2>(E, v);
  ok = sqrt_dlog_range<F, N / 2, N>(E, v) && ok;
  if ((E >> F::SQRT_DELTA) & 1u) ok = false;   // e odd: a non-residue
  const uint64_t H = E >> 1;
#pragma unroll 1
  for (int j = 0; j < N; j++) {
    const uint32_t d = (uint32_t)(H >> (C * j)) & ((1u << C) - 1u);
    Fe<F> f;
    fe_set_const<F>(f, F::SQRT_INV[((N - 1 - j) << C) + d]);
    fe_mul(t, r, f);
    r = t;
  }
  if (fe_is_zero_mod_p<F>(a)) {   // a = 0: v = 0 is no root of unity; the root is 0 (r = u a already is)
    fe_zero(r);
    return true;
  }
  return ok;
}

}  // namespace msmz

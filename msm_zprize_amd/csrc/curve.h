// Curve arithmetic for the MSM kernels and the host-side final sums.
//
// Short Weierstrass, a = 0 (BLS12-377 / BLS12-381 G1, Pallas):
//   * affine points in memory: [x | y], 2*NW words, lazy Montgomery residues in [0,3p);
//     the point at infinity is the all-zero record (x = y = 0 is never on y^2 = x^3 + b, b != 0).
//     (The reference keeps a separate isNonZero flag word: src/curve-affine.ts:20-52.)
//   * affine addition given the inverse of the x-difference -- the core of the batched-affine
//     accumulation (src/wasm/curve.ts:32-58 `addAffine`, src/curve-affine.ts:90-109 `double`).
//   * extended Jacobian "XYZZ" accumulators (X, Y, ZZ, ZZZ), x = X/ZZ, y = Y/ZZZ, for the bucket /
//     window reduction.  The reference uses homogeneous projective coordinates there
//     (src/curve-projective.ts:51-253, EFD add-1998-cmo-2 / dbl-1998-cmo-2); XYZZ (EFD
//     madd-2008-s / add-2008-s / dbl-2008-s-1) does the same job with 10M mixed / 14M full
//     additions.  Infinity is ZZ = 0.  All edge cases (infinity operands, equal points,
//     opposite points) are handled like the reference's `addOrSubtract` (curve-projective.ts:51-160).
//
// Twisted Edwards a = -1 (ed-on-bls12-377): extended coordinates, unified addition
// (src/curve-twisted-edwards.ts:84-165, EFD add-2008-hwcd-3 with k = 2d).
#pragma once
#include "fp.h"
#include "sqrt.h"

namespace msmz {

// ------------------------------------------------------------------------------------------------
// value in [0,3p) with normalized limbs (straight from fe_unpack / fe_reduce_small): is it 0 mod p ?
template <class F>
MSMZ_HD bool fe_reduced_is_zero(const Fe<F>& r) {
  int32_t d0 = 0, d1 = 0, d2 = 0;
#pragma unroll
  for (int j = 0; j < F::N; j++) {
    d0 |= r.l[j];
    d1 |= r.l[j] ^ F::PL[j];
    d2 |= r.l[j] ^ F::P2[j];
  }
  return d0 == 0 || d1 == 0 || d2 == 0;
}

// lazy value (|v| < 2^4 p) == 0 mod p ?
// Quick exact filter first: v = 0 mod p with |v| < 16 p means v = k p, |k| <= 15, and p = 1 mod 2^W, so the low W bits
// of v (= of limb 0: lazy limbs carry nothing INTO limb 0) are k mod 2^W.  Anything else is non-zero -- which is every
// value but ~2^-23 of them, so the full reduction below practically never runs.
template <class F>
MSMZ_HD bool fe_is_zero(const Fe<F>& a) {
  if constexpr (F::PL[0] == 1) {
    constexpr uint32_t MASK = (1u << F::W) - 1u;
    if ((((uint32_t)a.l[0] + 15u) & MASK) > 30u) return false;
  }
  Fe<F> t = a;
  fe_reduce_small(t);
  return fe_reduced_is_zero(t);
}

// ------------------------------------------------------------------------------------------------ affine
template <class F>
struct Affine {
  Fe<F> x, y;
};

template <class F>
MSMZ_HD bool words_point_is_inf(const uint32_t* w) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 2 * F::NW; i++) o |= w[i];
  return o == 0;
}

// (x3, y3) = (x1, y1) + (x2, y2) given inv = 1/(x2 - x1)        [2M + 1S]
//   m = (y2 - y1) * inv ; x3 = m^2 - x1 - x2 ; y3 = m (x1 - x3) - y1      (wasm/curve.ts:44-56)
template <class F>
MSMZ_HD void affine_add_with_inv(Affine<F>& r, const Affine<F>& p1, const Affine<F>& p2, const Fe<F>& inv) {
  Fe<F> dy, m, mm, t;
  fe_sub(dy, p2.y, p1.y);
  fe_mul(m, dy, inv);
  fe_sqr(mm, m);
  fe_sub(t, mm, p1.x);
  fe_sub(r.x, t, p2.x);          // x3: limbs within 3 * 2^W
  fe_sub(t, p1.x, r.x);          // x1 - x3: limbs within 4 * 2^W -> one parallel carry keeps the bound
  fe_carry(t);
  fe_mul(mm, m, t);
  fe_sub(r.y, mm, p1.y);
}

// (x3, y3) = 2 (x1, y1) given inv = 1/(2 y1)                    [2M + 2S]
//   m = 3 x1^2 * inv ; x3 = m^2 - 2 x1 ; y3 = m (x1 - x3) - y1             (curve-affine.ts:90-109)
template <class F>
MSMZ_HD void affine_double_with_inv(Affine<F>& r, const Affine<F>& p1, const Fe<F>& inv) {
  Fe<F> xx, x3, m, mm, t;
  fe_sqr(xx, p1.x);
  fe_add(x3, xx, xx);
  fe_add(x3, x3, xx);            // 3 x^2, limbs within 3 * 2^W
  fe_carry(x3);
  fe_mul(m, x3, inv);
  fe_sqr(mm, m);
  fe_sub(t, mm, p1.x);
  fe_sub(r.x, t, p1.x);
  fe_sub(t, p1.x, r.x);
  fe_carry(t);
  fe_mul(mm, m, t);
  fe_sub(r.y, mm, p1.y);
}

// ------------------------------------------------------------------------------------------------ XYZZ
template <class F>
struct Xyzz {
  Fe<F> X, Y, ZZ, ZZZ;
};

template <class F>
MSMZ_HD void xyzz_set_inf(Xyzz<F>& p) {
  fe_set_const<F>(p.X, F::ONE);
  fe_set_const<F>(p.Y, F::ONE);
  fe_zero(p.ZZ);
  fe_zero(p.ZZZ);
}

template <class F>
MSMZ_HD bool xyzz_is_inf(const Xyzz<F>& p) {
  return fe_is_zero(p.ZZ);
}

template <class F>
MSMZ_HD void xyzz_from_affine(Xyzz<F>& r, const Affine<F>& a) {
  r.X = a.x;
  r.Y = a.y;
  fe_set_const<F>(r.ZZ, F::ONE);
  fe_set_const<F>(r.ZZZ, F::ONE);
}

// keep the coordinates' limbs near-normalized after a chain of lazy adds
template <class F>
MSMZ_HD void xyzz_carry(Xyzz<F>& p) {
  fe_carry(p.X);
  fe_carry(p.Y);
}

// r = 2 * (x, y) for an affine input (EFD mdbl-2008-s-1, a = 0)
template <class F>
MSMZ_HD void xyzz_mdbl(Xyzz<F>& r, const Affine<F>& a) {
  Fe<F> U, V, W, S, M, t;
  fe_add(U, a.y, a.y);
  fe_carry(U);   // 2y has limbs up to 2^(W+1): 9 * 2^60 breaks N*A*B < 2^63 for the 255-bit fields
  fe_sqr(V, U);
  fe_mul(W, U, V);
  fe_mul(S, a.x, V);
  fe_sqr(t, a.x);
  fe_add(M, t, t);
  fe_add(M, M, t);
  fe_carry(M);
  fe_sqr(t, M);
  fe_sub(t, t, S);
  fe_sub(r.X, t, S);
  fe_sub(t, S, r.X);
  fe_carry(t);
  fe_mul(S, M, t);
  fe_mul(t, W, a.y);
  fe_sub(r.Y, S, t);
  r.ZZ = V;
  r.ZZZ = W;
  xyzz_carry(r);
}

// r = 2 * p (EFD dbl-2008-s-1, a = 0)                                  [6M + 3S]
template <class F>
MSMZ_HD void xyzz_dbl(Xyzz<F>& r, const Xyzz<F>& p) {
  if (xyzz_is_inf(p)) {
    r = p;
    return;
  }
  Fe<F> U, V, W, S, M, t, zz, zzz;
  fe_add(U, p.Y, p.Y);
  fe_carry(U);
  fe_sqr(V, U);
  fe_mul(W, U, V);
  fe_mul(S, p.X, V);
  fe_sqr(t, p.X);
  fe_add(M, t, t);
  fe_add(M, M, t);
  fe_carry(M);
  fe_mul(zz, V, p.ZZ);
  fe_mul(zzz, W, p.ZZZ);
  fe_sqr(t, M);
  fe_sub(t, t, S);
  fe_sub(r.X, t, S);
  fe_sub(t, S, r.X);
  fe_carry(t);
  fe_mul(S, M, t);
  fe_mul(t, W, p.Y);
  fe_sub(r.Y, S, t);
  r.ZZ = zz;
  r.ZZZ = zzz;
  xyzz_carry(r);
}

// r = p + (x2, y2)  -- mixed addition (EFD madd-2008-s)                 [8M + 2S]
// `a_inf`: the affine operand is the point at infinity.
template <class F>
MSMZ_HD void xyzz_madd(Xyzz<F>& r, const Xyzz<F>& p, const Affine<F>& a, bool a_inf) {
  if (a_inf) {
    r = p;
    return;
  }
  if (xyzz_is_inf(p)) {
    xyzz_from_affine(r, a);
    return;
  }
  Fe<F> U2, S2, P, R, PP, PPP, Q, t, u;
  fe_mul(U2, a.x, p.ZZ);
  fe_mul(S2, a.y, p.ZZZ);
  fe_sub(P, U2, p.X);
  fe_sub(R, S2, p.Y);
  fe_carry(P);
  fe_carry(R);
  if (fe_is_zero(P)) {
    if (fe_is_zero(R)) {
      xyzz_mdbl(r, a);
    } else {
      xyzz_set_inf(r);
    }
    return;
  }
  fe_sqr(PP, P);
  fe_mul(PPP, P, PP);
  fe_mul(Q, p.X, PP);
  fe_sqr(t, R);
  fe_sub(t, t, PPP);
  fe_sub(t, t, Q);
  fe_sub(u, t, Q);       // X3 = R^2 - PPP - 2Q
  fe_carry(u);
  fe_sub(t, Q, u);
  fe_carry(t);
  fe_mul(Q, R, t);       // R (Q - X3)
  fe_mul(t, p.Y, PPP);
  fe_sub(r.Y, Q, t);
  r.X = u;
  fe_mul(t, p.ZZ, PP);
  fe_mul(u, p.ZZZ, PPP);
  r.ZZ = t;
  r.ZZZ = u;
  fe_carry(r.Y);
}

// r = p + q (EFD add-2008-s) with the reference's edge-case handling   [12M + 2S]
template <class F>
MSMZ_HD void xyzz_add(Xyzz<F>& r, const Xyzz<F>& p, const Xyzz<F>& q) {
  if (xyzz_is_inf(p)) {
    r = q;
    return;
  }
  if (xyzz_is_inf(q)) {
    r = p;
    return;
  }
  Fe<F> U1, U2, S1, S2, P, R, PP, PPP, Q, t, u;
  fe_mul(U1, p.X, q.ZZ);
  fe_mul(U2, q.X, p.ZZ);
  fe_mul(S1, p.Y, q.ZZZ);
  fe_mul(S2, q.Y, p.ZZZ);
  fe_sub(P, U2, U1);
  fe_sub(R, S2, S1);
  if (fe_is_zero(P)) {
    if (fe_is_zero(R)) {
      xyzz_dbl(r, p);
    } else {
      xyzz_set_inf(r);
    }
    return;
  }
  fe_sqr(PP, P);
  fe_mul(PPP, P, PP);
  fe_mul(Q, U1, PP);
  fe_sqr(t, R);
  fe_sub(t, t, PPP);
  fe_sub(t, t, Q);
  fe_sub(u, t, Q);       // X3
  fe_carry(u);
  fe_sub(t, Q, u);
  fe_carry(t);
  fe_mul(Q, R, t);
  fe_mul(t, S1, PPP);
  fe_sub(r.Y, Q, t);
  r.X = u;
  fe_mul(t, p.ZZ, q.ZZ);
  fe_mul(u, t, PP);
  fe_mul(t, p.ZZZ, q.ZZZ);
  fe_mul(Q, t, PPP);
  r.ZZ = u;
  r.ZZZ = Q;
  fe_carry(r.Y);
}

template <class F>
MSMZ_HD void xyzz_neg(Xyzz<F>& p) {
  fe_neg(p.Y, p.Y);
}

// XYZZ -> canonical affine words (x | y); returns true for infinity (words zeroed).
// (curve-projective.ts:335-349 `toAffine` + curve-affine.ts:220-233 `toBigint`)
template <class F>
MSMZ_HD bool xyzz_to_affine_canon(uint32_t* w, const Xyzz<F>& p) {
  constexpr int NW = F::NW;
  if (xyzz_is_inf(p)) {
#pragma unroll
    for (int i = 0; i < 2 * NW; i++) w[i] = 0;
    return true;
  }
  Fe<F> zi, zi2, zi3, x, y, t;
  fe_inverse(zi3, p.ZZZ);        // 1/ZZZ
  fe_mul(t, zi3, p.ZZ);          // 1/Z   (ZZ/ZZZ = 1/Z)
  fe_sqr(zi2, t);                // 1/ZZ
  fe_mul(x, p.X, zi2);
  fe_mul(y, p.Y, zi3);
  fe_from_mont(t, x);
  fe_to_canon_words<F>(w, t);
  fe_from_mont(t, y);
  fe_to_canon_words<F>(w + NW, t);
  (void)zi;
  return false;
}

// ------------------------------------------------------------------------------------------------ twisted Edwards
template <class F>
struct TeExt {
  Fe<F> X, Y, Z, T;
};

// "Niels" form of an affine input: (y - x, y + x, 2d*x*y) -- lets the mixed addition skip 2 products.
template <class F>
struct TeNiels {
  Fe<F> ym, yp, kt;
};

template <class F>
MSMZ_HD void te_set_zero(TeExt<F>& p) {
  fe_zero(p.X);
  fe_set_const<F>(p.Y, F::ONE);
  fe_set_const<F>(p.Z, F::ONE);
  fe_zero(p.T);
}

// r = p + q, unified (curve-twisted-edwards.ts:84-165; bigint/twisted-edwards.ts:52-85)   [9M]
template <class F>
MSMZ_HD void te_add(TeExt<F>& r, const TeExt<F>& p, const TeExt<F>& q) {
  Fe<F> A, B, C, D, E, Fv, G, H, t, u, k;
  fe_sub(t, p.Y, p.X);
  fe_sub(u, q.Y, q.X);
  fe_carry(t);
  fe_carry(u);
  fe_mul(A, t, u);
  fe_add(t, p.Y, p.X);
  fe_add(u, q.Y, q.X);
  fe_carry(t);
  fe_carry(u);
  fe_mul(B, t, u);
  fe_mul(t, p.T, q.T);
  fe_set_const<F>(k, F::K2D);
  fe_mul(C, t, k);
  fe_mul(D, p.Z, q.Z);
  fe_add(D, D, D);
  fe_sub(E, B, A);
  fe_sub(Fv, D, C);
  fe_add(G, D, C);
  fe_add(H, B, A);
  fe_carry(E);
  fe_carry(Fv);
  fe_carry(G);
  fe_carry(H);
  fe_mul(r.X, E, Fv);
  fe_mul(r.Y, G, H);
  fe_mul(r.T, E, H);
  fe_mul(r.Z, Fv, G);
}

// r = p + (+-)n for a Niels-form affine input (negation swaps ym/yp and flips kt)        [7M]
template <class F>
MSMZ_HD void te_madd(TeExt<F>& r, const TeExt<F>& p, const TeNiels<F>& n, uint32_t neg) {
  Fe<F> A, B, C, D, E, Fv, G, H, t, ym, yp, kt;
  int32_t m = -(int32_t)(neg & 1u);
#pragma unroll
  for (int j = 0; j < F::N; j++) {
    ym.l[j] = (n.ym.l[j] & ~m) | (n.yp.l[j] & m);
    yp.l[j] = (n.yp.l[j] & ~m) | (n.ym.l[j] & m);
  }
  fe_cneg(kt, n.kt, neg);
  fe_sub(t, p.Y, p.X);
  fe_carry(t);
  fe_mul(A, t, ym);
  fe_add(t, p.Y, p.X);
  fe_carry(t);
  fe_mul(B, t, yp);
  fe_mul(C, p.T, kt);
  fe_add(D, p.Z, p.Z);
  fe_sub(E, B, A);
  fe_sub(Fv, D, C);
  fe_add(G, D, C);
  fe_add(H, B, A);
  fe_carry(E);
  fe_carry(Fv);
  fe_carry(G);
  fe_carry(H);
  fe_mul(r.X, E, Fv);
  fe_mul(r.Y, G, H);
  fe_mul(r.T, E, H);
  fe_mul(r.Z, Fv, G);
}

// extended -> canonical affine words (x | y)   (bigint/twisted-edwards.ts:39-45)
template <class F>
MSMZ_HD void te_to_affine_canon(uint32_t* w, const TeExt<F>& p) {
  Fe<F> zi, x, y, t;
  fe_inverse(zi, p.Z);
  fe_mul(x, p.X, zi);
  fe_mul(y, p.Y, zi);
  fe_from_mont(t, x);
  fe_to_canon_words<F>(w, t);
  fe_from_mont(t, y);
  fe_to_canon_words<F>(w + F::NW, t);
}

// ------------------------------------------------------------------------------------------------ curve equations
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

// ------------------------------------------------------------------------------------------------ compressed points
// A compressed record is one coordinate (the "wire" coordinate: x on the Weierstrass curves, y on the twisted Edwards
// curve) plus the sign of the other.  Two conventions for the sign of a canonical value c in [0, p):
//   largest (parity = 0)  sign = 1 iff c > (p - 1) / 2
//   parity  (parity = 1)  sign = 1 iff c is odd
// Of the two roots c and p - c exactly one has either sign (p is odd), except for c = 0, whose only sign is 0.
constexpr int DECOMPRESS_OK = 0, DECOMPRESS_NOT_A_POINT = 1;

// the sign of the Montgomery residue m under the convention; *zero: the value is 0                               [1M]
template <class F>
MSMZ_HD bool fe_wire_sign(bool* zero, const Fe<F>& m, int parity) {
  Fe<F> t;
  uint32_t w[F::NW];
  fe_from_mont(t, m);
  fe_to_canon_words<F>(w, t);
  *zero = words_is_zero<F::NW>(w);
  return parity ? (w[0] & 1u) != 0 : words_geq<F::NW>(w, F::PHALF1);
}

// r <- the one of r, -r whose sign is `sign`; a sign bit on the root 0 is refused (encodings are unique)
template <class F>
MSMZ_HD int fe_choose_root(Fe<F>& r, bool sign, int parity) {
  bool zero;
  const bool have = fe_wire_sign<F>(&zero, r, parity);
  if (zero) return sign ? DECOMPRESS_NOT_A_POINT : DECOMPRESS_OK;
  if (have != sign) fe_neg(r, r);
  return DECOMPRESS_OK;
}

// ------------------------------------------------------------------------------------------------ the group, once
// What the two curve forms share, under one static interface, host and device: code that walks a scalar, checks a
// point or builds a table is written once over a group G.  Every member forwards to the formulas above.
//   Acc    the accumulator: XYZZ / extended coordinates
//   Base   a point as the mixed addition takes it: affine + infinity flag / Niels form
// x and y arguments are lazy Montgomery residues.  `denominator` is what one inversion turns into affine coordinates
// (affine_from_inverse); to_affine_canon returns true for the point at infinity (Weierstrass only).
template <class F_>
struct WeierGroup {
  using F = F_;
  using Acc = Xyzz<F>;
  struct Base {
    Affine<F> a;
    bool inf;
  };
  static constexpr bool TE = false;
  static MSMZ_HD void set_identity(Acc& p) { xyzz_set_inf(p); }
  static MSMZ_HD bool is_identity(const Acc& p) { return xyzz_is_inf(p); }
  static MSMZ_HD void dbl(Acc& r, const Acc& p) { xyzz_dbl(r, p); }
  static MSMZ_HD void add(Acc& r, const Acc& p, const Acc& q) { xyzz_add(r, p, q); }
  static MSMZ_HD void madd(Acc& r, const Acc& p, const Base& b) { xyzz_madd(r, p, b.a, b.inf); }
  // p + the finite affine point (x, y)
  static MSMZ_HD void add_affine(Acc& r, const Acc& p, const Fe<F>& x, const Fe<F>& y) {
    xyzz_madd(r, p, Affine<F>{x, y}, false);
  }
  static MSMZ_HD void from_affine(Acc& p, const Fe<F>& x, const Fe<F>& y) { xyzz_from_affine(p, Affine<F>{x, y}); }
  static MSMZ_HD void base_from_affine(Base& b, const Fe<F>& x, const Fe<F>& y, bool inf) { b = Base{{x, y}, inf}; }
  static MSMZ_HD bool on_curve(const Fe<F>& x, const Fe<F>& y) { return weier_on_curve(Affine<F>{x, y}); }
  // (x, y) from the wire coordinate x (a Montgomery residue) and the sign of y: y^2 = x^3 + b   [1M + 1S + fe_sqrt + 1M]
  static MSMZ_HD int decompress(Fe<F>& x, Fe<F>& y, const Fe<F>& wire, bool sign, int parity) {
    Fe<F> xx, rhs, b;
    x = wire;
    fe_sqr(xx, x);
    fe_mul(rhs, xx, x);
    fe_set_const<F>(b, F::B);
    fe_add(rhs, rhs, b);
    fe_carry(rhs);
    if (!fe_sqrt<F>(y, rhs)) return DECOMPRESS_NOT_A_POINT;
    return fe_choose_root<F>(y, sign, parity);
  }
  static MSMZ_HD const Fe<F>& denominator(const Acc& p) { return p.ZZZ; }
  static MSMZ_HD void affine_from_inverse(Fe<F>& x, Fe<F>& y, const Acc& p, const Fe<F>& zi3) {
    Fe<F> t, zi2;
    fe_mul(t, zi3, p.ZZ);   // 1 / Z   (ZZ / ZZZ = 1 / Z)
    fe_sqr(zi2, t);         // 1 / ZZ
    fe_mul(x, p.X, zi2);
    fe_mul(y, p.Y, zi3);
  }
  static MSMZ_HD bool to_affine_canon(uint32_t* w, const Acc& p) { return xyzz_to_affine_canon<F>(w, p); }
};

// The identity is the affine point (0, 1): there is no infinity flag, and `inf` arguments are not read.  The doubling is
// the unified te_add(p, p): a = -1 is a square mod p and d is not, so the addition law has no exceptional pair on this
// curve (Hisil-Wong-Carter-Dawson 2008, section 3) -- the 2- and 4-torsion points included -- and Z never vanishes.
template <class F_>
struct TeGroup {
  using F = F_;
  using Acc = TeExt<F>;
  using Base = TeNiels<F>;
  static constexpr bool TE = true;
  static MSMZ_HD void set_identity(Acc& p) { te_set_zero(p); }
  static MSMZ_HD bool is_identity(const Acc& p) {
    Fe<F> d;
    fe_sub(d, p.Y, p.Z);
    fe_carry(d);
    return fe_is_zero(p.X) && fe_is_zero(d);   // X = 0 alone also holds for (0, -1): the identity has Y = Z
  }
  static MSMZ_HD void dbl(Acc& r, const Acc& p) { te_add(r, p, p); }
  static MSMZ_HD void add(Acc& r, const Acc& p, const Acc& q) { te_add(r, p, q); }
  static MSMZ_HD void madd(Acc& r, const Acc& p, const Base& b) { te_madd(r, p, b, 0); }
  static MSMZ_HD void add_affine(Acc& r, const Acc& p, const Fe<F>& x, const Fe<F>& y) {
    Acc q;
    from_affine(q, x, y);
    te_add(r, p, q);
  }
  static MSMZ_HD void from_affine(Acc& p, const Fe<F>& x, const Fe<F>& y) {
    p.X = x;
    p.Y = y;
    fe_set_const<F>(p.Z, F::ONE);
    fe_mul(p.T, x, y);
  }
  // the Niels form (y - x, y + x, 2d x y) that the resident records hold
  static MSMZ_HD void base_from_affine(Base& b, const Fe<F>& x, const Fe<F>& y, bool /*inf*/) {
    Fe<F> t, k;
    fe_sub(b.ym, y, x);
    fe_add(b.yp, y, x);
    fe_mul(t, x, y);
    fe_set_const<F>(k, F::K2D);
    fe_mul(b.kt, t, k);
  }
  static MSMZ_HD bool on_curve(const Fe<F>& x, const Fe<F>& y) {
    Fe<F> yc = y;   // (y = (y - x) + x of a record: two lazy values added)
    fe_carry(yc);
    return te_on_curve<F>(x, yc);
  }
  // (x, y) from the wire coordinate y and the sign of x: x^2 = (y^2 - 1) / (d y^2 + 1).  The denominator is never zero:
  // -1 / d is a non-residue (d is one, -1 is not; asserted by tools/gen_constants.py).  [2M + 1S + fe_inverse + fe_sqrt + 1M]
  static MSMZ_HD int decompress(Fe<F>& x, Fe<F>& y, const Fe<F>& wire, bool sign, int parity) {
    Fe<F> yy, one, d, num, den, inv, q;
    y = wire;
    fe_sqr(yy, y);
    fe_set_const<F>(one, F::ONE);
    fe_set_const<F>(d, F::D);
    fe_sub(num, yy, one);
    fe_mul(den, yy, d);
    fe_add(den, den, one);
    fe_carry(num);
    fe_carry(den);
    if (!fe_inverse<F>(inv, den)) return DECOMPRESS_NOT_A_POINT;
    fe_mul(q, num, inv);
    if (!fe_sqrt<F>(x, q)) return DECOMPRESS_NOT_A_POINT;
    return fe_choose_root<F>(x, sign, parity);
  }
  static MSMZ_HD const Fe<F>& denominator(const Acc& p) { return p.Z; }
  static MSMZ_HD void affine_from_inverse(Fe<F>& x, Fe<F>& y, const Acc& p, const Fe<F>& zi) {
    fe_mul(x, p.X, zi);
    fe_mul(y, p.Y, zi);
  }
  static MSMZ_HD bool to_affine_canon(uint32_t* w, const Acc& p) {
    te_to_affine_canon<F>(w, p);
    return false;
  }
};

}  // namespace msmz

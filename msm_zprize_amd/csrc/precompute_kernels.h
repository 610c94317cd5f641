// Fixed-base precomputation of a resident point set (msmz_precompute_points).  Included by kernels.h.
//
// Copy j of a precomputed set holds 2^(c j) P_i for every point P_i; one launch of k_precompute_copy makes copy j from
// copy j - 1: c doublings in XYZZ from the affine record (one mixed doubling, c - 1 general ones), then back to affine.
// The affine conversion needs 1 / ZZZ per point; the 64 of a wave are inverted together (Montgomery's trick across the
// lanes: exclusive prefix and suffix products by shuffles, ONE fe_inverse_wave of the wave's total product), so a point
// costs c doublings + ~17 field products instead of a field inversion.  Points at infinity (all-zero records) and points
// whose multiple is the identity stay all-zero records.  With `endo` the copy's records [n, 2n) get (beta x, y).
#pragma once

namespace msmz {

template <class F>
__device__ __forceinline__ void fe_shfl_up(Fe<F>& r, const Fe<F>& a, int d) {
#pragma unroll
  for (int j = 0; j < F::N; j++) r.l[j] = __shfl_up(a.l[j], d, 64);
}
template <class F>
__device__ __forceinline__ void fe_shfl_down(Fe<F>& r, const Fe<F>& a, int d) {
#pragma unroll
  for (int j = 0; j < F::N; j++) r.l[j] = __shfl_down(a.l[j], d, 64);
}

// out: copy j (records [0, n) and, with endo, [n, 2n)); in: copy j - 1 (records [0, n) are read).  Whole waves stay
// alive to the end: fe_inverse_wave spreads one value over the lanes of a wave.
template <class F>
__global__ void __launch_bounds__(256) k_precompute_copy(uint32_t* out, const uint32_t* in, uint32_t n, int c, int endo) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  bool inf = true;
  Xyzz<F> p;
  xyzz_set_inf(p);
  if (i < n) {
    Affine<F> a;
    inf = load_affine<F>(a, in + (size_t)i * PointFmt<F>::STRIDE, 0);
    if (!inf) {
      xyzz_mdbl(p, a);
      for (int s = 1; s < c; s++) {
        Xyzz<F> t;
        xyzz_dbl(t, p);
        p = t;
      }
      inf = fe_is_zero_mod_p(p.ZZZ);   // (a point of small order)
    }
  }
  Fe<F> d;
  if (inf) fe_set_const<F>(d, F::ONE); else d = p.ZZZ;
  // exclusive prefix (pre) and suffix (suf) products of the lanes' denominators; total = product of all 64
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
  suf = t;   // now exclusive: product of the lanes above
#pragma unroll
  for (int j = 0; j < F::N; j++) total.l[j] = __shfl(inc.l[j], 63, 64);
  fe_inverse_wave(inv, total);   // (never zero: the identity's denominators were replaced by one)
  if (i >= n) return;
  Affine<F> m;
  fe_zero(m.x);
  fe_zero(m.y);
  if (!inf) {
    Fe<F> zi3, zi2;
    fe_mul(t, inv, pre);
    fe_mul(zi3, t, suf);          // 1 / ZZZ
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

}  // namespace msmz

// Sequential and inverse arithmetic over resident scalar sets (msmz_scalars_recurrence / _inverse, include/msmz.h;
// DESIGN.md section 19):
//     recurrence:  y_i = a_i y_(i-1) + b_i     a: absent (1), one broadcast scalar, or a resident vector; b: absent or resident
//     inverse:     out_i = x_i^-1, 0 -> 0
// all mod q, on the 8-word canonical records of a scalar set, with the F_q functions and the affine maps of fr.h.
//
// The recurrence is a scan of affine maps in THREE launches, none of which waits on another workgroup:
//   k_scalars_rec_tile   one workgroup per tile of SREC_TILE consecutive scan positions -> the tile's aggregate map
//   k_scalars_rec_carry  ONE workgroup: the aggregates, SREC_PASS per pass of its loop -> every tile's incoming value
//   k_scalars_rec_apply  the tiling of the first launch: every thread's incoming value, then its run of y_i
// The inverse is Montgomery's trick with ONE fr_inv per wave chunk of SINV_CHUNK elements.
//
// The first part of this file is host/device code: the geometry and the per-thread bodies, which
// tests/native/scalar_scan_test.cpp runs on the CPU.  The kernels follow, for the device compiler only.
#pragma once
#include "scalar_kernels.h"

namespace msmz {

constexpr int SREC_THREADS = 256;
constexpr int SREC_E = 8;                          // consecutive scan positions one thread owns (its run)
constexpr int SREC_TILE = SREC_THREADS * SREC_E;   // ... and one workgroup
constexpr int SREC_PASS = SREC_THREADS;            // tile aggregates the carry kernel takes per pass
constexpr int SINV_THREADS = 256;
constexpr int SINV_E = 8;                          // consecutive elements one thread inverts
constexpr int SINV_CHUNK = 64 * SINV_E;            // ... and one wave: the share of ONE fr_inv

// how the multiplier of a recurrence arrives (a template parameter of the kernels: a mode pays for what it uses)
enum { SREC_A_NONE = 0, SREC_A_BROADCAST = 1, SREC_A_RESIDENT = 2 };
// the flag bits of msmz_scalar_rec
constexpr uint32_t SREC_REVERSE = 1, SREC_EXCLUSIVE = 2;

// record i of a scalar set -> s; true if it is >= q.  (Plain word copies behind a 16-byte alignment promise: the device
// compiler makes two 16-byte loads of them, as fr_load of scalar_kernels.h spells out.)
template <class Fr>
MSMZ_HD bool sscan_load(uint32_t* s, const uint32_t* set, uint64_t i) {
  const uint32_t* p = static_cast<const uint32_t*>(__builtin_assume_aligned(set + i * 8, 16));
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = p[j];
  return words_geq<8>(s, Fr::Q);
}

MSMZ_HD void sscan_store(uint32_t* set, uint64_t i, const uint32_t* s) {
  uint32_t* p = static_cast<uint32_t*>(__builtin_assume_aligned(set + i * 8, 16));
#pragma unroll
  for (int j = 0; j < 8; j++) p[j] = s[j];
}

// Scan position p of a recurrence over n entries is entry p of the ranges, or entry n - 1 - p with REVERSE: the mirror
// is all that a reverse recurrence needs.
MSMZ_HD uint64_t srec_entry(uint64_t p, uint64_t n, bool reverse) { return reverse ? n - 1 - p : p; }

// The element at entry i: its multiplier in Montgomery form -> am (resident multipliers only: ONE product; a broadcast
// multiplier arrives converted, in `k`), its addend -> bv.  -> the multiplier to use; *bad |= a record >= q.
template <class Fr, int AM, bool HB>
MSMZ_HD const uint32_t* srec_element(uint32_t* am, uint32_t* bv, const uint32_t* a, const uint32_t* b, const uint32_t* k,
                                     uint64_t i, bool* bad) {
  if (HB) *bad |= sscan_load<Fr>(bv, b, i);
  if (AM == SREC_A_RESIDENT) {
    *bad |= sscan_load<Fr>(am, a, i);
    fr_to_mont<Fr>(am, am);
    return am;
  }
  return k;
}

// m = the map of scan positions [p0, p0 + SREC_E) below n, composed in scan order: the first half of a thread's work in
// k_scalars_rec_tile and k_scalars_rec_apply.  Per element: resident a, 1 (conversion) + 1 (A) + 1 with an addend (B);
// broadcast a, 1 + 1 with an addend; no a, none.  -> a record >= q was read.
template <class Fr, int AM, bool HB>
MSMZ_HD bool srec_compose_run(FrMap& m, const uint32_t* a, const uint32_t* b, const uint32_t* k, uint64_t p0, uint64_t n,
                              bool reverse) {
  fr_map_identity<Fr, AM != SREC_A_NONE, HB>(m);
  bool bad = false;
#pragma unroll 1
  for (int j = 0; j < SREC_E; j++) {
    const uint64_t p = p0 + (uint64_t)j;
    if (p >= n) break;
    uint32_t am[8], bv[8];
    const uint32_t* mul = srec_element<Fr, AM, HB>(am, bv, a, b, k, srec_entry(p, n, reverse), &bad);
    if (HB) {
      if (AM != SREC_A_NONE) fr_mont_mul<Fr>(m.B, mul, m.B);
      fr_add<Fr>(m.B, m.B, bv);
    }
    if (AM != SREC_A_NONE) fr_mont_mul<Fr>(m.A, mul, m.A);
  }
  return bad;
}

// The second half: from y = the value before scan position p0, walk the run and store y_p (EXCLUSIVE: the value the step
// at p started from) at p's entry of `out`.  y leaves as the value after the run.  Entry i of a and b is read before
// entry i of `out` is written and no other entry is touched, so `out` may be the a or the b range exactly.
// Per element: resident a, 2 (conversion, step); broadcast a, 1; no a, none.
template <class Fr, int AM, bool HB>
MSMZ_HD void srec_walk_run(uint32_t* out, uint32_t* y, const uint32_t* a, const uint32_t* b, const uint32_t* k, uint64_t p0,
                           uint64_t n, bool reverse, bool exclusive) {
#pragma unroll 1
  for (int j = 0; j < SREC_E; j++) {
    const uint64_t p = p0 + (uint64_t)j;
    if (p >= n) break;
    const uint64_t i = srec_entry(p, n, reverse);
    uint32_t am[8], bv[8], before[8];
    bool bad = false;
    const uint32_t* mul = srec_element<Fr, AM, HB>(am, bv, a, b, k, i, &bad);
#pragma unroll
    for (int w = 0; w < 8; w++) before[w] = y[w];
    if (AM != SREC_A_NONE) fr_mont_mul<Fr>(y, mul, y);
    if (HB) fr_add<Fr>(y, y, bv);
    sscan_store(out, i, exclusive ? before : y);
  }
}

// ---------------------------------------------------------------------------------------------- inversion
// Montgomery's trick on plain (canonical) residues with the product u (x) v = fr_mont_mul(u, v) = u v 2^-256, which is
// associative and commutative like the plain one.  With P_j = x_0 (x) ... (x) x_j and I_j = the PLAIN inverse of P_j,
//     x_j^-1 = I_j (x) P_(j-1)     and     I_(j-1) = I_j (x) x_j:
// the factors 2^-256 of the two sides cancel, so no operand is ever converted and every out_j is canonical.
//
// Both directions step through the run by template recursion on the element number, not by a loop under an unroll
// pragma: eight copies of the body exceed the size up to which the compiler honours the pragma, and a loop left rolled
// would index P at run time, which puts it into scratch memory.
//
// Forward, for elements [i0, i0 + SINV_E) below n: P[j], with a zero, a record >= q and an element beyond n replaced by
// 1; *zeros = the mask of the zeros; *bad |= a record >= q was read.  One product per element.
template <class Fr, int J>
MSMZ_HD void sinv_forward_step(uint32_t (&P)[SINV_E][8], uint32_t* zeros, bool* bad, const uint32_t* x, uint64_t i0,
                               uint64_t n) {
  uint32_t v[8];
  bool unit = true;
  if (i0 + (uint64_t)J < n) {
    const bool big = sscan_load<Fr>(v, x, i0 + (uint64_t)J);
    uint32_t any = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) any |= v[w];
    if (!any) *zeros |= 1u << J;
    *bad |= big;
    unit = big || !any;
  }
  if (unit) {
#pragma unroll
    for (int w = 0; w < 8; w++) v[w] = w == 0 ? 1u : 0u;
  }
  if constexpr (J == 0) {
#pragma unroll
    for (int w = 0; w < 8; w++) P[0][w] = v[w];
  } else {
    fr_mont_mul<Fr>(P[J], P[J - 1], v);
  }
  if constexpr (J + 1 < SINV_E) sinv_forward_step<Fr, J + 1>(P, zeros, bad, x, i0, n);
}

template <class Fr>
MSMZ_HD bool sinv_forward(uint32_t (&P)[SINV_E][8], uint32_t* zeros, const uint32_t* x, uint64_t i0, uint64_t n) {
  bool bad = false;
  *zeros = 0;
  sinv_forward_step<Fr, 0>(P, zeros, &bad, x, i0, n);
  return bad;
}

// Backward: I enters as the plain inverse of P[J]; out_J = x_J^-1, or 0 where x_J was 0.  Element J is read again (not
// kept: eight more records of registers) before out_J is written, highest J first, so `out` may be `x` exactly.  Two
// products per element.
template <class Fr, int J>
MSMZ_HD void sinv_backward_step(uint32_t* out, const uint32_t* x, const uint32_t (&P)[SINV_E][8], uint32_t* I,
                                uint32_t zeros, uint64_t i0, uint64_t n) {
  uint32_t o[8], v[8];
  if constexpr (J > 0) {
    fr_mont_mul<Fr>(o, I, P[J - 1]);
  } else {
#pragma unroll
    for (int w = 0; w < 8; w++) o[w] = I[w];
  }
  const bool zero = (zeros >> J) & 1u;
  bool unit = true;
  if (i0 + (uint64_t)J < n) {
    unit = sscan_load<Fr>(v, x, i0 + (uint64_t)J) || zero;
    if (zero) {
#pragma unroll
      for (int w = 0; w < 8; w++) o[w] = 0;
    }
    sscan_store(out, i0 + (uint64_t)J, o);
  }
  if constexpr (J > 0) {
    if (unit) {
#pragma unroll
      for (int w = 0; w < 8; w++) v[w] = w == 0 ? 1u : 0u;
    }
    fr_mont_mul<Fr>(I, I, v);
    sinv_backward_step<Fr, J - 1>(out, x, P, I, zeros, i0, n);
  }
}

// `inv` = the plain inverse of P[SINV_E - 1]
template <class Fr>
MSMZ_HD void sinv_backward(uint32_t* out, const uint32_t* x, const uint32_t (&P)[SINV_E][8], const uint32_t* inv,
                           uint32_t zeros, uint64_t i0, uint64_t n) {
  uint32_t I[8];
#pragma unroll
  for (int w = 0; w < 8; w++) I[w] = inv[w];
  sinv_backward_step<Fr, SINV_E - 1>(out, x, P, I, zeros, i0, n);
}

}  // namespace msmz

#if defined(__HIPCC__)
namespace msmz {

// m = the composition of the maps of lanes 0 .. own lane, in lane order (all 64 lanes must be here): six steps, each a
// shuffle of the map from `s` lanes below and one composition
template <class Fr, bool HA, bool HB>
__device__ __forceinline__ void fr_map_wave_scan(FrMap& m) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    FrMap o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (HA) o.A[j] = (uint32_t)__shfl_up((int)m.A[j], s, 64);
      if (HB) o.B[j] = (uint32_t)__shfl_up((int)m.B[j], s, 64);
    }
    if (lane >= (uint32_t)s) fr_map_compose<Fr, HA, HB>(m, m, o);
  }
}

// the maps of the four waves, through LDS
template <bool HA, bool HB>
struct MapShare {
  uint32_t A[HA ? SREC_THREADS / 64 : 1][8];
  uint32_t B[HB ? SREC_THREADS / 64 : 1][8];
};

template <bool HA, bool HB>
__device__ __forceinline__ void map_share_put(MapShare<HA, HB>& sh, uint32_t w, const FrMap& m) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (HA) sh.A[w][j] = m.A[j];
    if (HB) sh.B[w][j] = m.B[j];
  }
}

template <bool HA, bool HB>
__device__ __forceinline__ void map_share_get(FrMap& m, const MapShare<HA, HB>& sh, uint32_t w) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (HA) m.A[j] = sh.A[w][j];
    if (HB) m.B[j] = sh.B[w][j];
  }
}

// agg[tile] = the map of the tile's SREC_TILE scan positions (A in Montgomery form into aggA, B into aggB; only what the
// mode carries).  Thread t composes its run, the wave scans, thread 0 composes the four wave totals.  A record >= q
// raises bit 2 of *err: this launch reads every entry of the ranges, the third one need not look again.
template <class Fr, int AM, bool HB>
__global__ void __launch_bounds__(SREC_THREADS) k_scalars_rec_tile(uint32_t* aggA, uint32_t* aggB, const uint32_t* a,
                                                                   const uint32_t* b, FrConst k, uint32_t n, uint32_t flags,
                                                                   uint32_t* err) {
  constexpr bool HA = AM != SREC_A_NONE;
  __shared__ MapShare<HA, HB> sh;
  const uint64_t p0 = (uint64_t)blockIdx.x * SREC_TILE + (uint64_t)threadIdx.x * SREC_E;
  FrMap m;
  if (srec_compose_run<Fr, AM, HB>(m, a, b, k.w, p0, n, flags & SREC_REVERSE)) atomicOr(err, 4u);
  fr_map_wave_scan<Fr, HA, HB>(m);
  if ((threadIdx.x & 63u) == 63u) map_share_put<HA, HB>(sh, threadIdx.x >> 6, m);
  __syncthreads();
  if (threadIdx.x == 0) {
    map_share_get<HA, HB>(m, sh, 0);
#pragma unroll
    for (int w = 1; w < SREC_THREADS / 64; w++) {
      FrMap o;
      map_share_get<HA, HB>(o, sh, w);
      fr_map_compose<Fr, HA, HB>(m, o, m);
    }
    if (HA) sscan_store(aggA, blockIdx.x, m.A);
    if (HB) sscan_store(aggB, blockIdx.x, m.B);
  }
}

// incoming[t] = the value before tile t's first scan position, t <= count; incoming[0] = init and incoming[count] = the
// final y, which also goes to `last`.  ONE workgroup: per pass thread t takes aggregate base + t, the block scans as
// above, and the running value is carried from pass to pass through LDS.  It waits on no other workgroup.
template <class Fr, bool HA, bool HB>
__global__ void __launch_bounds__(SREC_THREADS) k_scalars_rec_carry(uint32_t* incoming, uint32_t* last, const uint32_t* aggA,
                                                                    const uint32_t* aggB, FrConst init, uint32_t count) {
  __shared__ MapShare<HA, HB> sh;
  __shared__ uint32_t carried[8];
  const uint32_t wave = threadIdx.x >> 6;
  uint32_t carry[8];
#pragma unroll
  for (int j = 0; j < 8; j++) carry[j] = init.w[j];
  if (threadIdx.x == 0) sscan_store(incoming, 0, carry);
#pragma unroll 1
  for (uint32_t base = 0; base < count; base += SREC_PASS) {
    const uint32_t t = base + threadIdx.x;   // (count <= 2^21: no wrap)
    FrMap m;
    fr_map_identity<Fr, HA, HB>(m);
    if (t < count) {
      if (HA) sscan_load<Fr>(m.A, aggA, t);
      if (HB) sscan_load<Fr>(m.B, aggB, t);
    }
    fr_map_wave_scan<Fr, HA, HB>(m);
    if ((threadIdx.x & 63u) == 63u) map_share_put<HA, HB>(sh, wave, m);
    __syncthreads();
    uint32_t y[8];
#pragma unroll
    for (int j = 0; j < 8; j++) y[j] = carry[j];
#pragma unroll 1
    for (uint32_t w = 0; w < wave; w++) {
      FrMap o;
      map_share_get<HA, HB>(o, sh, w);
      fr_map_apply<Fr, HA, HB>(y, o);
    }
    fr_map_apply<Fr, HA, HB>(y, m);
    if (t < count) sscan_store(incoming, (uint64_t)t + 1, y);
    if (threadIdx.x == SREC_THREADS - 1) {
#pragma unroll
      for (int j = 0; j < 8; j++) carried[j] = y[j];   // (threads past `count` hold the identity: this is the last value)
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; j++) carry[j] = carried[j];
    // (the next pass writes `sh` before and `carried` after its first barrier: both after every read above)
  }
  if (threadIdx.x == 0) sscan_store(last, 0, carry);
}

// out = the recurrence's values over the tile: thread t's incoming value is the tile's, sent through the maps of the
// waves and of the lanes before it; then it walks its run (srec_walk_run).  A thread reads only entries it owns, all of
// them before its first write (the run is composed first), and entry i again just before it writes entry i.
template <class Fr, int AM, bool HB>
__global__ void __launch_bounds__(SREC_THREADS) k_scalars_rec_apply(uint32_t* out, const uint32_t* a, const uint32_t* b,
                                                                    FrConst k, const uint32_t* incoming, uint32_t n,
                                                                    uint32_t flags) {
  constexpr bool HA = AM != SREC_A_NONE;
  __shared__ MapShare<HA, HB> sh;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint64_t p0 = (uint64_t)blockIdx.x * SREC_TILE + (uint64_t)threadIdx.x * SREC_E;
  FrMap m;
  srec_compose_run<Fr, AM, HB>(m, a, b, k.w, p0, n, flags & SREC_REVERSE);
  fr_map_wave_scan<Fr, HA, HB>(m);
  if (lane == 63u) map_share_put<HA, HB>(sh, wave, m);
  FrMap before;   // the lanes below this one
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (HA) before.A[j] = (uint32_t)__shfl_up((int)m.A[j], 1, 64);
    if (HB) before.B[j] = (uint32_t)__shfl_up((int)m.B[j], 1, 64);
  }
  __syncthreads();
  uint32_t y[8];
  sscan_load<Fr>(y, incoming, blockIdx.x);
#pragma unroll 1
  for (uint32_t w = 0; w < wave; w++) {
    FrMap o;
    map_share_get<HA, HB>(o, sh, w);
    fr_map_apply<Fr, HA, HB>(y, o);
  }
  if (lane) fr_map_apply<Fr, HA, HB>(y, before);
  srec_walk_run<Fr, AM, HB>(out, y, a, b, k.w, p0, n, flags & SREC_REVERSE, flags & SREC_EXCLUSIVE);
}

// a (x)= the same value of every lane below (inclusive), by six shuffle steps
template <class Fr>
__device__ __forceinline__ void fr_wave_prefix_product(uint32_t* a) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = (uint32_t)__shfl_up((int)a[j], s, 64);
    if (lane >= (uint32_t)s) fr_mont_mul<Fr>(a, a, o);
  }
}

// ... and of every lane above (inclusive)
template <class Fr>
__device__ __forceinline__ void fr_wave_suffix_product(uint32_t* a) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = (uint32_t)__shfl_down((int)a[j], s, 64);
    if (lane + (uint32_t)s < 64u) fr_mont_mul<Fr>(a, a, o);
  }
}

// out_i = x_i^-1 (0 -> 0), res[9] += the zeros, bit 2 of res[8] for a record >= q.  A wave takes a chunk of SINV_CHUNK
// consecutive elements, lane l elements [l SINV_E, (l + 1) SINV_E) of it.  With t_l the lane totals (sinv_forward),
// S = t_0 (x) ... (x) t_63 and ONE fr_inv(S) per chunk (every lane computes the same value: one instruction stream),
// the plain inverse of t_l is fr_inv(S) (x) (the totals below l) (x) (the totals above l): a prefix and a suffix scan
// of the totals, 12 products and 2 more; then sinv_backward.  Whole waves run (the grid covers whole chunks), elements
// at or beyond n count as 1 and are neither read nor written.
template <class Fr>
__global__ void __launch_bounds__(SINV_THREADS) k_scalars_inverse(uint32_t* out, const uint32_t* x, uint32_t n,
                                                                  uint32_t* res) {
  __shared__ uint32_t nzero;
  if (threadIdx.x == 0) nzero = 0;
  __syncthreads();
  const uint64_t i0 = ((uint64_t)blockIdx.x * SINV_THREADS + threadIdx.x) * SINV_E;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t P[SINV_E][8];
  uint32_t zeros;
  if (sinv_forward<Fr>(P, &zeros, x, i0, n)) atomicOr(res + 8, 4u);
  uint32_t pre[8], suf[8], inv[8];
#pragma unroll
  for (int j = 0; j < 8; j++) pre[j] = suf[j] = P[SINV_E - 1][j];
  fr_wave_prefix_product<Fr>(pre);
  fr_wave_suffix_product<Fr>(suf);
#pragma unroll
  for (int j = 0; j < 8; j++) inv[j] = (uint32_t)__shfl((int)pre[j], 63, 64);   // S
  fr_inv<Fr>(inv, inv);
  // the totals strictly below and strictly above this lane
  uint32_t below[8], above[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    below[j] = (uint32_t)__shfl_up((int)pre[j], 1, 64);
    above[j] = (uint32_t)__shfl_down((int)suf[j], 1, 64);
  }
  if (lane) fr_mont_mul<Fr>(inv, inv, below);
  if (lane != 63u) fr_mont_mul<Fr>(inv, inv, above);
  sinv_backward<Fr>(out, x, P, inv, zeros, i0, n);
  uint32_t cnt = (uint32_t)__popc(zeros);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, s, 64);
  if (lane == 0 && cnt) atomicAdd(&nzero, cnt);
  __syncthreads();
  if (threadIdx.x == 0 && nzero) atomicAdd(res + 9, nzero);
}

}  // namespace msmz
#endif

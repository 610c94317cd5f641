// Import kernels (msmz_import_scalars / _into / msmz_import_points, include/msmz.h): records where the caller has them
// -- device memory or the packed staging copy of a host buffer -- in the form they have -- narrow, strided, canonical or
// 64-bit-limb Montgomery -- to the resident formats the MSM kernels read.  Streaming kernels: one thread per record, no
// LDS, no scratch.  The engine launches them only on pointers the HIP runtime has classified (Engine::vouch).
#pragma once
#include "kernels.h"

namespace msmz {

// `words` 32-bit words of the record at src + i * stride bytes (4-byte aligned), the rest of dst[0 .. MAXW) zero.
// Consecutive lanes read consecutive records: at stride = 4 * words every fetched line is used whole.
template <int MAXW>
__device__ __forceinline__ void import_load(uint32_t* dst, const uint8_t* src, uint64_t stride, uint32_t i, int words) {
  const uint32_t* p = reinterpret_cast<const uint32_t*>(src + (size_t)i * stride);
#pragma unroll
  for (int j = 0; j < MAXW; j++) dst[j] = j < words ? p[j] : 0u;
}

// out[i] = the 32-byte canonical scalar of record i (`words` = width / 4 little-endian words, zero-extended; mont: the
// record is v * 2^256 mod q and v is stored).  A raw value >= q raises bit 2 of *err, as k_check_scalars does.
template <class Fr>
__global__ void __launch_bounds__(256) k_import_scalars(uint32_t* out, const uint8_t* src, uint64_t stride, int words,
                                                        uint32_t n, int mont, uint32_t* err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t s[8];
  import_load<8>(s, src, stride, i, words);
  if (words_geq<8>(s, Fr::Q)) atomicOr(err, 4u);
  if (mont) fr_from_mont<Fr>(s, s);
  uint4* o = reinterpret_cast<uint4*>(out + (size_t)i * 8);
  o[0] = make_uint4(s[0], s[1], s[2], s[3]);
  o[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// the factor that takes a loaded coordinate to the kernels' Montgomery form: R^2 for canonical input (fe_to_mont),
// R^2 / 2^(32 NW) for 64-bit-limb Montgomery input
template <class F>
__device__ __forceinline__ void import_factor(Fe<F>& c, int mont) {
#pragma unroll
  for (int j = 0; j < F::N; j++) c.l[j] = mont ? F::R2STD[j] : F::R2[j];
}

// (x | y) records of 2 NW words at src + i * stride -> resident point records, exactly as k_points_to_resident writes
// them (Weierstrass: flagged points all-zero; with `endo`, records [n, 2n) hold (beta x, y)).  The raw words of either
// form must be < p.
template <class P>
__global__ void __launch_bounds__(256) k_import_points(uint32_t* out, const uint8_t* src, uint64_t stride,
                                                       const uint8_t* is_inf, uint32_t n, int endo, int mont,
                                                       uint32_t* err) {
  using F = typename P::F;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[2 * F::NW];
  import_load<2 * F::NW>(w, src, stride, i, 2 * F::NW);
  if (words_geq<F::NW>(w, F::PW) || words_geq<F::NW>(w + F::NW, F::PW)) atomicOr(err, 4u);
  Fe<F> px, py, f, x, y;
  fe_unpack<F>(px, w);
  fe_unpack<F>(py, w + F::NW);
  const bool flagged = is_inf != nullptr && is_inf[i] != 0;
  import_factor<F>(f, mont);
  fe_mul(x, px, f);
  fe_mul(y, py, f);
  P::store_resident(out, i, n, x, y, flagged, endo);
}

}  // namespace msmz

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

// Compressed records (msmz_import_points with MSMZ_SRC_COMPRESSED): F::NW little-endian words at
// src + i * stride, the wire coordinate (x; y on the twisted Edwards curve) with the sign of the other coordinate in
// bit 7 of the last byte, which every field leaves free.  The bit is masked off, the coordinate range-checked (bit 2 of
// *err), the point recovered by P::decompress -- one fe_sqrt per point (sqrt.h), the same instructions in every lane --
// and a record without a root or with a sign bit on a zero root raises bit 3 of *err.  The result goes through
// P::store_resident exactly as k_import_points writes it.  A flagged record is not read: it becomes the infinity record
// (the identity (0, 1) on the twisted Edwards curve, which has no point at infinity).  A refused record stores the
// same: the set is discarded, but every word written is defined.  One thread per point; the tables of the square root
// are read from constant memory (no LDS), everything else stays in registers.
template <class P>
__global__ void __launch_bounds__(256) k_import_points_compressed(uint32_t* out, const uint8_t* src, uint64_t stride,
                                                                  const uint8_t* is_inf, uint32_t n, int endo,
                                                                  int parity, uint32_t* err) {
  using F = typename P::F;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool flagged = is_inf != nullptr && is_inf[i] != 0;
  Fe<F> x, y;
  bool good = false;
  if (!flagged) {
    uint32_t w[F::NW];
    import_load<F::NW>(w, src, stride, i, F::NW);
    const bool sign = (w[F::NW - 1] >> 31) != 0;
    w[F::NW - 1] &= 0x7fffffffu;
    if (words_geq<F::NW>(w, F::PW)) {
      atomicOr(err, 4u);
    } else {
      Fe<F> c, f, wire;
      fe_unpack<F>(c, w);
      import_factor<F>(f, 0);
      fe_mul(wire, c, f);
      good = P::decompress(x, y, wire, sign, parity) == DECOMPRESS_OK;
      if (!good) atomicOr(err, 8u);
    }
  }
  if (!good) {
    fe_zero(x);
    fe_set_const<F>(y, F::ONE);
    flagged = true;
  }
  P::store_resident(out, i, n, x, y, flagged, endo);
}

// resident records -> compressed records of F::NW words (the inverse of the above; msmz_download_points_compressed) and
// one flag byte per point: the point at infinity is the all-zero record with flag 1.  (The flag cannot be read off the
// bytes: (0, 1) of BLS12-377 compresses to all-zero bytes under the `largest` convention.)
// (the per-record body, shared with k_export_points of export_kernels.h: w = the compressed record of the resident
// record at `rec`, -> is it the point at infinity)
template <class P>
__device__ __forceinline__ bool compress_record(uint32_t* w, const uint32_t* rec, int parity) {
  using F = typename P::F;
  Fe<F> x, y;
  const bool inf = P::load_resident_affine(x, y, rec);
  if (inf) {
#pragma unroll
    for (int j = 0; j < F::NW; j++) w[j] = 0;
  } else {
    Fe<F> t;
    bool zero;
    fe_carry(y);   // (a twisted-Edwards y is (y - x) + x of a record: two lazy values added)
    fe_from_mont(t, P::TE ? y : x);
    fe_to_canon_words<F>(w, t);
    if (fe_wire_sign<F>(&zero, P::TE ? x : y, parity)) w[F::NW - 1] |= 0x80000000u;   // (the value 0 has sign 0)
  }
  return inf;
}

template <class P>
__global__ void __launch_bounds__(256) k_points_compress(uint32_t* out, uint8_t* inf_out, const uint32_t* in, uint32_t n,
                                                         int parity) {
  using F = typename P::F;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[F::NW];
  const bool inf = compress_record<P>(w, in + (size_t)i * P::IN_WORDS, parity);
  uint32_t* o = out + (size_t)i * F::NW;
#pragma unroll
  for (int j = 0; j < F::NW; j += 4) *reinterpret_cast<uint4*>(o + j) = make_uint4(w[j], w[j + 1], w[j + 2], w[j + 3]);
  inf_out[i] = inf ? 1 : 0;
}

}  // namespace msmz

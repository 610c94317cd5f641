// Export kernels (msmz_export_scalars / msmz_export_points, include/msmz.h): the import kernels
// (import_kernels.h) read in the other direction.  Resident records go where the caller wants them -- device memory, or
// the packed staging buffer on the way to a host destination -- in the form it wants: narrow, strided, canonical,
// 64-bit-limb Montgomery or compressed.  Streaming kernels: one thread per record, no LDS, no scratch.  The engine
// launches them only on pointers the HIP runtime has classified (ResidentSets::vouch); a thread writes the `words` words
// of its own record at dst + i * stride and nothing else.
#pragma once
#include "../../include/msmz.h"
#include "fr.h"
#include "import_kernels.h"

namespace msmz {

// May a record be stored 16 bytes at a time?  Only where the pointer, the stride and the width are all multiples of 16:
// then every record starts 16-byte aligned and is whole 16-byte pieces.  All three are kernel arguments, so the answer is
// the same in every lane of every wave.
__device__ __forceinline__ bool export_vec16(const uint8_t* dst, uint64_t stride, int words) {
  return ((reinterpret_cast<uintptr_t>(dst) | stride | (uint64_t)(4 * words)) & 15u) == 0;
}

// the first `words` of w[0 .. MAXW) to the record at dst + i * stride bytes (4-byte aligned): 16 bytes per store where
// export_vec16 allows (a 32-byte record per lane at stride 32 is two such stores), else one word per store.
// Consecutive lanes write consecutive records: at stride = 4 * words every line written is written whole.
template <int MAXW>
__device__ __forceinline__ void export_store(uint8_t* dst, uint64_t stride, uint32_t i, const uint32_t* w, int words) {
  static_assert(MAXW % 4 == 0, "whole 16-byte pieces");
  uint8_t* rec = dst + (size_t)i * stride;
  if (export_vec16(dst, stride, words)) {
    uint4* p = reinterpret_cast<uint4*>(rec);
#pragma unroll
    for (int j = 0; j < MAXW / 4; j++)
      if (4 * j < words) p[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
  } else {
    uint32_t* p = reinterpret_cast<uint32_t*>(rec);
#pragma unroll
    for (int j = 0; j < MAXW; j++)
      if (j < words) p[j] = w[j];
  }
}

// record i at dst + i * stride = entry i of the resident scalars at src: its low `words` 32-bit words, little-endian
// (mont: v * 2^256 mod q, all 8 words: what fr_to_mont of fr.h computes, the inverse of k_import_scalars).  An entry
// >= q, or one with a non-zero word at or above `words`, raises bit 2 of *err.
template <class Fr>
__global__ void __launch_bounds__(256) k_export_scalars(uint8_t* dst, uint64_t stride, int words, const uint32_t* src,
                                                        uint32_t n, int mont, uint32_t* err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t s[8];
  load_scalar(s, src, i);
  uint32_t high = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) high |= j >= words ? s[j] : 0u;
  if (high != 0 || words_geq<8>(s, Fr::Q)) atomicOr(err, 4u);
  if (mont) fr_to_mont<Fr>(s, s);
  export_store<8>(dst, stride, i, s, words);
}

// record i at dst + i * stride = resident point record i of src, in the form the MSMZ_SRC_* bits of `form` name:
//   0                     x || y canonical, 2 NW words: what k_points_from_resident writes
//   MSMZ_SRC_MONTGOMERY   x || y as v * 2^(32 NW) mod p: ONE product of the resident v * R with F::RSTD = 2^(32 NW) mod p
//                         (the Montgomery product divides by R), the inverse of import_factor(.., mont)
//   MSMZ_SRC_COMPRESSED   NW words, one coordinate + sign bit (| MSMZ_SRC_SIGN_PARITY): compress_record, the body of
//                         k_points_compress
// The point at infinity of a Weierstrass curve is the all-zero record in every form, and inf_out[i] (if given) is 1.
// `form` is the same in every lane: its branches are wave-uniform.
template <class P>
__global__ void __launch_bounds__(256) k_export_points(uint8_t* dst, uint64_t stride, uint8_t* inf_out,
                                                       const uint32_t* src, uint32_t n, int form) {
  using F = typename P::F;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* rec = src + (size_t)i * P::IN_WORDS;
  uint32_t w[2 * F::NW];
  bool inf;
  if (form & MSMZ_SRC_COMPRESSED) {
    inf = compress_record<P>(w, rec, (form & MSMZ_SRC_SIGN_PARITY) ? 1 : 0);
    export_store<F::NW>(dst, stride, i, w, F::NW);
  } else {
    Fe<F> x, y;
    inf = P::load_resident_affine(x, y, rec);
    if (inf) {
#pragma unroll
      for (int j = 0; j < 2 * F::NW; j++) w[j] = 0;
    } else {
      Fe<F> f, t;
      if (P::TE) fe_carry(y);   // (a twisted-Edwards y is (y - x) + x of a record: two lazy values added)
      if (form & MSMZ_SRC_MONTGOMERY) {
        fe_set_const<F>(f, F::RSTD);
      } else {   // (fe_from_mont: the product with 1)
        fe_zero(f);
        f.l[0] = 1;
      }
      fe_mul(t, x, f);
      fe_to_canon_words<F>(w, t);
      fe_mul(t, y, f);
      fe_to_canon_words<F>(w + F::NW, t);
    }
    export_store<2 * F::NW>(dst, stride, i, w, 2 * F::NW);
  }
  if (inf_out) inf_out[i] = inf ? 1 : 0;
}

}  // namespace msmz

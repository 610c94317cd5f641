// Seeded synthetic inputs generated on the GPU -- the analogue of the reference's
// `randomPointsFast` / `randomScalars` (src/curve-random.ts:14-92, 151-194), which draw from an
// unseeded `crypto.getRandomValues`.  Here everything is a pure function of (seed, index):
//
//   point i  = a_i * G,  a_i = splitmix64(seed, i)  -- a sum of table entries  T_k[w_k],  w_k the
//              k-th 13-bit window of a_i and T_k[w] = w * 2^(13k) * G  (same windowed construction as
//              curve-random.ts:24-91, but over multiples of the generator so that a_i is known and
//              an MSM over any N has the closed form (sum s_i a_i) * G).
//   scalar i = first of the 32-byte little-endian draws  u(seed, i, attempt)  that is < q after
//              masking to the bit length of q  (curve-random.ts:151-190 rejection sampling).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "multi.h"

namespace msmz {

constexpr int GEN_BITS = 13;
constexpr int GEN_TABLE = 1 << GEN_BITS;
constexpr int GEN_WINDOWS = 5;   // 5 * 13 = 65 >= 64 bits

// local index on one device of a multi-GPU context -> global (seeded) index; identity for a single device
MSMZ_HD uint64_t gen_global_index(uint32_t local, const GenMap& m) {
  const uint64_t blk = (uint64_t)local >> m.blk_shift;
  return ((blk * m.nshards + m.shard) << m.blk_shift) | ((uint64_t)local & ((1ull << m.blk_shift) - 1));
}

MSMZ_HD uint64_t splitmix64(uint64_t seed, uint64_t index) {
  uint64_t z = seed + (index + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Montgomery affine coordinates of an accumulator that is not the point at infinity
template <class P>
__device__ __forceinline__ void gen_to_affine(Fe<typename P::F>& x, Fe<typename P::F>& y, const typename P::Acc& acc) {
  Fe<typename P::F> inv;
  fe_inverse(inv, P::denominator(acc));
  P::affine_from_inverse(x, y, acc, inv);
}

// table[k * GEN_TABLE + w] = w * base_k as an affine [x | y] record of 2*NW words; w = 0: the all-zero record of the
// point at infinity (Weierstrass) / the identity (0, 1) (twisted Edwards)
template <class P>
__global__ void __launch_bounds__(128) k_gen_table(uint32_t* table, const uint32_t* bases) {
  using F = typename P::F;
  constexpr int RW = 2 * F::NW;
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= GEN_WINDOWS * GEN_TABLE) return;
  uint32_t k = t / GEN_TABLE, w = t % GEN_TABLE;
  Affine<F> base;
  load_affine<F>(base, bases + (size_t)k * RW, 0);
  typename P::Acc acc, tmp;
  P::set_identity(acc);
  for (int bit = GEN_BITS - 1; bit >= 0; bit--) {
    P::dbl(tmp, acc);
    acc = tmp;
    if ((w >> bit) & 1u) {
      P::add_affine(tmp, acc, base.x, base.y);
      acc = tmp;
    }
  }
  Affine<F> a;
  const bool inf = !P::TE && P::is_identity(acc);
  if (!inf) gen_to_affine<P>(a.x, a.y, acc);
  store_affine<F>(table + (size_t)t * RW, a, inf);
}

template <class P>
__global__ void __launch_bounds__(128) k_gen_points(uint32_t* out, const uint32_t* table, uint32_t n, uint64_t seed,
                                                    int endo, GenMap map) {
  using F = typename P::F;
  constexpr int RW = 2 * F::NW;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t a = splitmix64(seed, gen_global_index(i, map));
  typename P::Acc acc, tmp;
  P::set_identity(acc);
#pragma unroll 1
  for (int k = 0; k < GEN_WINDOWS; k++) {
    uint32_t w = (uint32_t)(a >> (GEN_BITS * k)) & (GEN_TABLE - 1);
    if (w == 0) continue;
    Affine<F> p;
    load_affine<F>(p, table + ((size_t)k * GEN_TABLE + w) * RW, 0);
    P::add_affine(tmp, acc, p.x, p.y);
    acc = tmp;
  }
  Fe<F> x, y;
  const bool inf = !P::TE && P::is_identity(acc);
  if (!inf) gen_to_affine<P>(x, y, acc);
  P::store_resident(out, i, n, x, y, inf, endo);
}

template <class Fr>
__global__ void __launch_bounds__(256) k_gen_scalars(uint32_t* out, uint32_t n, uint64_t seed, GenMap map) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t gi = gen_global_index(i, map);
  constexpr int TOP_BITS = Fr::BITS - 224;            // bits kept in the top 32-bit word
  constexpr uint32_t TOP_MASK = TOP_BITS >= 32 ? 0xffffffffu : ((1u << TOP_BITS) - 1u);
  uint32_t w[8];
  for (uint32_t attempt = 0; attempt < 64; attempt++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint64_t v = splitmix64(seed ^ 0x5ca1a75ull, (gi * 64 + attempt) * 4 + j);
      w[2 * j] = (uint32_t)v;
      w[2 * j + 1] = (uint32_t)(v >> 32);
    }
    w[7] &= TOP_MASK;
    if (!words_geq<8>(w, Fr::Q)) break;
    if (attempt == 63) {
#pragma unroll
      for (int j = 0; j < 8; j++) w[j] = 0;   // unreachable in practice (p ~ 2^-64)
    }
  }
  uint4* o = reinterpret_cast<uint4*>(out + (size_t)i * 8);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

}  // namespace msmz

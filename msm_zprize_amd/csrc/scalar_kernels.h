// Arithmetic over resident scalar sets (msmz_scalars_combine / _dot / _powers, include/msmz.h):
//     combine:  out_i = A_i x_i (+ B_i y_i)       A, B: one broadcast scalar each, or resident vectors
//     dot:      sum_i x_i y_i  or  sum_i x_i
//     powers:   out_i = base ratio^i
// all mod q, on the 8-word canonical records of a scalar set, with the F_q functions of fr.h.  The first part of this
// file is host/device code: the geometry of the dot product and of the powers runs, and the body of the powers
// kernel, which tests/native/scalar_ops_test.cpp runs on the CPU.  The kernels follow, for the device compiler only.
#pragma once
#if defined(__HIPCC__)
#include "gen_kernels.h"
#include "kernels.h"
#endif
#include "fr.h"

namespace msmz {

// dot product, level 1: a workgroup of SDOT_THREADS covers a tile of SDOT_TILE consecutive elements, SDOT_E a thread,
// and leaves one partial sum; level 2: ONE workgroup folds the partial sums, SDOT_PASS of them per pass of its loop
constexpr int SDOT_THREADS = 256;
constexpr int SDOT_E = 8;
constexpr int SDOT_TILE = SDOT_THREADS * SDOT_E;
constexpr int SDOT_PASS = SDOT_THREADS;
// powers: consecutive indices one thread walks.  It divides the block of a multi-device split, so a run never crosses
// from one block of set indices into another.
constexpr int SPOW_RUN = 8;

// a scalar passed to a kernel by value (it arrives in scalar registers)
struct FrConst {
  uint32_t w[8];
};

// The body of k_scalars_powers for one thread: out[j] = base ratio^(g + j), j < count <= SPOW_RUN, as 8-word records
// behind `out` (16-byte aligned).  At most 32 + count - 1 products.
template <class Fr>
MSMZ_HD void fr_pow_run(uint32_t* out, const uint32_t* base, const FrPowTable& t, uint32_t g, uint32_t count) {
  uint32_t acc[8];
  fr_pow_start<Fr>(acc, base, t, g);
  uint32_t* o = static_cast<uint32_t*>(__builtin_assume_aligned(out, 16));
#pragma unroll 1
  for (uint32_t j = 0; j < count; j++) {
    if (j) fr_pow_step<Fr>(acc, t);
#pragma unroll
    for (int k = 0; k < 8; k++) o[(size_t)j * 8 + k] = acc[k];
  }
}

}  // namespace msmz

#if defined(__HIPCC__)
namespace msmz {

static_assert((1 << MULTI_BLOCK_SHIFT) % SPOW_RUN == 0, "a run of powers stays inside one block of set indices");

// record i of a scalar set -> s; true if it is >= q
template <class Fr>
__device__ __forceinline__ bool fr_load(uint32_t* s, const uint32_t* set, uint64_t i) {
  load_scalar(s, set, i);
  return words_geq<8>(s, Fr::Q);
}

__device__ __forceinline__ void fr_store(uint32_t* set, uint64_t i, const uint32_t* s) {
  uint4* o = reinterpret_cast<uint4*>(set + i * 8);
  o[0] = make_uint4(s[0], s[1], s[2], s[3]);
  o[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// One term c (.) v of a combination.  v: first record of the range (nullptr: the term is absent); c: first record of a
// coefficient range, or nullptr = the broadcast coefficient k, already k 2^256 mod q (one product), or `unit`: 1.
struct ScalarTerm {
  const uint32_t* v;
  const uint32_t* c;
  FrConst k;
  uint32_t unit;
};

// t = c_i v_i; true if a record read for it is >= q
template <class Fr>
__device__ __forceinline__ bool scalar_term(uint32_t* t, const ScalarTerm& T, uint32_t i) {
  uint32_t v[8];
  bool bad = fr_load<Fr>(v, T.v, i);
  if (T.c) {
    uint32_t c[8];
    bad |= fr_load<Fr>(c, T.c, i);
    fr_mul<Fr>(t, c, v);            // two products: both operands are canonical
  } else if (T.unit) {
#pragma unroll
    for (int j = 0; j < 8; j++) t[j] = v[j];
  } else {
    fr_mont_mul<Fr>(t, T.k.w, v);   // one
  }
  return bad;
}

// out_i = x.c_i x.v_i (+ y.c_i y.v_i).  One thread per element: it reads record i of every range and then writes record
// i of `out`, so `out` may be one of the ranges exactly (an in-place fold) or lie apart from them; the host refuses a
// partial overlap.  A record >= q raises bit 2 of *err (as k_points_mul does for a resident scalar).
template <class Fr>
__global__ void __launch_bounds__(256) k_scalars_combine(uint32_t* out, ScalarTerm x, ScalarTerm y, uint32_t n,
                                                         uint32_t* err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t r[8];
  bool bad = scalar_term<Fr>(r, x, i);
  if (y.v) {
    uint32_t t[8];
    bad |= scalar_term<Fr>(t, y, i);
    fr_add<Fr>(r, r, t);
  }
  if (bad) atomicOr(err, 4u);
  fr_store(out, i, r);
}

// a += the same value of every other lane of the wave (all 64 lanes must be here), by butterfly exchanges
template <class Fr>
__device__ __forceinline__ void fr_wave_sum(uint32_t* a) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = (uint32_t)__shfl_xor((int)a[j], s, 64);
    fr_add<Fr>(a, a, o);
  }
}

// the sum of `a` over the SDOT_THREADS threads of the workgroup, valid in thread 0: the waves by fr_wave_sum, their four
// sums through LDS.  Every thread of the workgroup must be here.
template <class Fr>
__device__ __forceinline__ void fr_block_sum(uint32_t* a) {
  __shared__ uint32_t sh[SDOT_THREADS / 64][8];
  fr_wave_sum<Fr>(a);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (int j = 0; j < 8; j++) sh[wave][j] = a[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < SDOT_THREADS / 64; w++) {
      uint32_t o[8];
#pragma unroll
      for (int j = 0; j < 8; j++) o[j] = sh[w][j];
      fr_add<Fr>(a, a, o);
    }
  }
}

// partial[tile] = sum over the tile's elements of x_i y_i 2^-256 (y == nullptr: of x_i).  Thread t takes elements
// tile SDOT_TILE + e SDOT_THREADS + t: a wave reads 2 KiB in a row.  No atomics on the sums: addition mod q is exact,
// so the result does not depend on the order.  A record >= q raises bit 2 of *err.
template <class Fr>
__global__ void __launch_bounds__(SDOT_THREADS) k_scalars_dot(uint32_t* partial, const uint32_t* x, const uint32_t* y,
                                                              uint32_t n, uint32_t* err) {
  const uint64_t base = (uint64_t)blockIdx.x * SDOT_TILE + threadIdx.x;
  uint32_t acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0;
  bool bad = false;
#pragma unroll 1
  for (int e = 0; e < SDOT_E; e++) {
    const uint64_t i = base + (uint64_t)e * SDOT_THREADS;
    if (i < n) {
      uint32_t a[8];
      bad |= fr_load<Fr>(a, x, i);
      if (y) {
        uint32_t b[8];
        bad |= fr_load<Fr>(b, y, i);
        fr_mont_mul<Fr>(a, a, b);
      }
      if (!bad) fr_add<Fr>(acc, acc, a);   // (a flagged record is not below q: it stays out of the sum)
    }
  }
  if (bad) atomicOr(err, 4u);
  fr_block_sum<Fr>(acc);
  if (threadIdx.x == 0) fr_store(partial, blockIdx.x, acc);
}

// result = the sum of `count` partial sums, times 2^256 if to_canon (the ONE conversion of a product sum).  One
// workgroup; thread t adds partials t, t + SDOT_PASS, ...  A grid of several workgroups folds as many sums at once
// (the values of a sumcheck round, mle_kernels.h): workgroup b takes partials [b count, (b + 1) count) into record b.
template <class Fr>
__global__ void __launch_bounds__(SDOT_THREADS) k_scalars_dot_fold(uint32_t* result, const uint32_t* partial,
                                                                   uint32_t count, int to_canon) {
  result += (size_t)blockIdx.x * 8;
  partial += (size_t)blockIdx.x * count * 8;
  uint32_t acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0;
#pragma unroll 1
  for (uint32_t i = threadIdx.x; i < count; i += SDOT_PASS) {
    uint32_t a[8];
    fr_load<Fr>(a, partial, i);
    fr_add<Fr>(acc, acc, a);
  }
  fr_block_sum<Fr>(acc);
  if (threadIdx.x == 0) {
    if (to_canon) fr_to_mont<Fr>(acc, acc);
    fr_store(result, 0, acc);
  }
}

// out_i = base ratio^(set index of i), the set index through GenMap as in k_gen_scalars.  Thread t owns local indices
// [t SPOW_RUN, (t + 1) SPOW_RUN) (fr_pow_run).  The table is an argument: `k` of fr_pow_start is uniform and reads it
// from the argument segment.
template <class Fr>
__global__ void __launch_bounds__(256) k_scalars_powers(uint32_t* out, FrConst base, FrPowTable table, uint32_t n,
                                                        GenMap map) {
  const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * SPOW_RUN;
  if (first >= n) return;
  const uint64_t left = (uint64_t)n - first;
  const uint64_t g = gen_global_index((uint32_t)first, map);
  fr_pow_run<Fr>(out + first * 8, base.w, table, (uint32_t)g, left < SPOW_RUN ? (uint32_t)left : (uint32_t)SPOW_RUN);
}

}  // namespace msmz
#endif

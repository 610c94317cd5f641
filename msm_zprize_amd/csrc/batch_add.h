// Host side of batch_kernels.h: launches of batched-affine additions into one slot array, as a value.  The engine builds
// one per MSM for the tree rounds and hands it to the reduction's batched-affine first level (reduce.h); the
// msmz_test_batch_add hook (test_hooks.h) builds its own.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace msmz {

template <class F>
inline size_t slot_words(uint32_t rec) {   // host twin of slot_offset<F> (rec a multiple of 64)
  return (size_t)(rec >> 6) * (SlotFmt<F>::CH * 64) * 4;
}

template <class Cfg>
struct BatchAdder {
  using F = typename Cfg::F;
  hipStream_t stream;
  uint32_t* slots;     // the slot array: operands named by slot locations, and every result
  uint32_t min_wgs;    // workgroups a launch keeps in flight before its threads take more pairs (MSMZ_BATCH_WGS)
  int b_override;      // > 0: pairs per thread of every launch (MSMZ_BATCH_B)

  // pairs per thread of a launch of `pairs` batched-affine additions: as many as keep >= ~2 workgroups per CU in
  // flight, capped at BMAX = 16 (measured per round at 2^20: 7.6 M pairs B = 8..16, 3.7 M: 16, 1.8 M: 8, 0.9 M: 4,
  // < 0.3 M: 2; 32 is slower everywhere)
  int batch_b(uint32_t pairs) const {
    constexpr int T = MSMZ_BATCH_T, BMAX = MSMZ_BATCH_BMAX;
    int B = 1;
    while (B < BMAX && (uint64_t)pairs >= (uint64_t)T * (B * 2) * min_wgs) B *= 2;
    if (b_override > 0) B = b_override < BMAX ? b_override : BMAX;
    return B;
  }

  // one launch of batched-affine additions: pairs `dsc[0 .. pairs)`, results in slot records out_base + t; B pairs per
  // thread (1 <= B <= MSMZ_BATCH_BMAX; 0: batch_b's choice)
  void launch(uint32_t pairs, bool safe, const uint32_t* d_points, const uint2* dsc, uint32_t out_base, MsmMeta* d_meta,
              int B = 0) const {
    constexpr int T = MSMZ_BATCH_T, OCC = MSMZ_BATCH_OCC, BMAX = MSMZ_BATCH_BMAX;
    if (B == 0) B = batch_b(pairs);
    dim3 grid((pairs + T * B - 1) / (T * B)), block(T);
    if constexpr (!Cfg::TE) {
      if (safe) {
        hipLaunchKernelGGL((k_batch_add<F, T, true, OCC, BMAX>), grid, block, 0, stream, slots, d_points, dsc, out_base,
                           pairs, B, d_meta);
      } else {
        hipLaunchKernelGGL((k_batch_add<F, T, false, OCC, BMAX>), grid, block, 0, stream, slots, d_points, dsc, out_base,
                           pairs, B, d_meta);
      }
    }
  }
};

}  // namespace msmz

// The bucket sort as one host-side stage: scalars -> sorted references + bucket offsets.  BucketSort owns what only the
// sort touches -- its buffers (the outputs included), the two algorithms (the two-level LDS-staged sort of
// sort_kernels.h and the fallback with materialized digits), the dynamic-LDS limits of its kernels and the dispatch over
// their compiled instances -- so its callers (engine.h, test_hooks.h) see run() and four read-only outputs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/msmz.h"
#include "kernels.h"
#include "plan.h"
#include "run.h"
#include "store.h"

namespace msmz {

#ifdef MSMZ_TRACE
constexpr size_t kTraceBytes = 128;   // per workgroup, behind the buffers the traced kernels receive (tools/wg_timeline.py)
// appends one section {name[32], n, n x 16 stamps} to the file MSMZ_TRACE_OUT names (`first` truncates it)
inline int trace_dump(hipStream_t stream, const char* name, const void* d_stamps, uint32_t n_wgs, bool first) {
  const char* path = getenv("MSMZ_TRACE_OUT");
  if (!path) return MSMZ_OK;
  MSMZ_HIP(hipStreamSynchronize(stream));
  std::vector<uint64_t> t((size_t)n_wgs * 16);
  MSMZ_HIP(hipMemcpy(t.data(), d_stamps, t.size() * 8, hipMemcpyDeviceToHost));
  if (FILE* f = fopen(path, first ? "wb" : "ab")) {
    char nm[32] = {};
    strncpy(nm, name, 31);
    const uint64_t n = n_wgs;
    fwrite(nm, 1, 32, f);
    fwrite(&n, 8, 1, f);
    fwrite(t.data(), 8, t.size(), f);
    fclose(f);
  }
  return MSMZ_OK;
}
#else
constexpr size_t kTraceBytes = 0;
#endif

// The three-launch exclusive scan (kernels.h) of n values: out[g] = the sum of v(g') over g' < g, out[n] = the total,
// which also goes to *total_out; *max_out (may be null) is raised to the largest v.  `what` is summed: SCAN_VALUES
// (v(g) = in[g]) or a chunk shift s (v(g) = the chunks of 2^s entries of bucket g, `in` being bucket offsets).
// partials: the scan's scratch, grown as needed.
inline int scan_exclusive(hipStream_t stream, DevBuf& partials, uint32_t* out, const uint32_t* in, uint32_t n, int what,
                          uint32_t* total_out, uint32_t* max_out) {
  const uint32_t nblocks = (n + SCAN_TILE - 1) / SCAN_TILE;
  if (int st = partials.ensure((size_t)nblocks * 4)) return st;
  uint32_t* d_partials = partials.as<uint32_t>();
  hipLaunchKernelGGL(k_scan_partials, dim3(nblocks), dim3(SCAN_T), 0, stream, d_partials, in, n, what);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(SCAN_T), 0, stream, d_partials, nblocks, total_out);
  hipLaunchKernelGGL(k_scan_apply, dim3(nblocks), dim3(SCAN_T), 0, stream, out, d_partials, in, n, what, max_out);
  return MSMZ_OK;
}

// Fr: the scalar field; TE: a twisted-Edwards curve (msmBasic only: neither GLV nor segmented problems).
template <class Fr, bool TE>
class BucketSort {
  static_assert(TE || Fr::HAS_GLV, "the Weierstrass instance list has the GLV kernels");

 public:
  // Kernels that stage more than the default dynamic-LDS allowance get their limit raised ONCE, when the context is
  // created -- not lazily inside the first MSM and not on every MSM.  static + dynamic LDS is checked against the
  // device's per-workgroup LDS, so a kernel that cannot launch fails context creation with its name.
  int init(int device) {
    int st;
    if ((st = raise_lds_limit(device, (const void*)k_fine<false>, "k_fine", kFineLds))) return st;
    if constexpr (!TE) {
      if ((st = raise_lds_limit(device, (const void*)k_fine<true>, "k_fine<seg>", kFineLds))) return st;
    }
    return each_instance([&](auto inst) {
      using I = decltype(inst);
      char name[48];
      snprintf(name, sizeof name, "k_coarse<glv=%d, c=%d, seg=%d>", I::glv, I::c, I::seg);
      if (int st2 = raise_lds_limit(device, (const void*)k_coarse<Fr, I::glv, I::c, I::seg>, name, kCoarseLdsMax)) return st2;
      snprintf(name, sizeof name, "k_hist<glv=%d, c=%d, seg=%d>", I::glv, I::c, I::seg);
      return raise_lds_limit(device, (const void*)k_hist<Fr, I::glv, I::c, I::seg>, name, kHistLdsMax);
    });
  }

  // scalars -> sorted references refs() + bucket offsets off() (+ meta->max_bucket, n_entries, error; the block is reset
  // first); the sort's stage events of `run`.  No host round trip.  pl.nprob > 1 (batched MSM): problem p reads scalars
  // [p n, (p + 1) n); its bins follow problem p - 1's in ONE exclusive scan, so refs / off come out as one dense sort
  // of pl.nprob * nb buckets.  The two-level sort only.
  // `sl`: the planner's sort layout of pl; copy_stride: records per copy of a precomputed point set.
  // d_segs (segmented MSM): problem p's descriptor; d_scalars is then the whole set, pl.n the longest segment.
  int run(const Plan& pl, const SortLayout& sl, const uint32_t* d_scalars, const Run& run, hipStream_t stream,
          MsmMeta* d_meta, uint32_t copy_stride, const SegDesc* d_segs = nullptr) {
    const uint32_t n = pl.n, M = pl.M, nb = pl.nb, P = pl.nprob;
    const int c = pl.c, K = pl.K;
    int st;
    if ((st = refs_.ensure((size_t)P * K * M * 4))) return st;
    if ((st = off_.ensure(((size_t)P * nb + 1) * 4))) return st;
    MSMZ_HIP(hipMemsetAsync(d_meta, 0, sizeof(MsmMeta), stream));
    if (!sl.two_level && (P > 1 || pl.F > 1)) return MSMZ_ERR_ARG;   // (msm_batch only batches plans the two-level sort handles)
    if (d_segs && (TE || !sl.two_level)) return MSMZ_ERR_ARG;         // (run_segments: the batched pipeline only)
    const uint32_t nbins = sl.nbins, fbins = sl.fbins;
    const uint32_t n_half = pl.glv ? n : 0xffffffffu;
    if (sl.two_level) {
      const SortGeom& g = sl.geom;
      const size_t pbins = (size_t)P * g.sbins;   // bins of all problems
      if ((st = packed_.ensure((size_t)P * K * M * 4))) return st;
      if ((st = bins_.ensure((pbins + 2) * 4 + kTraceBytes * pbins))) return st;
      if ((st = counts_.ensure(pbins * 4))) return st;
      uint32_t* d_counts = counts_.as<uint32_t>();
      MSMZ_HIP(hipMemsetAsync(d_counts, 0, pbins * 4, stream));
      run.mark(run.ev.sort0, stream);
      const uint32_t per_tile = pl.glv ? COARSE_TILE / 2 : COARSE_TILE;   // scalars per workgroup (k_hist and k_coarse)
      const uint32_t tiles = (n + per_tile - 1) / per_tile;
      if ((st = tilecnt_.ensure((size_t)P * tiles * nbins * 2))) return st;
      if ((st = tileoff_.ensure((size_t)P * tiles * nbins * 4 + kTraceBytes * tiles))) return st;   // the tiles' runs inside the bins
      // k_hist (coarse = false) or k_coarse of the instance (pl.glv, sl.cspec, d_segs); a plan without one is an error
      auto launch_sort = [&](bool coarse) {
        bool launched = false;
        each_instance([&](auto inst) {
          using I = decltype(inst);
          if (I::glv != pl.glv || I::c != sl.cspec || I::seg != (d_segs != nullptr)) return MSMZ_OK;
          launched = true;
          if (!coarse)
            hipLaunchKernelGGL((k_hist<Fr, I::glv, I::c, I::seg>), dim3(tiles, P), dim3(COARSE_T), (size_t)nbins * 4, stream,
                               d_counts, tilecnt_.as<uint16_t>(), tileoff_.as<uint32_t>(), d_meta, d_scalars, g, nbins, d_segs);
          else   // dynamic LDS <= kCoarseLdsMax (nbins <= SORT_MAX_BINS): the limit init() raised
            hipLaunchKernelGGL((k_coarse<Fr, I::glv, I::c, I::seg>), dim3(tiles, P), dim3(COARSE_T), (size_t)2 * nbins * 4,
                               stream, packed_.as<uint32_t>(), tileoff_.as<uint32_t>(), bins_.as<uint32_t>(),
                               tilecnt_.as<uint16_t>(), d_scalars, g, nbins, d_segs);
          return MSMZ_OK;
        });
        return launched ? MSMZ_OK : MSMZ_ERR_ARG;
      };
      if ((st = launch_sort(false))) return st;
      run.mark(run.ev.hist_end, stream);
      MSMZ_HIP(hipGetLastError());
      if (pbins <= (size_t)SORT_MAX_BINS) {
        hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(1024), 0, stream, bins_.as<uint32_t>(), d_counts, (uint32_t)pbins,
                           &d_meta->n_entries);
      } else {   // a batch with more bins than one workgroup scans
        if ((st = scan_exclusive(stream, partials_, bins_.as<uint32_t>(), d_counts, (uint32_t)pbins, SCAN_VALUES,
                                 &d_meta->n_entries, nullptr)))
          return st;
      }
      run.mark(run.ev.scan_end, stream);
      MSMZ_HIP(hipGetLastError());
      if ((st = launch_sort(true))) return st;
      run.mark(run.ev.coarse_end, stream);
      MSMZ_HIP(hipGetLastError());
      auto launch_fine = [&](auto seg) {
        hipLaunchKernelGGL(k_fine<decltype(seg)::value>, dim3(fbins, P), dim3(FINE_T), kFineLds, stream, refs_.as<uint32_t>(),
                           off_.as<uint32_t>(), &d_meta->max_bucket, packed_.as<uint32_t>(), bins_.as<uint32_t>(), g.fb, g.fbt,
                           sl.fine_top, fbins, g.idx_bits, n_half, pl.endo_delta, g.F, g.mbits, copy_stride, d_segs);
      };
      if constexpr (!TE) {
        if (d_segs) launch_fine(std::true_type{});
      }
      if (!d_segs) launch_fine(std::false_type{});
#ifdef MSMZ_TRACE
      // development aid: workgroup time stamps of k_coarse / k_fine (tools/wg_timeline.py)
      if ((st = trace_dump(stream, "k_coarse", tileoff_.as<uint32_t>() + (size_t)P * tiles * nbins, tiles, true))) return st;
      if ((st = trace_dump(stream, "k_fine", bins_.as<uint32_t>() + ((P * g.sbins + 2) & ~1u), fbins, false))) return st;
#endif
    } else {
      // fallback (window sizes whose coarse bins do not fit the LDS staging): digits materialized, one global
      // atomic per entry
      if (pl.fold_shift != 0) return MSMZ_ERR_ARG;   // (make_plan only folds when the two-level sort applies)
      if ((st = digits_.ensure((size_t)K * M * 4))) return st;
      if ((st = counts_.ensure(((size_t)nb + 1) * 4))) return st;
      if ((st = cursor_.ensure((size_t)nb * 4))) return st;
      MSMZ_HIP(hipMemsetAsync(counts_.p, 0, ((size_t)nb + 1) * 4, stream));
      MSMZ_HIP(hipMemsetAsync(cursor_.p, 0, (size_t)nb * 4, stream));
      const uint32_t dgrid = (n + 256 * DIGITS_ITEMS - 1) / (256 * DIGITS_ITEMS);
      run.mark(run.ev.sort0, stream);
      auto launch_digits = [&](auto glv) {
        hipLaunchKernelGGL((k_digits<Fr, decltype(glv)::value>), dim3(dgrid), dim3(256), 0, stream, digits_.as<uint32_t>(),
                           counts_.as<uint32_t>(), d_meta, d_scalars, n, c, K, pl.spread, pl.sbits ? pl.sbits : 256);
      };
      if constexpr (Fr::HAS_GLV) {
        if (pl.glv) launch_digits(std::true_type{});
      }
      if (!pl.glv) launch_digits(std::false_type{});
      run.mark(run.ev.hist_end, stream);
      MSMZ_HIP(hipGetLastError());
      if ((st = scan_exclusive(stream, partials_, off_.as<uint32_t>(), counts_.as<uint32_t>(), nb, SCAN_VALUES,
                               &d_meta->n_entries, &d_meta->max_bucket)))
        return st;
      run.mark(run.ev.scan_end, stream);
      MSMZ_HIP(hipGetLastError());
      {
        dim3 grid((M + 256 * 4 - 1) / (256 * 4), K);
        hipLaunchKernelGGL(k_scatter, grid, dim3(256), 0, stream, refs_.as<uint32_t>(), cursor_.as<uint32_t>(),
                           off_.as<uint32_t>(), digits_.as<uint32_t>(), M, c, pl.spread, n_half, pl.endo_delta);
      }
      run.mark(run.ev.coarse_end, stream);
      MSMZ_HIP(hipGetLastError());
    }
    run.mark(run.ev.sort_end, stream);
    MSMZ_HIP(hipGetLastError());
    return MSMZ_OK;
  }

  // the outputs of the last run(): the sorted references, the bucket offsets; two-level sort: the bin scan, the packed words
  const uint32_t* refs() const { return refs_.as<uint32_t>(); }
  const uint32_t* off() const { return off_.as<uint32_t>(); }
  const uint32_t* bins() const { return bins_.as<uint32_t>(); }
  const uint32_t* packed() const { return packed_.as<uint32_t>(); }

  // f(buffer) for every device buffer of the stage: all scratch, undefined at the start of every run()
  template <class Fn>
  void each_scratch(Fn f) {
    f(packed_), f(bins_), f(counts_), f(tilecnt_), f(tileoff_), f(digits_), f(cursor_), f(refs_), f(off_), f(partials_);
  }

 private:
  // dynamic LDS the sort kernels may be launched with (run() never asks for more: SORT_MAX_BINS caps nbins)
  static constexpr size_t kFineLds = ((size_t)(1 << FINE_MAX_BITS) + FINE_STAGE) * 4;
  static constexpr size_t kCoarseLdsMax = (size_t)2 * SORT_MAX_BINS * 4;
  static constexpr size_t kHistLdsMax = (size_t)SORT_MAX_BINS * 4;

  template <bool GLV, int C, bool SEG>
  struct Instance {
    static constexpr bool glv = GLV, seg = SEG;
    static constexpr int c = C;
  };
  // f(Instance) for every compiled instance of k_hist / k_coarse (the list: sort_kernels.h), until one returns non-zero
  template <class Fn>
  static int each_instance(Fn f) {
    int st;
#define MSMZ_X(f, GLV, C, SEG) \
  if ((st = f(Instance<GLV, C, SEG>{}))) return st;
    MSMZ_SORT_INSTANCES(MSMZ_X, f)
    if constexpr (!TE) {
      MSMZ_SORT_INSTANCES_WEIERSTRASS(MSMZ_X, f)
    }
#undef MSMZ_X
    return MSMZ_OK;
  }

  static int raise_lds_limit(int device, const void* fn, const char* name, size_t dyn_max) {
    hipFuncAttributes fa;
    memset(&fa, 0, sizeof(fa));
    MSMZ_HIP(hipFuncGetAttributes(&fa, fn));
    hipDeviceProp_t prop;
    MSMZ_HIP(hipGetDeviceProperties(&prop, device));
    // per-workgroup LDS of the device: gfx950 reports 160 KiB as the opt-in maximum (64 KiB is the default allowance)
    size_t dev_max = prop.sharedMemPerBlock;
    if (prop.sharedMemPerBlockOptin > dev_max) dev_max = prop.sharedMemPerBlockOptin;
    if (prop.maxSharedMemoryPerMultiProcessor > dev_max) dev_max = prop.maxSharedMemoryPerMultiProcessor;
    if (fa.sharedSizeBytes + dyn_max > dev_max) {
      fprintf(stderr, "msmz: %s needs %zu B static + %zu B dynamic LDS, the device offers %zu B per workgroup\n", name,
              (size_t)fa.sharedSizeBytes, dyn_max, dev_max);
      return MSMZ_ERR_HIP;
    }
    MSMZ_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_max));
    return MSMZ_OK;
  }

  DevBuf packed_, bins_, counts_, tilecnt_, tileoff_, digits_, cursor_, refs_, off_, partials_;
};

}  // namespace msmz

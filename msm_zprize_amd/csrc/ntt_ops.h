// Number-theoretic transforms over resident scalar sets, as one stage: the passes of a plan (ntt_plan.h), the tables of
// powers they read, and the cache of twiddle tables.  NttOps owns ntt_scratch_, ntt_coset_ and the cache; it reaches the
// engine through the SetsCore it is built with (sets_core.h) and fills its tables through ScalarOps::launch_powers
// (scalar_ops.h).  ResidentSets (resident.h) forwards the IEngine method here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <deque>

#include "../../include/msmz.h"
#include "ntt_kernels.h"
#include "scalar_ops.h"
#include "sets_core.h"

namespace msmz {

template <class Cfg>
class NttOps {
  using Core = SetsCore<Cfg>;
  using Fr = typename Cfg::Fr;

 public:
  NttOps(Core& core, ScalarOps<Cfg>& scalars) : core_(core), scalars_(scalars) {}

  // f(buffer) for every scratch buffer of the stage: undefined at the start of every call.  (Not the cached twiddle
  // tables: they stay valid across calls, and are bound to the engine's Poison when they are built.)
  template <class Fn>
  void each_scratch(Fn f) {
    f(ntt_scratch_), f(ntt_coset_);
  }

  // msmz_scalars_ntt: one launch per pass of the plan (ntt_plan.h), in stream order, from the source through scratch to
  // the destination; the error word (a resident record >= q, raised by the first pass) comes back behind the ONE host
  // wait.  Twiddle tables: built on the device by k_scalars_powers in the same stream, cached per (log_n, root as used).
  int scalars_ntt(const msmz_ntt& t, uint64_t first_out, uint64_t* out_handle) {
    const bool inverse = t.flags & MSMZ_NTT_INVERSE, coset = t.flags & MSMZ_NTT_COSET;
    if (!out_handle || t.count == 0 || (t.flags & ~(uint32_t)(MSMZ_NTT_INVERSE | MSMZ_NTT_COSET)) || coset != (t.shift != nullptr))
      return MSMZ_ERR_ARG;
    if (t.log_n > (uint32_t)Fr::TWO_ADICITY) return MSMZ_ERR_UNSUPPORTED;
    if (t.log_n >= 32) return MSMZ_ERR_ARG;
    const uint64_t n = 1ull << t.log_n, total = n * t.count, n_in = t.n_in ? t.n_in : n;
    if (total >> 32 || n_in > n || (inverse && n_in != n)) return MSMZ_ERR_ARG;
    const uint32_t* X = nullptr;
    uint32_t* out = nullptr;
    if (int st = core_.resolve({{t.handle, t.first, &X, n_in * t.count}}, total, first_out, *out_handle, &out)) return st;
    uint32_t w[8], g[8];
    if (t.root) {
      if (int st = Core::read_fr(t.root, w, false)) return st;
      if (!fr_is_primitive_root<Fr>(w, t.log_n)) return MSMZ_ERR_ARG;
    } else {
      fr_root_of_unity<Fr>(w, t.log_n);
    }
    if (coset) {
      if (int st = Core::read_fr(t.shift, g, false)) return st;
      uint32_t any = 0;
      for (int j = 0; j < 8; j++) any |= g[j];
      if (!any) return MSMZ_ERR_ARG;
    }
    NttCall call{};
    call.plan = ntt_plan(t.log_n);
    call.inverse = inverse;
    call.n_in = n_in;
    call.count = t.count;
    if (inverse) {   // the inverse root, n^-1 and g^-1: three host inversions
      uint32_t nn[8] = {};
      nn[t.log_n >> 5] = 1u << (t.log_n & 31);
      fr_inv<Fr>(nn, nn);
      fr_to_mont<Fr>(call.ninv.w, nn);
      fr_inv<Fr>(w, w);
      if (coset) fr_inv<Fr>(g, g);
    }
    MSMZ_HIP(hipSetDevice(core_.device_));
    const uint32_t P = call.plan.n_passes;
    // every allocation first: once a table build is queued nothing below returns before the stream is drained
    NttTableSpec lo, hi;
    if (coset) ntt_two_level_specs<Fr>(call.plan, g, inverse ? call.ninv.w : Fr::ONE, &lo, &hi);
    if (int st = ntt_scratch_.ensure((size_t)(P > 2 ? 2 : P - 1) * total * 32)) return st;
    if (coset)
      if (int st = ntt_coset_.ensure((size_t)(lo.count + hi.count) * 32)) return st;
    Handle hd;
    if (int st = core_.fresh_out(total, &hd, &out)) return st;
    if (int st = ntt_twiddles(call.plan, w, &call.twiddles)) return st;
    if (coset) {
      fill(ntt_coset_.as<uint32_t>(), lo);
      fill(ntt_coset_.as<uint32_t>() + lo.count * 8, hi);
      call.coset = ntt_coset_.as<const uint32_t>();
    }
    const int st = core_.checked([&](uint32_t* d_err) {   // a resident record >= group order (the first pass: bit 2)
      call.err = d_err;
      uint32_t* scratch[2] = {ntt_scratch_.as<uint32_t>(), ntt_scratch_.as<uint32_t>() + (size_t)total * 8};
      const uint32_t* src = X;
      uint64_t stride = n_in;
      for (uint32_t j = 0; j < P; j++) {
        uint32_t* dst = j + 1 == P ? out : scratch[j & 1];
        const NttArgs a = ntt_pass_args(call, j, src, stride, dst);
        const dim3 grid(ntt_pass_tiles(a.pass), t.count < NTT_GRID_VECTORS ? t.count : NTT_GRID_VECTORS);
        hipLaunchKernelGGL((k_ntt_pass<Fr>), grid, dim3(NTT_THREADS), 0, core_.stream_, a);
        src = dst;
        stride = n;
      }
    });
    return st || !hd.mem.p ? st : core_.add_handle(std::move(hd), out_handle);
  }

  uint64_t test_ntt_tables() const { return ntt_built_; }

 private:
  // a table of powers (ntt_kernels.h) into device memory, queued on the stream
  void fill(uint32_t* dst, const NttTableSpec& s) {
    FrConst base;
    memcpy(base.w, s.base, 32);
    scalars_.launch_powers(dst, base, s.ratio, s.count, GenMap{});
  }

  // *tables = the three twiddle tables of `plan` for the root w (the inverse root of an inverse transform), from the
  // cache or built now.  At most NTT_CACHE sets are kept, the oldest goes first; all are freed with the engine.
  struct NttTwiddles {
    uint32_t log_n;
    uint32_t w[8];
    DevBuf mem;
  };
  int ntt_twiddles(const NttPlan& plan, const uint32_t* w, const uint32_t** tables) {
    for (const NttTwiddles& c : ntt_cache_) {
      if (c.log_n == plan.log_n && !memcmp(c.w, w, 32)) {
        *tables = c.mem.template as<const uint32_t>();
        return MSMZ_OK;
      }
    }
    NttTwiddles c;
    c.mem.poison = &core_.poison_;
    c.log_n = plan.log_n;
    memcpy(c.w, w, 32);
    if (int st = c.mem.ensure((size_t)ntt_twiddle_entries(plan) * 32)) return st;
    NttTableSpec spec[3];
    ntt_twiddle_specs<Fr>(plan, w, spec);
    uint32_t* at = c.mem.template as<uint32_t>();
    for (int k = 0; k < 3; k++) {
      fill(at, spec[k]);
      at += spec[k].count * 8;
    }
    // (no wait on the way through: the transform's own is the one wait.  A failed launch drains what was queued, and c
    // frees its memory)
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return core_.wait_after(e);
    ntt_built_++;
    if (ntt_cache_.size() == NTT_CACHE) {
      // (the set that leaves may still be read by a transform in flight only if the stream has work: every entry point
      // returns with the stream drained, so it has none)
      ntt_cache_.pop_front();
    }
    ntt_cache_.push_back(std::move(c));
    *tables = ntt_cache_.back().mem.template as<const uint32_t>();
    return MSMZ_OK;
  }

  Core& core_;
  ScalarOps<Cfg>& scalars_;
  DevBuf ntt_scratch_;                 // one or two copies of the batch between the passes of a plan
  DevBuf ntt_coset_;                   // the two-level powers of the coset shift of the call in progress
  std::deque<NttTwiddles> ntt_cache_;  // the twiddle tables of the last NTT_CACHE (log_n, root) pairs
  uint64_t ntt_built_ = 0;             // ... the sets built so far (msmz_test_ntt_tables)
};

}  // namespace msmz

// Host-side MSM engine: owns the device buffers of one GPU, sequences the kernels on one HIP stream
// and finishes the K window sums on the host.  This replaces the reference's SPMD worker runtime
// (src/threads/threads.ts:132-359, src/parallel.ts:291-320) and the JS orchestration inside
// `msm` (src/msm-batched-affine.ts:74-328): barriers between phases become stream order, the
// per-thread bucket split (msm-common.ts:88-188) becomes grid sizing.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>
#include <vector>

#include "../../include/msmz.h"
#include "kernels.h"
#include "gen_kernels.h"
#include "import_kernels.h"
#include "check_kernels.h"
#include "mul_kernels.h"
#include "scalar_kernels.h"
#include "host64.h"
#include "multi.h"
#include "plan.h"

namespace msmz {

#define MSMZ_HIP(x)                                                                        \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      fprintf(stderr, "msmz: HIP error '%s' from `%s` at %s:%d\n", hipGetErrorString(e_), #x, __FILE__, __LINE__); \
      return MSMZ_ERR_HIP;                                                                 \
    }                                                                                      \
  } while (0)

// Device memory owned by one object: freed when it goes out of scope, so every error path releases it.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, bytes = o.bytes;
      o.p = nullptr, o.bytes = 0;
    }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  int ensure(size_t need) {   // grow-only
    if (need <= bytes) return MSMZ_OK;
    release();
    size_t sz = need + need / 8;
    if (hipMalloc(&p, sz) != hipSuccess) {
      if (hipMalloc(&p, need) != hipSuccess) return MSMZ_ERR_HIP;
      sz = need;
    }
    bytes = sz;
    return MSMZ_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

struct Handle {
  int kind;        // 0 = points, 1 = scalars
  uint64_t n;
  bool has_endo;   // points: records [n, 2n) hold the endomorphism images
  DevBuf mem;
  // precomputed point set (msmz_precompute_points): `factor` copies, copy j = records [j R, (j + 1) R) holds 2^(c j) P_i
  // (R = copy_stride = n, or 2 n with the endomorphism images); built for window size c and GLV choice glv.  0 = plain.
  uint32_t factor = 0;
  int c = 0, glv = 0;
  uint64_t copy_stride = 0;
  int sbits = 0;   // scalar bit bound the copies were built for (Planner::bound: 0 = none)
};

// Named events of an MSM's stages, created once per engine; a timed MSM records them in stream order.
struct StageEvents {
  hipEvent_t sort0, hist_end, scan_end, coarse_end, sort_end;   // sort: digits / histogram, scan, scatter
  hipEvent_t plan0, plan_end;                                    // plan (incl. its host round trip)
  hipEvent_t round_end[32];                                      // tree round r (recorded for non-empty rounds)
  hipEvent_t acc_end, red_end;                                   // accumulation, bucket reduction
  std::vector<hipEvent_t*> all() {
    std::vector<hipEvent_t*> v{&sort0, &hist_end, &scan_end, &coarse_end, &sort_end, &plan0, &plan_end, &acc_end, &red_end};
    for (hipEvent_t& e : round_end) v.push_back(&e);
    return v;
  }
};

// One MSM call's run state, beside its Plan (the planner's output): whether it is timed, its stage events, and the
// device totals fetch_meta reads back.  n_pairs: the additions of the accumulation (the tree rounds' pairs; msmBasic:
// the entries).
struct Run {
  bool timing = false;
  StageEvents ev{};
  uint32_t max_bucket = 0, n_entries = 0, rounds = 0;
  uint32_t round_pairs[32] = {}, round_base[32] = {};
  uint64_t n_pairs = 0;
};

// What an MSM attempt asks of its caller besides its status: nothing, the same MSM again with windows for the proven
// GLV bound (a GLV half was longer than assumed), or this sub-batch's problems one by one (its plan does not batch).
enum class Redo { NONE, PROVEN_BITS, PER_PROBLEM };

// Host-side group addition of two canonical affine points (msmz_point_add; fold_partial, multi.h, folds partial MSM
// results with it).
template <class F, bool TE>
static int host_point_add(const uint8_t* a, int ai, const uint8_t* b, int bi, uint8_t* out, int* oi) {
  constexpr int NW = F::NW;
  if constexpr (TE) {
    auto load = [](TeExt<F>& p, const uint8_t* xy) {
      uint32_t w[2 * NW];
      memcpy(w, xy, sizeof(w));
      Fe<F> x, y;
      fe_unpack<F>(x, w);
      fe_unpack<F>(y, w + NW);
      fe_to_mont(p.X, x);
      fe_to_mont(p.Y, y);
      fe_set_const<F>(p.Z, F::ONE);
      fe_mul(p.T, p.X, p.Y);
    };
    if (!a || !b) return MSMZ_ERR_ARG;   // twisted Edwards has no infinity flag: the identity is (0, 1)
    TeExt<F> p, q, r;
    load(p, a);
    load(q, b);
    te_add(r, p, q);
    uint32_t w[2 * NW];
    te_to_affine_canon<F>(w, r);
    memcpy(out, w, sizeof(w));
    *oi = 0;
  } else {
    auto load = [](Xyzz<F>& p, const uint8_t* xy, int inf) {
      if (inf) {
        xyzz_set_inf(p);
        return;
      }
      uint32_t w[2 * NW];
      memcpy(w, xy, sizeof(w));
      Affine<F> t, m;
      fe_unpack<F>(t.x, w);
      fe_unpack<F>(t.y, w + NW);
      fe_to_mont(m.x, t.x);
      fe_to_mont(m.y, t.y);
      xyzz_from_affine(p, m);
    };
    Xyzz<F> p, q, r;
    load(p, a, ai);
    load(q, b, bi);
    xyzz_add(r, p, q);
    uint32_t w[2 * NW];
    bool inf = xyzz_to_affine_canon<F>(w, r);
    memcpy(out, w, sizeof(w));
    *oi = inf ? 1 : 0;
  }
  return MSMZ_OK;
}

// Which kernel a level of the bucket reduction runs; none changes a result.  The engine holds one, constant, which the
// MSM paths pass to the reduction; a test hook passes a copy with its caller's values.
struct ReduceKnobs {
  uint32_t tail_n;           // entries per window at which k_reduce_tail takes over
  uint32_t quad16_max;       // levels with at most this many groups use k_reduce_quad16
  uint32_t pairsum_x4_max;   // pair-sum levels with at most this many additions use DPP quads
};

template <class Cfg>
class TestHooks;   // test_hooks.h

template <class Cfg>
class Engine : public IEngine {
  friend class TestHooks<Cfg>;
  using F = typename Cfg::F;
  using Fr = typename Cfg::Fr;
  static constexpr int NW = F::NW;
  static constexpr int RW = 2 * NW;      // affine record words
  static constexpr int XW = 4 * NW;      // XYZZ / extended record words
  static constexpr int FE_BYTES = NW * 4;
  static constexpr bool TE = Cfg::TE;
  static constexpr int PW_WORDS = TE ? 4 * NW : PointFmt<F>::STRIDE;   // words between the records of a resident point set

 public:
  Engine(int curve_id, int device) : curve_id_(curve_id), device_(device) {}

  int init() {
    MSMZ_HIP(hipSetDevice(device_));
    MSMZ_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    for (hipEvent_t* e : ev_.all()) MSMZ_HIP(hipEventCreate(e));
    MSMZ_HIP(hipEventCreateWithFlags(&import_ev_, hipEventDisableTiming));
    MSMZ_HIP(hipHostMalloc(&h_meta_, sizeof(MsmMeta)));
    int st;
    if ((st = ensure_host_results((size_t)2 * kMaxWindows * XW))) return st;   // the results of one problem
    // Kernels that stage more than the default dynamic-LDS allowance get their limit raised ONCE, here, right after
    // hipSetDevice -- not lazily inside the first MSM and not on every MSM.  static + dynamic LDS is checked against
    // the device's per-workgroup LDS, so a kernel that cannot launch fails context creation with its name.
    if ((st = raise_lds_limit((const void*)k_fine, "k_fine", kFineLds))) return st;
    if constexpr (!TE) {
      if ((st = raise_lds_limit((const void*)k_fine_seg, "k_fine_seg", kFineLds))) return st;
    }
    if ((st = raise_sort_limits<false, 0>()) || (st = raise_sort_limits<false, 16>()) || (st = raise_sort_limits<false, 17>())) return st;
    if constexpr (Fr::HAS_GLV) {
      if ((st = raise_sort_limits<true, 0>()) || (st = raise_sort_limits<true, 16>())) return st;
    }
    return meta_.ensure(sizeof(MsmMeta) + kTraceBytes * 65536);
  }
 private:
  template <bool GLV, int C>
  int raise_sort_limits() {
    int st;
    if ((st = raise_lds_limit((const void*)k_coarse<Fr, GLV, C>, GLV ? "k_coarse<glv>" : "k_coarse", kCoarseLdsMax))) return st;
    if ((st = raise_lds_limit((const void*)k_hist<Fr, GLV, C>, GLV ? "k_hist<glv>" : "k_hist", kHistLdsMax))) return st;
    if constexpr (!TE) {   // the segmented variants (msm_segments: the batched pipeline is Weierstrass only)
      if ((st = raise_lds_limit((const void*)k_coarse_seg<Fr, GLV, C>, GLV ? "k_coarse_seg<glv>" : "k_coarse_seg", kCoarseLdsMax))) return st;
      if ((st = raise_lds_limit((const void*)k_hist_seg<Fr, GLV, C>, GLV ? "k_hist_seg<glv>" : "k_hist_seg", kHistLdsMax))) return st;
    }
    return MSMZ_OK;
  }
  // dynamic LDS the sort kernels may be launched with (sort_phase never asks for more: SORT_MAX_BINS caps nbins)
  static constexpr size_t kFineLds = ((size_t)(1 << FINE_MAX_BITS) + FINE_STAGE) * 4;
  static constexpr size_t kCoarseLdsMax = (size_t)2 * SORT_MAX_BINS * 4;
  static constexpr size_t kHistLdsMax = (size_t)SORT_MAX_BINS * 4;
#ifdef MSMZ_TRACE
  static constexpr size_t kTraceBytes = 128;   // per workgroup, behind the buffers the sort kernels receive (tools/wg_timeline.py)
#else
  static constexpr size_t kTraceBytes = 0;
#endif

#ifdef MSMZ_TRACE
  // appends one section {name[32], n, n x 16 stamps} to the file MSMZ_TRACE_OUT names (`first` truncates it)
  int trace_dump(const char* name, const void* d_stamps, uint32_t n_wgs, bool first) {
    const char* path = getenv("MSMZ_TRACE_OUT");
    if (!path) return MSMZ_OK;
    MSMZ_HIP(hipStreamSynchronize(stream_));
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
#endif

  int raise_lds_limit(const void* fn, const char* name, size_t dyn_max) {
    hipFuncAttributes fa;
    memset(&fa, 0, sizeof(fa));
    MSMZ_HIP(hipFuncGetAttributes(&fa, fn));
    hipDeviceProp_t prop;
    MSMZ_HIP(hipGetDeviceProperties(&prop, device_));
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

 public:
  ~Engine() override {   // (the device buffers and handles free themselves after this, on this device)
    (void)hipSetDevice(device_);
    if (h_meta_) (void)hipHostFree(h_meta_);
    if (h_res_) (void)hipHostFree(h_res_);
    if (h_check_) (void)hipHostFree(h_check_);
    if (h_segs_) (void)hipHostFree(h_segs_);
    for (hipEvent_t* e : ev_.all())
      if (*e) (void)hipEventDestroy(*e);
    if (import_ev_) (void)hipEventDestroy(import_ev_);
    if (stream_) (void)hipStreamDestroy(stream_);
  }

  // ------------------------------------------------------------------------------------------ data
  int upload_points(const uint8_t* xy, const uint8_t* inf, uint64_t n, uint64_t* h, const GenMap* split = nullptr) override {
    if (!xy || !h || n == 0 || n >= (1ull << (Cfg::HAS_ENDO ? 29 : 30))) return MSMZ_ERR_ARG;   // record indices (incl. endomorphism images) fit 30 bits
    MSMZ_HIP(hipSetDevice(device_));
    int st = stage_.ensure(n * RW * 4 + n);
    if (st) return st;
    if ((st = copy_h2d(stage_.p, xy, (size_t)RW * 4, n, split))) return st;
    uint8_t* d_inf = nullptr;
    if (inf) {
      d_inf = stage_.as<uint8_t>() + n * RW * 4;
      if ((st = copy_h2d(d_inf, inf, 1, n, split))) return st;
    }
    const bool endo = Cfg::HAS_ENDO;
    Handle hd{0, n, endo};
    if ((st = alloc_handle(hd, (size_t)n * PW_WORDS * 4 * (endo ? 2 : 1)))) return st;
    MsmMeta* d_meta = meta_.as<MsmMeta>();
    MSMZ_HIP(hipMemsetAsync(&d_meta->error, 0, 4, stream_));
    if constexpr (TE) {
      hipLaunchKernelGGL((k_te_points_to_niels<F>), dim3((n + 255) / 256), dim3(256), 0, stream_, hd.mem.as<uint32_t>(),
                         stage_.as<uint32_t>(), (uint32_t)n, &d_meta->error);
    } else {
      hipLaunchKernelGGL((k_points_to_mont<F>), dim3((n + 255) / 256), dim3(256), 0, stream_, hd.mem.as<uint32_t>(),
                         stage_.as<uint32_t>(), d_inf, (uint32_t)n, endo ? 1 : 0, &d_meta->error);
    }
    uint32_t err = 0;
    if ((st = fetch_error(&err))) return st;
    if (err) return MSMZ_ERR_RANGE;   // a coordinate >= p
    return add_handle(std::move(hd), h);
  }

  int upload_scalars(const uint8_t* s, uint64_t n, uint64_t* h, const GenMap* split = nullptr) override {
    if (!s || !h || n == 0) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd{1, n, false};
    int st;
    if ((st = alloc_handle(hd, n * 32)) || (st = copy_h2d(hd.mem.p, s, 32, n, split))) return st;
    MsmMeta* d_meta = meta_.as<MsmMeta>();
    MSMZ_HIP(hipMemsetAsync(&d_meta->error, 0, 4, stream_));
    hipLaunchKernelGGL((k_check_scalars<Fr>), dim3((n + 255) / 256), dim3(256), 0, stream_, &d_meta->error,
                       hd.mem.as<const uint32_t>(), (uint32_t)n);
    uint32_t err = 0;
    if ((st = fetch_error(&err))) return st;
    if (err) return MSMZ_ERR_RANGE;   // a scalar >= group order
    return add_handle(std::move(hd), h);
  }

  // ------------------------------------------------------------------------------------------ imports
  int import_scalars(const msmz_src& s, uint64_t n, uint64_t* h, const GenMap* split = nullptr) override {
    if (!h || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd{1, n, false};
    ImportView v;
    int st;
    {
      uint32_t w = 0;
      uint64_t sb = 0;
      if ((st = src_check(&s, 0, &w, &sb))) return st;
    }
    if ((st = alloc_handle(hd, n * 32)) || (st = import_view(s, 0, n, split, &v))) return st;   // (allocate first: no copy is queued yet)
    if ((st = import_scalars_to(hd.mem.as<uint32_t>(), s, v, n))) return st;
    return add_handle(std::move(hd), h);
  }

  // a new scalar set of n zeros: the target of import_scalars_into when a batch is assembled vector by vector
  int alloc_scalars(uint64_t n, uint64_t* h) override {
    if (!h || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd{1, n, false};
    if (int st = alloc_handle(hd, n * 32)) return st;
    MSMZ_HIP(hipMemsetAsync(hd.mem.p, 0, n * 32, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return add_handle(std::move(hd), h);
  }

  int import_scalars_into(uint64_t h, uint64_t first, const msmz_src& s, uint64_t n) override {
    auto it = handles_.find(h);
    if (it == handles_.end() || it->second.kind != 1 || n == 0) return MSMZ_ERR_ARG;
    if (first > it->second.n || n > it->second.n - first) return MSMZ_ERR_ARG;   // (no first + n: it can wrap)
    MSMZ_HIP(hipSetDevice(device_));
    ImportView v;
    if (int st = import_view(s, 0, n, nullptr, &v)) return st;
    return import_scalars_to(it->second.mem.template as<uint32_t>() + first * 8, s, v, n);
  }

  int import_points(const msmz_src& s, uint64_t n, uint64_t* h, const GenMap* split = nullptr) override {
    if (!h || n == 0 || n >= (1ull << (Cfg::HAS_ENDO ? 29 : 30))) return MSMZ_ERR_ARG;   // as upload_points
    MSMZ_HIP(hipSetDevice(device_));
    ImportView v;
    int st;
    const bool endo = Cfg::HAS_ENDO;
    const int mont = (s.flags & MSMZ_SRC_MONTGOMERY) ? 1 : 0;
    Handle hd{0, n, endo};
    {   // (checked before the allocation, which comes before any copy is queued)
      uint32_t w = 0;
      uint64_t sb = 0;
      if ((st = src_check(&s, FE_BYTES, &w, &sb))) return st;
    }
    if ((st = alloc_handle(hd, (size_t)n * PW_WORDS * 4 * (endo ? 2 : 1))) || (st = import_view(s, FE_BYTES, n, split, &v))) return st;
    MsmMeta* d_meta = meta_.as<MsmMeta>();
    MSMZ_HIP(hipMemsetAsync(&d_meta->error, 0, 4, stream_));
    if constexpr (TE) {
      hipLaunchKernelGGL((k_te_import_points<F>), dim3((n + 255) / 256), dim3(256), 0, stream_, hd.mem.as<uint32_t>(),
                         v.ptr, v.stride, (uint32_t)n, mont, &d_meta->error);
    } else {
      hipLaunchKernelGGL((k_import_points<F>), dim3((n + 255) / 256), dim3(256), 0, stream_, hd.mem.as<uint32_t>(), v.ptr,
                         v.stride, v.is_inf, (uint32_t)n, endo ? 1 : 0, mont, &d_meta->error);
    }
    uint32_t err = 0;
    if ((st = fetch_error(&err))) return st;
    if (err) return MSMZ_ERR_RANGE;   // a coordinate (either form) >= p
    return add_handle(std::move(hd), h);
  }

  int gather_src(const msmz_src& s, int point_fe_bytes, uint64_t n, std::vector<uint8_t>* recs,
                 std::vector<uint8_t>* flags) override {
    uint32_t width = 0;
    uint64_t stride = 0;
    if (int st = src_check(&s, point_fe_bytes, &width, &stride)) return st;
    if (n == 0 || n >> 32 || !recs || !flags) return MSMZ_ERR_ARG;
    recs->resize((size_t)n * width);
    flags->clear();
    const uint8_t* p = (const uint8_t*)s.ptr;
    if (!(s.flags & MSMZ_SRC_DEVICE)) {
      for (uint64_t i = 0; i < n; i++) memcpy(recs->data() + i * width, p + i * stride, width);
      if (s.is_inf) flags->assign(s.is_inf, s.is_inf + n);
      return MSMZ_OK;
    }
    MSMZ_HIP(hipSetDevice(device_));
    const void* dp = nullptr;
    const void* di = nullptr;
    int st;
    if ((st = vouch(p, (n - 1) * stride + width, true, &dp))) return st;
    if (s.is_inf && (st = vouch(s.is_inf, n, true, &di))) return st;
    if (s.stream) MSMZ_HIP(hipStreamSynchronize((hipStream_t)s.stream));
    if (s.flags & MSMZ_SRC_DEFAULT_STREAM) MSMZ_HIP(hipStreamSynchronize(nullptr));
    MSMZ_HIP(hipMemcpy2D(recs->data(), width, dp, stride, width, n, hipMemcpyDefault));
    if (di) {
      flags->resize(n);
      MSMZ_HIP(hipMemcpy(flags->data(), di, n, hipMemcpyDefault));
    }
    return MSMZ_OK;
  }

 private:
  // where the import kernel reads: the caller's device memory, or the packed staging copy of a host source
  struct ImportView {
    const uint8_t* ptr = nullptr;
    uint64_t stride = 0;
    uint32_t width = 0;
    const uint8_t* is_inf = nullptr;
  };

  // May a kernel of this device read [p, p + bytes)?  Yes only if the HIP runtime knows p as memory of this device, or
  // as pinned / registered host memory (then *dev is its device-side address), AND the whole range lies inside the one
  // allocation p belongs to (hipMemGetAddressRange): a range that starts in one allocation and ends in another is
  // refused, whatever lies between.  A pointer the runtime does not know (pageable host memory, a stale or made-up
  // address), managed memory and another device's memory are refused: nothing is launched on them.  Pinned host memory
  // whose allocation the runtime cannot report is accepted only if the first and the last byte are both pinned and
  // their device-side addresses are `bytes - 1` apart.  any_device: the caller only copies (gather_src).
  int vouch(const void* p, uint64_t bytes, bool any_device, const void** dev) const {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    if (bytes == 0 || hipPointerGetAttributes(&a, p) != hipSuccess) {
      (void)hipGetLastError();   // (an unknown pointer is an answer, not a sticky error)
      return MSMZ_ERR_ARG;
    }
    if ((a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeHost) || a.isManaged) return MSMZ_ERR_ARG;
    if (a.type == hipMemoryTypeDevice && !any_device && a.device != device_) return MSMZ_ERR_ARG;
    *dev = a.type == hipMemoryTypeHost ? a.devicePointer : p;
    if (!*dev) return MSMZ_ERR_ARG;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)*dev) == hipSuccess) {
      const uintptr_t lo = (uintptr_t)base, at = (uintptr_t)*dev;
      return at >= lo && bytes <= size && at - lo <= size - bytes ? MSMZ_OK : MSMZ_ERR_ARG;
    }
    (void)hipGetLastError();
    if (a.type != hipMemoryTypeHost) return MSMZ_ERR_ARG;
    hipPointerAttribute_t z;
    memset(&z, 0, sizeof(z));
    if (hipPointerGetAttributes(&z, (const uint8_t*)p + (bytes - 1)) != hipSuccess) {
      (void)hipGetLastError();
      return MSMZ_ERR_ARG;
    }
    if (z.type != hipMemoryTypeHost || z.isManaged || !z.devicePointer) return MSMZ_ERR_ARG;
    return (uintptr_t)z.devicePointer - (uintptr_t)a.devicePointer == bytes - 1 ? MSMZ_OK : MSMZ_ERR_ARG;
  }

  // Checks the source and makes it readable for the import kernel, in stream order.  Device source: the pointers are
  // vouched for and stream_ waits for an event recorded on the producing stream (no host wait).  Host source: `width`
  // bytes per record go to stage_ (a strided source is packed on the host first; `split`: this engine's blocks of a
  // packed source), the flag bytes behind them.
  int import_view(const msmz_src& s, int point_fe_bytes, uint64_t n, const GenMap* split, ImportView* v) {
    if (int st = src_check(&s, point_fe_bytes, &v->width, &v->stride)) return st;
    const uint8_t* p = (const uint8_t*)s.ptr;
    if (s.flags & MSMZ_SRC_DEVICE) {
      if (split) return MSMZ_ERR_ARG;   // (a multi-device context hands its engines host copies)
      const void* dp = nullptr;
      int st;
      if ((st = vouch(p, (n - 1) * v->stride + v->width, false, &dp))) return st;
      v->ptr = (const uint8_t*)dp;
      if (s.is_inf) {
        if ((st = vouch(s.is_inf, n, false, &dp))) return st;
        v->is_inf = (const uint8_t*)dp;
      }
      if (s.stream || (s.flags & MSMZ_SRC_DEFAULT_STREAM)) {
        MSMZ_HIP(hipEventRecord(import_ev_, (hipStream_t)s.stream));
        MSMZ_HIP(hipStreamWaitEvent(stream_, import_ev_, 0));
      }
      return MSMZ_OK;
    }
    const uint32_t w = v->width;
    if (split && v->stride != w) return MSMZ_ERR_ARG;
    int st = stage_.ensure((size_t)n * w + n);
    if (st) return st;
    if (v->stride != w) {
      import_pack_.resize((size_t)n * w);   // (lives until the import's error-word fetch has drained the stream)
      for (uint64_t i = 0; i < n; i++) memcpy(import_pack_.data() + i * w, p + i * v->stride, w);
      p = import_pack_.data();
    }
    // (a failure once a copy may be queued drains the stream: when the call returns the source is no longer read)
    if ((st = copy_h2d(stage_.p, p, w, n, split))) return (void)hipStreamSynchronize(stream_), st;
    if (s.is_inf) {
      uint8_t* d_inf = stage_.as<uint8_t>() + (size_t)n * w;
      if ((st = copy_h2d(d_inf, s.is_inf, 1, n, split))) return (void)hipStreamSynchronize(stream_), st;
      v->is_inf = d_inf;
    }
    v->ptr = stage_.as<const uint8_t>();
    v->stride = w;
    return MSMZ_OK;
  }

  // the conversion kernel over a view, then the error-word fetch: when it returns the source has been read
  int import_scalars_to(uint32_t* dst, const msmz_src& s, const ImportView& v, uint64_t n) {
    MsmMeta* d_meta = meta_.as<MsmMeta>();
    MSMZ_HIP(hipMemsetAsync(&d_meta->error, 0, 4, stream_));
    hipLaunchKernelGGL((k_import_scalars<Fr>), dim3((n + 255) / 256), dim3(256), 0, stream_, dst, v.ptr, v.stride,
                       (int)(v.width / 4), (uint32_t)n, (s.flags & MSMZ_SRC_MONTGOMERY) ? 1 : 0, &d_meta->error);
    uint32_t err = 0;
    if (int st = fetch_error(&err)) return st;
    return err ? MSMZ_ERR_RANGE : MSMZ_OK;   // a scalar (either form) >= group order
  }

 public:
  int random_points(uint64_t n, uint64_t seed, const GenMap& map, uint64_t* h) override {
    if (!h || n == 0 || n >= (1ull << (Cfg::HAS_ENDO ? 29 : 30))) return MSMZ_ERR_ARG;   // record indices (incl. endomorphism images) fit 30 bits
    MSMZ_HIP(hipSetDevice(device_));
    int st = ensure_gen_table();
    if (st) return st;
    const bool endo = Cfg::HAS_ENDO;
    Handle hd{0, n, endo};
    if ((st = alloc_handle(hd, (size_t)n * PW_WORDS * 4 * (endo ? 2 : 1)))) return st;
    if constexpr (TE) {
      hipLaunchKernelGGL((k_te_gen_points<F>), dim3((n + 127) / 128), dim3(128), 0, stream_, hd.mem.as<uint32_t>(),
                         gen_table_.as<uint32_t>(), (uint32_t)n, seed, map);
    } else {
      hipLaunchKernelGGL((k_gen_points<F>), dim3((n + 127) / 128), dim3(128), 0, stream_, hd.mem.as<uint32_t>(),
                         gen_table_.as<uint32_t>(), (uint32_t)n, seed, endo ? 1 : 0, map);
    }
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return add_handle(std::move(hd), h);
  }

  int random_scalars(uint64_t n, uint64_t seed, const GenMap& map, uint64_t* h) override {
    if (!h || n == 0) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd{1, n, false};
    if (int st = alloc_handle(hd, n * 32)) return st;
    hipLaunchKernelGGL((k_gen_scalars<Fr>), dim3((n + 255) / 256), dim3(256), 0, stream_, hd.mem.as<uint32_t>(),
                       (uint32_t)n, seed, map);
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return add_handle(std::move(hd), h);
  }

  int download_points(uint64_t hd, uint64_t first, uint64_t count, uint8_t* xy, uint8_t* inf) override {
    auto it = handles_.find(hd);
    if (it == handles_.end() || it->second.kind != 0 || !xy) return MSMZ_ERR_ARG;
    {
      // the endomorphism images stay readable; a precomputed set: all its copies
      const uint64_t have = it->second.factor ? it->second.copy_stride * it->second.factor
                                              : it->second.n * (it->second.has_endo ? 2 : 1);
      if (first > have || count > have - first) return MSMZ_ERR_ARG;        // (no first + count: it can wrap)
    }
    if (count == 0) return MSMZ_OK;
    MSMZ_HIP(hipSetDevice(device_));
    int st = stage_.ensure(count * RW * 4);
    if (st) return st;
    if constexpr (TE) {
      hipLaunchKernelGGL((k_te_points_from_niels<F>), dim3((count + 255) / 256), dim3(256), 0, stream_,
                         stage_.as<uint32_t>(), it->second.mem.template as<const uint32_t>() + first * PW_WORDS, (uint32_t)count);
    } else {
      hipLaunchKernelGGL((k_points_from_mont<F>), dim3((count + 255) / 256), dim3(256), 0, stream_,
                         stage_.as<uint32_t>(), it->second.mem.template as<const uint32_t>() + first * PW_WORDS, (uint32_t)count);
    }
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipMemcpyAsync(xy, stage_.p, count * RW * 4, hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    if (inf) {
      for (uint64_t i = 0; i < count; i++) {
        bool z = !TE;   // twisted Edwards has no point at infinity: the identity is the affine point (0, 1)
        for (int j = 0; j < RW * 4; j++) z = z && xy[i * RW * 4 + j] == 0;
        inf[i] = z ? 1 : 0;
      }
    }
    return MSMZ_OK;
  }

  int download_scalars(uint64_t hd, uint64_t first, uint64_t count, uint8_t* s) override {
    auto it = handles_.find(hd);
    if (it == handles_.end() || it->second.kind != 1 || !s) return MSMZ_ERR_ARG;
    if (first > it->second.n || count > it->second.n - first) return MSMZ_ERR_ARG;
    if (count == 0) return MSMZ_OK;
    MSMZ_HIP(hipSetDevice(device_));
    MSMZ_HIP(hipMemcpy(s, it->second.mem.template as<const uint8_t>() + first * 32, count * 32, hipMemcpyDeviceToHost));
    return MSMZ_OK;
  }

  int free_handle(uint64_t hd) override {
    auto it = handles_.find(hd);
    if (it == handles_.end()) return MSMZ_ERR_ARG;
    (void)hipSetDevice(device_);
    handles_.erase(it);
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ validation
  // msmz_check_points: the curve equation, then (if asked, and unless the curve has cofactor 1) [q]P = O, over base
  // points [first, first + count) of a plain point handle.  A query: bad points are reported, not refused.  Two launches,
  // then the result record and the verdict bytes come back behind ONE host wait, like the error word of an upload.
  int check_points(uint64_t hd, uint64_t first, uint64_t count, uint32_t what, msmz_check_result* out,
                   uint8_t* verdicts) override {
    if (!out || count == 0 || what == 0 || (what & ~(uint32_t)(MSMZ_CHECK_CURVE | MSMZ_CHECK_SUBGROUP))) return MSMZ_ERR_ARG;
    auto it = handles_.find(hd);
    if (it == handles_.end() || it->second.kind != 0) return MSMZ_ERR_ARG;
    if (it->second.factor) return MSMZ_ERR_UNSUPPORTED;   // derived data: the source set is what a caller checks
    if (first > it->second.n || count > it->second.n - first) return MSMZ_ERR_ARG;   // (base points only; no first + count: it can wrap)
    MSMZ_HIP(hipSetDevice(device_));
    if (int st = ensure_host_check(verdicts ? count : 0)) return st;
    if (int st = check_.ensure(sizeof(CheckResult) + count)) return st;
    CheckResult* d_res = check_.as<CheckResult>();
    uint8_t* d_verdicts = check_.as<uint8_t>() + sizeof(CheckResult);
    const uint32_t* recs = it->second.mem.template as<const uint32_t>() + first * PW_WORDS;
    const dim3 grid((uint32_t)((count + 255) / 256)), block(256);
    MSMZ_HIP(hipMemsetAsync(d_res, 0, 8, stream_));
    MSMZ_HIP(hipMemsetAsync(&d_res->first_bad, 0xff, 4, stream_));
    const bool chain = (what & MSMZ_CHECK_SUBGROUP) && !Fr::PRIME_ORDER;   // cofactor 1: the curve is the subgroup
    if constexpr (TE) {
      hipLaunchKernelGGL((k_te_check_curve<F>), grid, block, 0, stream_, d_verdicts, d_res, recs, (uint32_t)count, (uint32_t)first);
      if (chain)
        hipLaunchKernelGGL((k_te_check_subgroup<F, Fr>), grid, block, 0, stream_, d_verdicts, d_res, recs, (uint32_t)count, (uint32_t)first);
    } else {
      hipLaunchKernelGGL((k_check_curve<F>), grid, block, 0, stream_, d_verdicts, d_res, recs, (uint32_t)count, (uint32_t)first);
      if (chain)
        hipLaunchKernelGGL((k_check_subgroup<F, Fr>), grid, block, 0, stream_, d_verdicts, d_res, recs, (uint32_t)count, (uint32_t)first);
    }
    MSMZ_HIP(hipGetLastError());
    // both land in pinned memory (a copy into the caller's pageable buffer would block the host a second time)
    MSMZ_HIP(hipMemcpyAsync(h_check_, d_res, sizeof(CheckResult) + (verdicts ? count : 0), hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    if (verdicts) memcpy(verdicts, reinterpret_cast<const uint8_t*>(h_check_) + sizeof(CheckResult), count);
    out->off_curve = h_check_->off_curve;
    out->off_subgroup = h_check_->off_subgroup;
    out->first_bad = h_check_->first_bad == 0xffffffffu ? UINT64_MAX : h_check_->first_bad;
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ per-point multiplication
  // msmz_points_mul: a new plain point handle, record i = [s_i] P_i (+ Q_i).  One launch; the error word (a resident
  // scalar >= q) comes back behind the ONE host wait, like that of an upload.
  int points_mul(const msmz_mul& m, uint64_t n, uint64_t* h) override {
    if (!h || n == 0 || n >= (1ull << (Cfg::HAS_ENDO ? 29 : 30))) return MSMZ_ERR_ARG;   // as random_points
    auto pit = handles_.find(m.points_handle);
    if (pit == handles_.end() || pit->second.kind != 0) return MSMZ_ERR_ARG;
    auto qit = handles_.end(), sit = handles_.end();
    if (m.addend_handle) {
      qit = handles_.find(m.addend_handle);
      if (qit == handles_.end() || qit->second.kind != 0) return MSMZ_ERR_ARG;
    }
    if (m.scalars_handle) {
      sit = handles_.find(m.scalars_handle);
      if (sit == handles_.end() || sit->second.kind != 1) return MSMZ_ERR_ARG;
    } else if (!m.scalar) {
      return MSMZ_ERR_ARG;
    }
    if (pit->second.factor || (m.addend_handle && qit->second.factor)) return MSMZ_ERR_UNSUPPORTED;   // derived data
    auto beyond = [n](const Handle& s, uint64_t first) { return first > s.n || n > s.n - first; };   // (no first + n: it can wrap)
    if (beyond(pit->second, m.first_p) || (m.addend_handle && beyond(qit->second, m.first_q)) ||
        (m.scalars_handle && beyond(sit->second, m.first_s)))
      return MSMZ_ERR_ARG;
    MulScalar bc{};
    if (!m.scalars_handle) {
      memcpy(bc.w, m.scalar, 32);
      if (words_geq<8>(bc.w, Fr::Q)) return MSMZ_ERR_RANGE;
    }
    MSMZ_HIP(hipSetDevice(device_));
    const bool endo = Cfg::HAS_ENDO;
    Handle hd{0, n, endo};
    if (int st = alloc_handle(hd, (size_t)n * PW_WORDS * 4 * (endo ? 2 : 1))) return st;
    MsmMeta* d_meta = meta_.as<MsmMeta>();
    MSMZ_HIP(hipMemsetAsync(&d_meta->error, 0, 4, stream_));
    const uint32_t* P = pit->second.mem.template as<const uint32_t>() + m.first_p * PW_WORDS;
    const uint32_t* Q = m.addend_handle ? qit->second.mem.template as<const uint32_t>() + m.first_q * PW_WORDS : nullptr;
    const uint32_t* S = m.scalars_handle ? sit->second.mem.template as<const uint32_t>() + m.first_s * 8 : nullptr;
    const dim3 grid((uint32_t)((n + 255) / 256)), block(256);   // whole blocks: every wave reaches the inversion entire
    if constexpr (TE) {
      hipLaunchKernelGGL((k_te_points_mul<F, Fr>), grid, block, 0, stream_, hd.mem.as<uint32_t>(), P, S, bc, Q, (uint32_t)n,
                         &d_meta->error);
    } else {
      hipLaunchKernelGGL((k_points_mul<F, Fr>), grid, block, 0, stream_, hd.mem.as<uint32_t>(), P, S, bc, Q, (uint32_t)n,
                         endo ? 1 : 0, &d_meta->error);
    }
    uint32_t err = 0;
    if (int st = fetch_error(&err)) return st;
    if (err) return MSMZ_ERR_RANGE;   // a resident scalar >= group order
    return add_handle(std::move(hd), h);
  }

  // ------------------------------------------------------------------------------------------ scalar-set arithmetic
  // msmz_scalars_combine: out_i = x.c_i x.v_i (+ y.c_i y.v_i) into a new scalar handle or over a range of an existing
  // one.  One launch; the error word (a resident record >= q) comes back behind the ONE host wait.
  int scalars_combine(const msmz_scalar_term& x, const msmz_scalar_term* y, uint64_t n, uint64_t first_out,
                      uint64_t* out_handle) override {
    if (!out_handle || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    const bool fresh = *out_handle == 0;
    if (fresh && first_out != 0) return MSMZ_ERR_ARG;
    auto beyond = [n](const Handle& s, uint64_t first) { return first > s.n || n > s.n - first; };   // (no first + n: it can wrap)
    // a range of a scalar set -> its first record; a partial overlap with the destination is refused
    auto range = [&](uint64_t h, uint64_t first, const uint32_t** p) {
      auto it = handles_.find(h);
      if (it == handles_.end() || it->second.kind != 1 || beyond(it->second, first)) return false;
      if (!fresh && h == *out_handle && first != first_out && (first > first_out ? first - first_out : first_out - first) < n)
        return false;
      *p = it->second.mem.template as<const uint32_t>() + first * 8;
      return true;
    };
    ScalarTerm t[2] = {};
    const msmz_scalar_term* in[2] = {&x, y};
    for (int k = 0; k < 2; k++) {
      if (!in[k]) continue;
      if (!range(in[k]->handle, in[k]->first, &t[k].v)) return MSMZ_ERR_ARG;
      if (in[k]->coeff_handle && !range(in[k]->coeff_handle, in[k]->coeff_first, &t[k].c)) return MSMZ_ERR_ARG;
    }
    uint32_t* out = nullptr;
    if (!fresh) {
      auto it = handles_.find(*out_handle);
      if (it == handles_.end() || it->second.kind != 1 || beyond(it->second, first_out)) return MSMZ_ERR_ARG;
      out = it->second.mem.template as<uint32_t>() + first_out * 8;
    }
    for (int k = 0; k < 2; k++) {
      if (!in[k] || in[k]->coeff_handle) continue;
      if (!in[k]->coeff) {
        t[k].unit = 1;
        continue;
      }
      uint32_t c[8];
      memcpy(c, in[k]->coeff, 32);
      if (words_geq<8>(c, Fr::Q)) return MSMZ_ERR_RANGE;
      fr_to_mont<Fr>(t[k].k.w, c);
    }
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd{1, n, false};
    if (fresh) {
      if (int st = alloc_handle(hd, n * 32)) return st;
      out = hd.mem.as<uint32_t>();
    }
    MsmMeta* d_meta = meta_.as<MsmMeta>();
    MSMZ_HIP(hipMemsetAsync(&d_meta->error, 0, 4, stream_));
    hipLaunchKernelGGL((k_scalars_combine<Fr>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream_, out, t[0], t[1],
                       (uint32_t)n, &d_meta->error);
    uint32_t err = 0;
    if (int st = fetch_error(&err)) return st;
    if (err) return MSMZ_ERR_RANGE;   // a resident record >= group order
    return fresh ? add_handle(std::move(hd), out_handle) : (int)MSMZ_OK;
  }

  // msmz_scalars_dot: one partial sum per tile, one workgroup folds them; the result and the error word share a
  // 64-byte record in front of the partial sums and come back in ONE copy behind ONE host wait.
  int scalars_dot(uint64_t xh, uint64_t first_x, uint64_t yh, uint64_t first_y, uint64_t n, uint8_t* out) override {
    if (!out || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    auto xit = handles_.find(xh);
    if (xit == handles_.end() || xit->second.kind != 1) return MSMZ_ERR_ARG;
    auto yit = handles_.end();
    if (yh) {
      yit = handles_.find(yh);
      if (yit == handles_.end() || yit->second.kind != 1) return MSMZ_ERR_ARG;
    } else if (first_y) {
      return MSMZ_ERR_ARG;
    }
    auto beyond = [n](const Handle& s, uint64_t first) { return first > s.n || n > s.n - first; };
    if (beyond(xit->second, first_x) || (yh && beyond(yit->second, first_y))) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    const uint32_t tiles = (uint32_t)((n + SDOT_TILE - 1) / SDOT_TILE);
    if (int st = sdot_.ensure(64 + (size_t)tiles * 32)) return st;
    uint32_t* d_res = sdot_.as<uint32_t>();   // words 0..7: the result, word 8: the error word, from word 16: the partial sums
    MSMZ_HIP(hipMemsetAsync(d_res, 0, 64, stream_));
    const uint32_t* X = xit->second.mem.template as<const uint32_t>() + first_x * 8;
    const uint32_t* Y = yh ? yit->second.mem.template as<const uint32_t>() + first_y * 8 : nullptr;
    hipLaunchKernelGGL((k_scalars_dot<Fr>), dim3(tiles), dim3(SDOT_THREADS), 0, stream_, d_res + 16, X, Y, (uint32_t)n, d_res + 8);
    hipLaunchKernelGGL((k_scalars_dot_fold<Fr>), dim3(1), dim3(SDOT_THREADS), 0, stream_, d_res, d_res + 16, tiles, Y ? 1 : 0);
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipMemcpyAsync(h_res_, d_res, 64, hipMemcpyDeviceToHost, stream_));   // (pinned: init sized it for far more)
    MSMZ_HIP(hipStreamSynchronize(stream_));
    if (h_res_[8]) return MSMZ_ERR_RANGE;   // a resident record >= group order
    memcpy(out, h_res_, 32);
    return MSMZ_OK;
  }

  // msmz_scalars_powers: a new scalar handle, local entry i = base ratio^(set index of i).  The host builds the table of
  // ratio^(2^k) with fr.h; it travels as a kernel argument.
  int scalars_powers(const uint8_t* base, const uint8_t* ratio, uint64_t n, const GenMap& map, uint64_t* h) override {
    if (!h || !ratio || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    FrConst b{};
    uint32_t r[8];
    b.w[0] = 1;
    if (base) memcpy(b.w, base, 32);
    memcpy(r, ratio, 32);
    if (words_geq<8>(b.w, Fr::Q) || words_geq<8>(r, Fr::Q)) return MSMZ_ERR_RANGE;
    FrPowTable table;
    fr_pow_table<Fr>(table, r);
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd{1, n, false};
    if (int st = alloc_handle(hd, n * 32)) return st;
    const uint64_t threads = (n + SPOW_RUN - 1) / SPOW_RUN;
    hipLaunchKernelGGL((k_scalars_powers<Fr>), dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream_,
                       hd.mem.as<uint32_t>(), b, table, (uint32_t)n, map);
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return add_handle(std::move(hd), h);
  }

  // A range of n entries of a scalar set for msmz_scalars_recurrence / _inverse -> its first record; false: not a scalar
  // set, beyond it, or overlapping the destination [first_out, +n) of *out_handle in part (fresh: no destination yet).
  bool scan_range(uint64_t h, uint64_t first, uint64_t n, bool fresh, uint64_t out_handle, uint64_t first_out,
                  const uint32_t** p) {
    auto it = handles_.find(h);
    if (it == handles_.end() || it->second.kind != 1 || first > it->second.n || n > it->second.n - first) return false;
    if (!fresh && h == out_handle && first != first_out && (first > first_out ? first - first_out : first_out - first) < n)
      return false;
    *p = it->second.mem.template as<const uint32_t>() + first * 8;
    return true;
  }

  // msmz_scalars_recurrence: three launches (tile aggregates, ONE workgroup of carries, apply); the final value and the
  // error word share a 64-byte record in front of the scratch and come back in ONE copy behind ONE host wait.
  int scalars_recurrence(const msmz_scalar_rec& r, uint64_t n, uint64_t first_out, uint64_t* out_handle,
                         uint8_t* last) override {
    if (!out_handle || n == 0 || n >> 32 || (r.flags & ~(uint32_t)(MSMZ_REC_REVERSE | MSMZ_REC_EXCLUSIVE)))
      return MSMZ_ERR_ARG;
    if (!r.a_handle && !r.a && !r.b_handle) return MSMZ_ERR_ARG;   // y_i = y_(i-1): nothing to do
    const bool fresh = *out_handle == 0;
    if (fresh && first_out != 0) return MSMZ_ERR_ARG;
    const uint32_t *A = nullptr, *B = nullptr;
    if (r.a_handle && !scan_range(r.a_handle, r.a_first, n, fresh, *out_handle, first_out, &A)) return MSMZ_ERR_ARG;
    if (r.b_handle && !scan_range(r.b_handle, r.b_first, n, fresh, *out_handle, first_out, &B)) return MSMZ_ERR_ARG;
    uint32_t* out = nullptr;
    if (!fresh) {
      auto it = handles_.find(*out_handle);
      if (it == handles_.end() || it->second.kind != 1 || first_out > it->second.n || n > it->second.n - first_out)
        return MSMZ_ERR_ARG;
      out = it->second.mem.template as<uint32_t>() + first_out * 8;
    }
    FrConst k{}, init{};
    if (!r.a_handle && r.a) {
      uint32_t c[8];
      memcpy(c, r.a, 32);
      if (words_geq<8>(c, Fr::Q)) return MSMZ_ERR_RANGE;
      fr_to_mont<Fr>(k.w, c);
    }
    if (r.init) {
      memcpy(init.w, r.init, 32);
      if (words_geq<8>(init.w, Fr::Q)) return MSMZ_ERR_RANGE;
    } else if (!B) {
      init.w[0] = 1;
    }
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd{1, n, false};
    if (fresh) {
      if (int st = alloc_handle(hd, n * 32)) return st;
      out = hd.mem.as<uint32_t>();
    }
    const uint32_t tiles = (uint32_t)((n + SREC_TILE - 1) / SREC_TILE);
    // words 0..7: the final value, word 8: the error word; then the aggregates' A, their B, and tiles + 1 incoming values
    if (int st = sscan_.ensure(64 + ((size_t)tiles * 3 + 1) * 32)) return st;
    uint32_t* d_res = sscan_.as<uint32_t>();
    uint32_t* aggA = d_res + 16;
    uint32_t* aggB = aggA + (size_t)tiles * 8;
    uint32_t* incoming = aggB + (size_t)tiles * 8;
    MSMZ_HIP(hipMemsetAsync(d_res, 0, 64, stream_));
    const uint32_t nn = (uint32_t)n, flags = r.flags;
    const dim3 grid(tiles), block(SREC_THREADS);
#define MSMZ_REC_LAUNCH(AM, HB)                                                                                          \
  do {                                                                                                                   \
    hipLaunchKernelGGL((k_scalars_rec_tile<Fr, AM, HB>), grid, block, 0, stream_, aggA, aggB, A, B, k, nn, flags, d_res + 8); \
    hipLaunchKernelGGL((k_scalars_rec_carry<Fr, AM != SREC_A_NONE, HB>), dim3(1), block, 0, stream_, incoming, d_res,    \
                       (const uint32_t*)aggA, (const uint32_t*)aggB, init, tiles);                                       \
    hipLaunchKernelGGL((k_scalars_rec_apply<Fr, AM, HB>), grid, block, 0, stream_, out, A, B, k, (const uint32_t*)incoming, \
                       nn, flags);                                                                                       \
  } while (0)
    if (A && B) MSMZ_REC_LAUNCH(SREC_A_RESIDENT, true);
    else if (A) MSMZ_REC_LAUNCH(SREC_A_RESIDENT, false);
    else if (r.a && B) MSMZ_REC_LAUNCH(SREC_A_BROADCAST, true);
    else if (r.a) MSMZ_REC_LAUNCH(SREC_A_BROADCAST, false);
    else MSMZ_REC_LAUNCH(SREC_A_NONE, true);
#undef MSMZ_REC_LAUNCH
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipMemcpyAsync(h_res_, d_res, 64, hipMemcpyDeviceToHost, stream_));   // (pinned: init sized it for far more)
    MSMZ_HIP(hipStreamSynchronize(stream_));
    if (h_res_[8]) return MSMZ_ERR_RANGE;   // a resident record >= group order
    if (last) memcpy(last, h_res_, 32);
    return fresh ? add_handle(std::move(hd), out_handle) : (int)MSMZ_OK;
  }

  // msmz_scalars_inverse: one launch; the error word and the zero count share the record
  int scalars_inverse(uint64_t h, uint64_t first, uint64_t n, uint64_t first_out, uint64_t* out_handle,
                      uint64_t* n_zero) override {
    if (!out_handle || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    const bool fresh = *out_handle == 0;
    if (fresh && first_out != 0) return MSMZ_ERR_ARG;
    const uint32_t* X = nullptr;
    if (!scan_range(h, first, n, fresh, *out_handle, first_out, &X)) return MSMZ_ERR_ARG;
    uint32_t* out = nullptr;
    if (!fresh) {
      auto it = handles_.find(*out_handle);
      if (it == handles_.end() || it->second.kind != 1 || first_out > it->second.n || n > it->second.n - first_out)
        return MSMZ_ERR_ARG;
      out = it->second.mem.template as<uint32_t>() + first_out * 8;
    }
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd{1, n, false};
    if (fresh) {
      if (int st = alloc_handle(hd, n * 32)) return st;
      out = hd.mem.as<uint32_t>();
    }
    if (int st = sscan_.ensure(64)) return st;
    uint32_t* d_res = sscan_.as<uint32_t>();   // word 8: the error word, word 9: the zeros
    MSMZ_HIP(hipMemsetAsync(d_res, 0, 64, stream_));
    const uint64_t per_block = (uint64_t)SINV_THREADS * SINV_E;
    hipLaunchKernelGGL((k_scalars_inverse<Fr>), dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(SINV_THREADS), 0,
                       stream_, out, X, (uint32_t)n, d_res);
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipMemcpyAsync(h_res_, d_res, 64, hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    if (h_res_[8]) return MSMZ_ERR_RANGE;   // a resident record >= group order
    if (n_zero) *n_zero = h_res_[9];
    return fresh ? add_handle(std::move(hd), out_handle) : (int)MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ precomputed point sets
  int precompute_params(uint64_t n, const msmz_opts* o, uint32_t factor, int* c_out, int* glv_out,
                        uint32_t* f_out, int* k_out, int* sbits_out) const override {
    if (TE) return MSMZ_ERR_UNSUPPORTED;   // twisted Edwards runs msmBasic: no batched-affine buckets to share
    return planner_.precompute_params(n, o, factor, c_out, glv_out, f_out, k_out, sbits_out);
  }

  // new handle: `F` copies of the first n points of `ph`, copy j = 2^(c j) P_i (+ the endomorphism images with glv)
  int precompute_points(uint64_t ph, uint64_t n, int c, int glv, uint32_t copies, int sbits, uint64_t* h) override {
    if (TE) return MSMZ_ERR_UNSUPPORTED;
    auto pit = handles_.find(ph);
    if (!h || pit == handles_.end() || pit->second.kind != 0 || pit->second.factor != 0 || n == 0 || pit->second.n < n ||
        copies < 2 || c < 2 || c > 24)
      return MSMZ_ERR_ARG;
    const Handle& src = pit->second;
    if (glv && !src.has_endo) return MSMZ_ERR_UNSUPPORTED;
    MSMZ_HIP(hipSetDevice(device_));
    const uint64_t R = n * (glv ? 2 : 1);
    const size_t rec = (size_t)PW_WORDS * 4;
    Handle hd{0, n, glv != 0};
    if (int st = alloc_handle(hd, (size_t)copies * R * rec)) return st;
    uint8_t* dev = hd.mem.as<uint8_t>();
    // copy 0: the source's first n points (and their images, which follow the source's whole set)
    MSMZ_HIP(hipMemcpyAsync(dev, src.mem.p, n * rec, hipMemcpyDeviceToDevice, stream_));
    if (glv)
      MSMZ_HIP(hipMemcpyAsync(dev + n * rec, src.mem.template as<const uint8_t>() + src.n * rec, n * rec,
                              hipMemcpyDeviceToDevice, stream_));
    for (uint32_t j = 1; j < copies; j++) {
      if constexpr (!TE)
        hipLaunchKernelGGL((k_precompute_copy<F>), dim3((n + 255) / 256), dim3(256), 0, stream_,
                           (uint32_t*)(dev + j * R * rec), (const uint32_t*)(dev + (j - 1) * R * rec), (uint32_t)n, c, glv);
      MSMZ_HIP(hipGetLastError());
    }
    MSMZ_HIP(hipStreamSynchronize(stream_));
    hd.factor = copies;
    hd.c = c;
    hd.glv = glv;
    hd.copy_stride = R;
    hd.sbits = planner_.bound(sbits);
    return add_handle(std::move(hd), h);
  }

  int precomputed_info(uint64_t hd, int32_t* c, int32_t* glv, uint32_t* factor, uint32_t* K, uint64_t* records,
                       int32_t* sbits) override {
    auto it = handles_.find(hd);
    if (it == handles_.end() || it->second.factor == 0) return MSMZ_ERR_ARG;
    const Handle& h = it->second;
    const int b = planner_.scalar_bits(h.glv != 0, 0, h.sbits);
    if (sbits) *sbits = h.sbits;
    if (c) *c = h.c;
    if (glv) *glv = h.glv;
    if (factor) *factor = h.factor;
    if (K) *K = (uint32_t)((b + 1 + h.c - 1) / h.c);
    if (records) *records = h.copy_stride * h.factor;
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ msm
  // `batch` MSMs over the first n points: problem k's scalars are entries [k n, (k + 1) n) of the resident set `sh`, or
  // vector k of the host buffer (at host_scalars + k host_stride 32; host_stride = n unless a multi-device context hands
  // this engine its share `split` of longer vectors).  batch = 1 is msmz_msm.  Sub-batches run one after another
  // (run_problems decides how each runs), their logs summed.
  int msm_batch(uint64_t ph, const uint8_t* host_scalars, uint64_t sh, uint64_t n, uint32_t batch, const msmz_opts* o,
                uint8_t* out, int* out_inf, msmz_log* log, const GenMap* split = nullptr,
                uint64_t host_stride = 0) override {
    auto t_begin = std::chrono::steady_clock::now();
    if (!out || !out_inf || n == 0 || batch == 0) return MSMZ_ERR_ARG;
    auto pit = handles_.find(ph);
    if (pit == handles_.end() || pit->second.kind != 0 || pit->second.n < n) return MSMZ_ERR_ARG;
    msmz_opts opt;
    int st0 = resolve_opts(pit->second, o, &opt);
    if (st0) return st0;
    if (opt.glv < 0) opt.glv = pit->second.has_endo && planner_.default_glv(n, opt.reserved[1]) ? 1 : 0;   // (per problem: batch = 1 is msm())
    if (host_stride == 0) host_stride = n;
    if (host_scalars && host_stride < n) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    const uint64_t total = (uint64_t)batch * n;
    const uint32_t* d_scalars = nullptr;
    if (host_scalars) {
      // range (< group order) is checked on the device while the scalars are sliced
      int st = stage_.ensure(total * 32);
      if (st) return st;
      if (!split && host_stride == n) {
        if ((st = copy_h2d(stage_.p, host_scalars, 32, total, nullptr))) return st;
      } else {
        for (uint32_t k = 0; k < batch; k++)
          if ((st = copy_h2d(stage_.as<uint8_t>() + (size_t)k * n * 32, host_scalars + (size_t)k * host_stride * 32, 32, n,
                             split)))
            return st;
      }
      d_scalars = stage_.as<uint32_t>();
    } else {
      auto sit = handles_.find(sh);
      if (sit == handles_.end() || sit->second.kind != 1 || sit->second.n < total) return MSMZ_ERR_ARG;
      d_scalars = sit->second.mem.template as<const uint32_t>();
    }
    if (log) memset(log, 0, sizeof(*log));
    const Handle& pts = pit->second;
    int st = MSMZ_OK;
    for (uint32_t done = 0; done < batch && st == MSMZ_OK;) {
      msmz_log plog;
      memset(&plog, 0, sizeof(plog));
      uint32_t ran = 0;
      st = run_problems(pts, d_scalars + (size_t)done * n * 8, n, batch - done, opt, out + (size_t)done * RW * 4,
                        out_inf + done, log ? &plog : nullptr, &ran);
      if (st) break;
      if (log) merge_log(log, plog, done == 0, LogMerge::SEQUENTIAL);
      done += ran;
    }
    if (log) {
      log->stage_ms[MSMZ_ST_TOTAL] =
          std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    }
    return st;
  }

  // msmz_msm_segments: problem k = scalars [first_s, first_s + n) of `sh` times base points [first_p, first_p + n) of `ph`.
  // The segments are dealt into length classes (segment_classes, multi.h); run_segments decides how each class runs, for
  // its longest segment; results go back through the permutation, logs are summed as msm_batch sums them.
  int msm_segments(uint64_t ph, uint64_t sh, const msmz_segment* segs, uint32_t n_segs, const msmz_opts* o, uint8_t* out,
                   int* out_inf, msmz_log* log) override {
    auto t_begin = std::chrono::steady_clock::now();
    if (!segs || !out || !out_inf || n_segs == 0) return MSMZ_ERR_ARG;
    auto pit = handles_.find(ph), sit = handles_.find(sh);
    if (pit == handles_.end() || pit->second.kind != 0 || sit == handles_.end() || sit->second.kind != 1) return MSMZ_ERR_ARG;
    const Handle& pts = pit->second;
    const Handle& sc = sit->second;
    std::vector<uint64_t> lens(n_segs);
    for (uint32_t k = 0; k < n_segs; k++) {
      const msmz_segment& s = segs[k];   // (no first + n: it can wrap)
      if (s.n == 0 || s.first_p > pts.n || s.n > pts.n - s.first_p || s.first_s > sc.n || s.n > sc.n - s.first_s)
        return MSMZ_ERR_ARG;
      lens[k] = s.n;
    }
    msmz_opts opt;
    if (int st = resolve_opts(pts, o, &opt)) return st;
    MSMZ_HIP(hipSetDevice(device_));
    if (log) memset(log, 0, sizeof(*log));
    std::vector<uint32_t> order, starts;
    segment_classes(lens.data(), n_segs, &order, &starts);
    const bool fits32 = !(sc.n >> 32);   // the descriptors of the batched pipeline hold 32-bit offsets
    int st = MSMZ_OK;
    bool first = true;
    for (size_t ci = 0; ci + 1 < starts.size() && st == MSMZ_OK; ci++) {
      const uint32_t lo = starts[ci], hi = starts[ci + 1];
      uint64_t n_max = 0;
      for (uint32_t j = lo; j < hi; j++) n_max = lens[order[j]] > n_max ? lens[order[j]] : n_max;
      msmz_opts copt = opt;
      if (copt.glv < 0) copt.glv = pts.has_endo && planner_.default_glv(n_max, copt.reserved[1]) ? 1 : 0;   // (as msm_batch, per class)
      for (uint32_t done = lo; done < hi && st == MSMZ_OK;) {
        msmz_log plog;
        memset(&plog, 0, sizeof(plog));
        uint32_t ran = 0;
        st = run_segments(pts, sc.mem.template as<const uint32_t>(), segs, order.data() + done, hi - done, n_max, fits32, copt,
                          out, out_inf, log ? &plog : nullptr, &ran);
        if (st) break;
        if (log) merge_log(log, plog, first, LogMerge::SEQUENTIAL);
        first = false;
        done += ran;
      }
    }
    if (log) {
      log->stage_ms[MSMZ_ST_TOTAL] =
          std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    }
    return st;
  }

  // ------------------------------------------------------------------ tests (msmz_test.h; the stage hooks: test_hooks.h)
  int test_set_glv_bits(int bits) override {
    if (!Fr::HAS_GLV) return MSMZ_ERR_UNSUPPORTED;
    if (bits != 0 && (bits < 8 || bits > Fr::GLV_BITS - 1)) return MSMZ_ERR_ARG;
    planner_.k.glv_bits_assumed = bits;
    return MSMZ_OK;
  }
  int test_retries() override { return retries_; }
  int test_set_limits(uint64_t pass_entries, uint64_t batch_entries) override {
    if (pass_entries != 0 && (pass_entries < 2 || pass_entries > kMaxEntriesPerPass)) return MSMZ_ERR_ARG;
    if (batch_entries > kMaxBatchEntries) return MSMZ_ERR_ARG;
    pass_entries_ = pass_entries ? pass_entries : kMaxEntriesPerPass;
    planner_.k.batch_entries = batch_entries;
    return MSMZ_OK;
  }
  void test_passes(uint64_t* range_passes, uint64_t* sub_batches) override {
    if (range_passes) *range_passes = range_passes_;
    if (sub_batches) *sub_batches = sub_batches_;
  }
  ITestHooks* test_hooks() override { return &hooks_; }

  // ------------------------------------------------------------------------------------------ what only the engine calls
 private:
  // Host -> device copy of this engine's `n` local records of `rec` bytes.  split == nullptr: one contiguous copy.
  // Otherwise the engine is shard `split->shard` of `split->nshards` inside a multi-device context (multi.h): its local
  // block b is global block b * nshards + shard of the caller's buffer, so every block is copied straight from where
  // the caller has it -- no gathered host copy in between.
  int copy_h2d(void* dst, const uint8_t* src, size_t rec, uint64_t n, const GenMap* split) {
    if (!split || split->nshards <= 1) {
      MSMZ_HIP(hipMemcpyAsync(dst, src, n * rec, hipMemcpyHostToDevice, stream_));
      return MSMZ_OK;
    }
    const uint64_t blk = 1ull << split->blk_shift;
    for (uint64_t li = 0; li < n; li += blk) {
      const uint64_t len = n - li < blk ? n - li : blk;
      const uint64_t gi = ((li >> split->blk_shift) * split->nshards + split->shard) << split->blk_shift;
      MSMZ_HIP(hipMemcpyAsync((uint8_t*)dst + li * rec, src + gi * rec, len * rec, hipMemcpyHostToDevice, stream_));
    }
    return MSMZ_OK;
  }

  // *word = the meta error word as the launches queued so far leave it (one host round trip).  What a bit means is the
  // caller's to say: it differs between the kernels that raise them.
  int fetch_error(uint32_t* word) {
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipMemcpyAsync(&h_meta_->error, &meta_.as<MsmMeta>()->error, 4, hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    *word = h_meta_->error;
    return MSMZ_OK;
  }

  // the device memory of a new handle (owned by it: an error before add_handle frees it)
  int alloc_handle(Handle& hd, size_t bytes) {
    MSMZ_HIP(hipMalloc(&hd.mem.p, bytes));
    hd.mem.bytes = bytes;
    return MSMZ_OK;
  }
  int add_handle(Handle&& hd, uint64_t* h) {
    *h = next_handle_++;
    handles_.emplace(*h, std::move(hd));
    return MSMZ_OK;
  }

  // The options of an MSM over handle `h`: a precomputed set fixes c and the GLV choice (opts->c must be 0 or its c,
  // opts->glv -1 or its choice; a null opts means both defaults) and takes batched-affine buckets with the 2-D reduction.
  // reserved[1], the scalar bit bound, leaves here as the planner's (Planner::bound); a precomputed set fixes it too.
  int resolve_opts(const Handle& h, const msmz_opts* o, msmz_opts* opt) const {
    memset(opt, 0, sizeof(*opt));
    if (o) *opt = *o;
    if (opt->reserved[1] < 0 || opt->reserved[1] > 256) return MSMZ_ERR_ARG;
    opt->reserved[1] = planner_.bound(opt->reserved[1]);
    if (!h.factor) return MSMZ_OK;
    if (!o) opt->glv = -1;
    if (opt->buckets == MSMZ_BUCKETS_PROJECTIVE || opt->reserved[0] == 1) return MSMZ_ERR_UNSUPPORTED;
    if ((opt->c != 0 && opt->c != h.c) || (opt->glv >= 0 && (opt->glv != 0) != (h.glv != 0))) return MSMZ_ERR_ARG;
    if (opt->reserved[1] != 0 && opt->reserved[1] != h.sbits) return MSMZ_ERR_ARG;
    opt->c = h.c;
    opt->glv = h.glv;
    opt->reserved[1] = h.sbits;
    return MSMZ_OK;
  }

  // How a shape runs is decided here.  Up to `remaining` problems over device scalars; *ran = how many it ran.
  //  - one batched pipeline over a sub-batch of them (planner_.batch_size): Weierstrass batched-affine buckets with the
  //    2-D reduction, n within one sort pass, and a sub-batch plan the two-level sort takes -- a plan that falls off it
  //    (also only after the GLV retry) runs the first problem alone and the rest is decided again;
  //  - else the first problem alone over consecutive index ranges of at most one sort pass (2^24 entries; 2^23 points
  //    with GLV) whose partial sums are folded on the host -- the same additivity the multi-GPU split uses -- each range
  //    with batched-affine buckets (Weierstrass) or msmBasic (projective buckets, twisted Edwards).
  // first_p (a segment run alone, remaining = 1): the problem's points start at record first_p of the set.
  int run_problems(const Handle& pts, const uint32_t* d_scalars, uint64_t n, uint32_t remaining, const msmz_opts& opt,
                   uint8_t* out, int* out_inf, msmz_log* log, uint32_t* ran, uint64_t first_p = 0) {
    const bool basic = TE || opt.buckets == MSMZ_BUCKETS_PROJECTIVE;
    const uint64_t per_pass = (opt.glv != 0 && !TE) ? pass_entries_ / 2 : pass_entries_;
    *ran = 1;
    const uint32_t bs = !basic && opt.reserved[0] != 1 && n <= per_pass && remaining > 1
                            ? planner_.batch_size(n, opt, (uint32_t)pts.n, pts.factor, remaining)
                            : 1;
    if (bs > 1) {
      Redo redo = Redo::NONE;   // (a GLV half longer than assumed: the whole sub-batch again)
      const int st = glv_retry(&redo, [&](int extra_bits, Redo* r) {
        return msm_weierstrass_affine(pts, pts.mem.template as<const uint32_t>(), d_scalars, n, opt, out, out_inf, log,
                                      extra_bits, bs, r);
      });
      if (st || redo != Redo::PER_PROBLEM) {
        if (!st) sub_batches_++;
        *ran = bs;
        return st;
      }
    }
    uint8_t part[RW * 4];
    int st = MSMZ_OK;
    for (uint64_t done = 0; done < n && st == MSMZ_OK; done += per_pass) {
      const uint64_t cnt = n - done < per_pass ? n - done : per_pass;
      range_passes_++;
      const uint32_t* d_points = pts.mem.template as<const uint32_t>() + (first_p + done) * PW_WORDS;
      const uint32_t* d_sc = d_scalars + done * 8;
      int pinf = 0;
      msmz_log plog;
      msmz_log* lp = log ? &plog : nullptr;
      if (lp) memset(lp, 0, sizeof(*lp));
      uint8_t* o = done == 0 ? out : part;
      int* oi = done == 0 ? out_inf : &pinf;
      if (basic) {
        st = msm_basic(pts, d_points, d_sc, cnt, opt, o, oi, lp);
      } else {
        Redo redo = Redo::NONE;
        st = glv_retry(&redo, [&](int extra_bits, Redo* r) {
          return msm_weierstrass_affine(pts, d_points, d_sc, cnt, opt, o, oi, lp, extra_bits, 1, r);
        });
      }
      if (st) break;
      if (done > 0) st = fold_partial(curve_id_, RW * 4, out, out_inf, part, pinf);
      if (log) merge_log(log, plog, done == 0, LogMerge::SEQUENTIAL);
    }
    return st;
  }

  // The next segments of one length class (order[0 .. remaining): indices into segs; n_max: the class's longest): the
  // decision of run_problems, taken for n_max.  Either a sub-batch of them in ONE batched pipeline planned for n_max, the
  // kernels reading each problem's offsets and length from a descriptor table (SegDesc; filled from pinned memory in
  // stream order, no host wait) -- or the first segment alone through the range loop of run_problems, the base pointers
  // advanced to it.  Results go to out / out_inf at the segments' own indices.  batchable: the offsets fit the table.
  int run_segments(const Handle& pts, const uint32_t* d_scalars, const msmz_segment* segs, const uint32_t* order,
                   uint32_t remaining, uint64_t n_max, bool batchable, const msmz_opts& opt, uint8_t* out, int* out_inf,
                   msmz_log* log, uint32_t* ran) {
    const bool basic = TE || opt.buckets == MSMZ_BUCKETS_PROJECTIVE;
    const uint64_t per_pass = (opt.glv != 0 && !TE) ? pass_entries_ / 2 : pass_entries_;
    *ran = 1;
    const uint32_t most = remaining < kMaxSegProblems ? remaining : kMaxSegProblems;
    const uint32_t bs = !basic && opt.reserved[0] != 1 && n_max <= per_pass && most > 1 && batchable
                            ? planner_.batch_size(n_max, opt, (uint32_t)pts.n, pts.factor, most)
                            : 1;
    if (bs > 1) {
      int st;
      if ((st = ensure_host_segs(bs)) || (st = segs_.ensure((size_t)bs * sizeof(SegDesc)))) return st;
      for (uint32_t p = 0; p < bs; p++) {
        const msmz_segment& s = segs[order[p]];
        h_segs_[p] = SegDesc{(uint32_t)s.first_s, (uint32_t)s.first_p, (uint32_t)s.n};
      }
      MSMZ_HIP(hipMemcpyAsync(segs_.p, h_segs_, (size_t)bs * sizeof(SegDesc), hipMemcpyHostToDevice, stream_));
      std::vector<uint8_t> res((size_t)bs * RW * 4);
      std::vector<int> inf(bs, 0);
      Redo redo = Redo::NONE;
      st = glv_retry(&redo, [&](int extra_bits, Redo* r) {
        return msm_weierstrass_affine(pts, pts.mem.template as<const uint32_t>(), d_scalars, n_max, opt, res.data(),
                                      inf.data(), log, extra_bits, bs, r, segs_.as<const SegDesc>());
      });
      if (st || redo != Redo::PER_PROBLEM) {
        if (!st) {
          sub_batches_++;
          for (uint32_t p = 0; p < bs; p++) {
            memcpy(out + (size_t)order[p] * RW * 4, res.data() + (size_t)p * RW * 4, RW * 4);
            out_inf[order[p]] = inf[p];
          }
        }
        *ran = bs;
        return st;
      }
    }
    const msmz_segment& s = segs[order[0]];
    uint32_t one = 0;
    return run_problems(pts, d_scalars + s.first_s * 8, s.n, 1, opt, out + (size_t)order[0] * RW * 4, out_inf + order[0], log,
                        &one, s.first_p);
  }
  static constexpr uint32_t kMaxSegProblems = 32768;   // problems of one pipeline = gridDim.y of the sort kernels

  // attempt(extra_bits, &redo): a GLV half longer than the assumed 127 bits (k_hist flags it) redoes the MSM with
  // windows for the PROVEN bound (Fr::GLV_PROVEN_BITS, tools/gen_constants.py), which no half can exceed -- a second
  // flag is an internal error.  *redo: what the last attempt asks beyond that (Redo::PER_PROBLEM).
  template <class Attempt>
  int glv_retry(Redo* redo, Attempt attempt) {
    int st = attempt(0, redo);
    if (*redo != Redo::PROVEN_BITS) return st;
    retries_++;
    *redo = Redo::NONE;
    st = attempt(1, redo);
    return *redo == Redo::PROVEN_BITS ? MSMZ_ERR_ARG : st;
  }

  // ------------------------------------------------------------------------------------------ shared phases
  Run new_run(const msmz_opts& opt) const {
    Run run;
    run.timing = opt.timing != 0;
    run.ev = ev_;
    return run;
  }
  void mark(const Run& run, hipEvent_t e) {
    if (run.timing) (void)hipEventRecord(e, stream_);
  }
  static float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
  }

  // scalars -> sorted references `refs_` + bucket offsets `off_` (+ meta->max_bucket); the sort's stage events.  No host
  // round trip.  pl.nprob > 1 (batched MSM): problem p reads scalars [p n, (p + 1) n); its bins follow problem p - 1's in
  // ONE exclusive scan, so refs_ / off_ come out as one dense sort of pl.nprob * nb buckets.  The two-level sort only.
  // `sl`: the planner's sort layout of pl; copy_stride: records per copy of a precomputed point set.
  // d_segs (segmented MSM): problem p's descriptor; d_scalars is then the whole set, pl.n the longest segment.
  int sort_phase(const Plan& pl, const SortLayout& sl, const uint32_t* d_scalars, Run& run, uint32_t copy_stride,
                 const SegDesc* d_segs = nullptr) {
    const uint32_t n = pl.n, M = pl.M, nb = pl.nb, nblocks = pl.nblocks, P = pl.nprob;
    const int c = pl.c, K = pl.K;
    int st;
    if ((st = refs_.ensure((size_t)P * K * M * 4))) return st;
    if ((st = off_.ensure(((size_t)P * nb + 1) * 4))) return st;
    MsmMeta* d_meta = meta_.as<MsmMeta>();
    MSMZ_HIP(hipMemsetAsync(d_meta, 0, sizeof(MsmMeta), stream_));
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
      MSMZ_HIP(hipMemsetAsync(d_counts, 0, pbins * 4, stream_));
      mark(run, run.ev.sort0);
      const uint32_t per_tile = pl.glv ? COARSE_TILE / 2 : COARSE_TILE;   // scalars per workgroup (k_hist and k_coarse)
      const uint32_t tiles = (n + per_tile - 1) / per_tile;
      if ((st = tilecnt_.ensure((size_t)P * tiles * nbins * 2))) return st;
      if ((st = tileoff_.ensure((size_t)P * tiles * nbins * 4 + kTraceBytes * tiles))) return st;   // the tiles' runs inside the bins
      const int cspec = sl.cspec;
      auto launch_sort = [&](auto glvc, auto cc, bool coarse) {
        constexpr bool G = decltype(glvc)::value;
        constexpr int C = decltype(cc)::value;
        if constexpr (!TE) {
          if (d_segs) {
            if (!coarse)
              hipLaunchKernelGGL((k_hist_seg<Fr, G, C>), dim3(tiles, P), dim3(COARSE_T), (size_t)nbins * 4, stream_, d_counts,
                                 tilecnt_.as<uint16_t>(), tileoff_.as<uint32_t>(), d_meta, d_scalars, g, nbins, d_segs);
            else
              hipLaunchKernelGGL((k_coarse_seg<Fr, G, C>), dim3(tiles, P), dim3(COARSE_T), (size_t)2 * nbins * 4, stream_,
                                 packed_.as<uint32_t>(), tileoff_.as<uint32_t>(), bins_.as<uint32_t>(),
                                 tilecnt_.as<uint16_t>(), d_scalars, g, nbins, d_segs);
            return;
          }
        }
        if (!coarse)
          hipLaunchKernelGGL((k_hist<Fr, G, C>), dim3(tiles, P), dim3(COARSE_T), (size_t)nbins * 4, stream_, d_counts,
                             tilecnt_.as<uint16_t>(), tileoff_.as<uint32_t>(), d_meta, d_scalars, g, nbins);
        else   // dynamic LDS <= kCoarseLdsMax (nbins <= SORT_MAX_BINS): the limit init() raised
          hipLaunchKernelGGL((k_coarse<Fr, G, C>), dim3(tiles, P), dim3(COARSE_T), (size_t)2 * nbins * 4, stream_,
                             packed_.as<uint32_t>(), tileoff_.as<uint32_t>(), bins_.as<uint32_t>(), tilecnt_.as<uint16_t>(),
                             d_scalars, g, nbins);
      };
      auto dispatch_sort = [&](bool coarse) {
        using std::integral_constant;
        if (pl.glv) {
          if constexpr (Fr::HAS_GLV) {
            if (cspec == 16) launch_sort(std::true_type{}, integral_constant<int, 16>{}, coarse);
            else launch_sort(std::true_type{}, integral_constant<int, 0>{}, coarse);
          }
        } else if (cspec == 17) {
          launch_sort(std::false_type{}, integral_constant<int, 17>{}, coarse);
        } else if (cspec == 16) {
          launch_sort(std::false_type{}, integral_constant<int, 16>{}, coarse);
        } else {
          launch_sort(std::false_type{}, integral_constant<int, 0>{}, coarse);
        }
      };
      dispatch_sort(false);
      mark(run, run.ev.hist_end);
      MSMZ_HIP(hipGetLastError());
      if (pbins <= (size_t)SORT_MAX_BINS) {
        hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(1024), 0, stream_, bins_.as<uint32_t>(), d_counts, (uint32_t)pbins,
                           &d_meta->n_entries);
      } else {   // a batch with more bins than one workgroup scans: the three-launch scan
        const uint32_t sblocks = (uint32_t)((pbins + SCAN_TILE - 1) / SCAN_TILE);
        if ((st = partials_.ensure((size_t)sblocks * 4))) return st;
        hipLaunchKernelGGL(k_scan_partials, dim3(sblocks, 1), dim3(SCAN_T), 0, stream_, partials_.as<uint32_t>(), d_counts,
                           (uint32_t)pbins, 0, sblocks);
        hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(SCAN_T), 0, stream_, partials_.as<uint32_t>(), sblocks,
                           &d_meta->n_entries);
        hipLaunchKernelGGL(k_scan_apply, dim3(sblocks, 1), dim3(SCAN_T), 0, stream_, bins_.as<uint32_t>(),
                           partials_.as<uint32_t>(), d_counts, (uint32_t)pbins, 0, sblocks, (size_t)0, (uint32_t*)nullptr);
      }
      mark(run, run.ev.scan_end);
      MSMZ_HIP(hipGetLastError());
      dispatch_sort(true);
      mark(run, run.ev.coarse_end);
      MSMZ_HIP(hipGetLastError());
      {
        const size_t lds = kFineLds;
        if (d_segs)
          hipLaunchKernelGGL(k_fine_seg, dim3(fbins, P), dim3(FINE_T), lds, stream_, refs_.as<uint32_t>(),
                             off_.as<uint32_t>(), &d_meta->max_bucket, packed_.as<uint32_t>(), bins_.as<uint32_t>(), g.fb,
                             g.fbt, sl.fine_top, fbins, g.idx_bits, n_half, pl.endo_delta, g.F, g.mbits, copy_stride, d_segs);
        else
          hipLaunchKernelGGL(k_fine, dim3(fbins, P), dim3(FINE_T), lds, stream_, refs_.as<uint32_t>(), off_.as<uint32_t>(),
                             &d_meta->max_bucket, packed_.as<uint32_t>(), bins_.as<uint32_t>(), g.fb, g.fbt, sl.fine_top,
                             fbins, g.idx_bits, n_half, pl.endo_delta, g.F, g.mbits, copy_stride);
      }
#ifdef MSMZ_TRACE
      // development aid: workgroup time stamps of k_coarse / k_fine (tools/wg_timeline.py)
      if ((st = trace_dump("k_coarse", tileoff_.as<uint32_t>() + (size_t)P * tiles * nbins, tiles, true))) return st;
      if ((st = trace_dump("k_fine", bins_.as<uint32_t>() + ((P * g.sbins + 2) & ~1u), fbins, false))) return st;
#endif
    } else {
      // fallback (window sizes whose coarse bins do not fit the LDS staging): digits materialized, one global
      // atomic per entry
      if (pl.fold_shift != 0) return MSMZ_ERR_ARG;   // (make_plan only folds when the two-level sort applies)
      if ((st = digits_.ensure((size_t)K * M * 4))) return st;
      if ((st = counts_.ensure(((size_t)nb + 1) * 4))) return st;
      if ((st = cursor_.ensure((size_t)nb * 4))) return st;
      if ((st = partials_.ensure((size_t)32 * nblocks * 4))) return st;
      MSMZ_HIP(hipMemsetAsync(counts_.p, 0, ((size_t)nb + 1) * 4, stream_));
      MSMZ_HIP(hipMemsetAsync(cursor_.p, 0, (size_t)nb * 4, stream_));
      const uint32_t dgrid = (n + 256 * DIGITS_ITEMS - 1) / (256 * DIGITS_ITEMS);
      mark(run, run.ev.sort0);
      if (pl.glv) {
        if constexpr (Fr::HAS_GLV)
          hipLaunchKernelGGL((k_digits<Fr, true>), dim3(dgrid), dim3(256), 0, stream_, digits_.as<uint32_t>(),
                             counts_.as<uint32_t>(), d_meta, d_scalars, n, c, K, pl.spread, pl.sbits ? pl.sbits : 256);
      } else {
        hipLaunchKernelGGL((k_digits<Fr, false>), dim3(dgrid), dim3(256), 0, stream_, digits_.as<uint32_t>(),
                           counts_.as<uint32_t>(), d_meta, d_scalars, n, c, K, pl.spread, pl.sbits ? pl.sbits : 256);
      }
      mark(run, run.ev.hist_end);
      MSMZ_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_scan_partials, dim3(nblocks, 1), dim3(SCAN_T), 0, stream_, partials_.as<uint32_t>(),
                         counts_.as<uint32_t>(), nb, 0, nblocks);
      hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(SCAN_T), 0, stream_, partials_.as<uint32_t>(), nblocks,
                         &d_meta->n_entries);
      hipLaunchKernelGGL(k_scan_apply, dim3(nblocks, 1), dim3(SCAN_T), 0, stream_, off_.as<uint32_t>(),
                         partials_.as<uint32_t>(), counts_.as<uint32_t>(), nb, 0, nblocks, (size_t)0,
                         &d_meta->max_bucket);
      mark(run, run.ev.scan_end);
      MSMZ_HIP(hipGetLastError());
      {
        dim3 grid((M + 256 * 4 - 1) / (256 * 4), K);
        hipLaunchKernelGGL(k_scatter, grid, dim3(256), 0, stream_, refs_.as<uint32_t>(), cursor_.as<uint32_t>(),
                           off_.as<uint32_t>(), digits_.as<uint32_t>(), M, c, pl.spread, n_half, pl.endo_delta);
      }
      mark(run, run.ev.coarse_end);
      MSMZ_HIP(hipGetLastError());
    }
    mark(run, run.ev.sort_end);
    MSMZ_HIP(hipGetLastError());
    return MSMZ_OK;
  }

  // read the device-side totals (one host round trip)
  int fetch_meta(Run& run) {
    MSMZ_HIP(hipMemcpyAsync(h_meta_, meta_.p, sizeof(MsmMeta), hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    run.max_bucket = h_meta_->max_bucket;
    run.n_entries = h_meta_->n_entries;
    run.rounds = h_meta_->rounds;
    memcpy(run.round_pairs, h_meta_->round_pairs, sizeof(run.round_pairs));
    memcpy(run.round_base, h_meta_->round_base, sizeof(run.round_base));
    return MSMZ_OK;
  }

  // reduce levels on accumulator records: rows in red_[cur*2], C in red_[cur*2+1]; ends with one entry per window
  template <class P>
  int reduce_levels(const ReduceKnobs& rk, int& cur, uint32_t n_in, uint32_t nprob) {
    constexpr int AW = P::ACC_WORDS;
    int st;
    while (n_in > rk.tail_n) {
      const uint32_t S = 4;   // quads handle short tails too
      uint32_t g2 = (n_in + S - 1) / S;
      int nxt = cur ^ 1;
      if ((st = red_[nxt * 2].ensure((size_t)nprob * g2 * AW * 4))) return st;
      if ((st = red_[nxt * 2 + 1].ensure((size_t)nprob * g2 * AW * 4))) return st;
      uint32_t total = nprob * g2;
      if (total <= rk.quad16_max) {
        // small level: latency-bound, one DPP quad per addition
        hipLaunchKernelGGL((k_reduce_quad16<P>), dim3((total * 16 + 63) / 64), dim3(64), 0, stream_,
                           red_[nxt * 2].as<uint32_t>(), red_[nxt * 2 + 1].as<uint32_t>(),
                           red_[cur * 2].as<uint32_t>(), red_[cur * 2 + 1].as<uint32_t>(), n_in, g2, total);
      } else {
        hipLaunchKernelGGL((k_reduce_quad<P>), dim3((total * 4 + 63) / 64), dim3(64), 0, stream_,
                           red_[nxt * 2].as<uint32_t>(), red_[nxt * 2 + 1].as<uint32_t>(),
                           red_[cur * 2].as<uint32_t>(), red_[cur * 2 + 1].as<uint32_t>(), n_in, g2, total);
      }
      n_in = g2;
      cur = nxt;
    }
    // the last levels (<= REDUCE_TAIL_N entries per window) in ONE launch, one workgroup per window; leaves the
    // window sums in final_
    {
      const int nxt = cur ^ 1;
      if ((st = red_[nxt * 2].ensure((size_t)nprob * n_in * AW * 4))) return st;
      if ((st = red_[nxt * 2 + 1].ensure((size_t)nprob * n_in * AW * 4))) return st;
      if ((st = final_.ensure((size_t)nprob * AW * 4))) return st;
      hipLaunchKernelGGL((k_reduce_tail<P>), dim3(nprob), dim3(REDUCE_TAIL_T), 0, stream_, red_[cur * 2].as<uint32_t>(),
                         red_[cur * 2 + 1].as<uint32_t>(), red_[nxt * 2].as<uint32_t>(), red_[nxt * 2 + 1].as<uint32_t>(),
                         final_.as<uint32_t>(), n_in, n_in);
    }
    return MSMZ_OK;
  }

  // copy the window results of all pl.nprob problems (the C entries of the last level; its rows are multiples of the
  // weight unit and not needed) to h_res_, and the meta block to the host
  int fetch_window_sums(const Plan& pl, size_t per_problem) {
    const size_t words = pl.nprob * per_problem * XW;
    if (int st = ensure_host_results(words)) return st;
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipMemcpyAsync(h_res_, final_.p, words * 4, hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipMemcpyAsync(h_meta_, meta_.p, sizeof(MsmMeta), hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return MSMZ_OK;
  }

  // twisted Edwards as a host group of host_horner (fp.h limbs)
  struct HostTe {
    using Pt = TeExt<F>;
    void set_inf(Pt& p) const { te_set_zero(p); }
    void dbl(Pt& r, const Pt& p) const { te_add(r, p, p); }
    void add_pt(Pt& r, const Pt& a, const Pt& b) const { te_add(r, a, b); }
    void load_pt(Pt& p, const uint32_t* w) const {
      fe_unpack<F>(p.X, w);
      fe_unpack<F>(p.Y, w + NW);
      fe_unpack<F>(p.Z, w + 2 * NW);
      fe_unpack<F>(p.T, w + 3 * NW);
    }
  };

  // The end of every MSM, after its bucket reduction: fetch the window results (two_d: two per bucket set, else one),
  // combine each problem's on the host (msm-batched-affine.ts:300-322) and fill the log.
  int finish_msm(const Plan& pl, Run& run, bool two_d, uint8_t* out, int* out_inf, msmz_log* log) {
    mark(run, run.ev.red_end);
    const size_t per_problem = (size_t)(two_d ? 2 : 1) * pl.Keff;
    // (the terms are listed while the device still reduces)
    const std::vector<WindowTerm> terms =
        window_terms(pl.c, pl.K, pl.Keff, (int)pl.F, two_d ? planner_.split_2d(pl).b : -1, pl.fold_shift != 0);
    int st = fetch_window_sums(pl, per_problem);
    if (st) return st;
    const auto t_host = std::chrono::steady_clock::now();
    if (h_meta_->error & 1u) return MSMZ_ERR_DEGENERATE;
    for (uint32_t p = 0; p < pl.nprob; p++) {
      const uint32_t* rp = h_res_ + p * per_problem * XW;
      uint32_t w[RW];
      if constexpr (TE) {
        te_to_affine_canon<F>(w, host_horner(HostTe{}, terms, rp, XW));
        out_inf[p] = 0;
      } else {
        // ~K*c dependent doublings: on 64-bit limbs (host64.h), ~4x faster on a CPU core than the kernels' limb code
        Xyzz<F> fin;
        host64_.to_xyzz(fin, host_horner(host64_, terms, rp, XW));
        out_inf[p] = xyzz_to_affine_canon<F>(w, fin) ? 1 : 0;
      }
      memcpy(out + (size_t)p * RW * 4, w, sizeof(w));
    }
    const float host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_host).count();
    fill_log(log, pl, run, host_ms);
    return MSMZ_OK;
  }

  // Two-dimensional bucket reduction (reduce2d_kernels.h): line sums, then the weighted sums over H lines of 2 Keff
  // problems with the upper-level kernels.  Leaves result 2 kw (rows) / 2 kw + 1 (columns) of bucket set kw in final_.
  // basic = true: the buckets are sums of partial accumulators (msmBasic path: slots_ + rscan_), else the affine bucket
  // sums of the tree rounds (bfin_).  sp: the planner's split of pl (planner_.split_2d); rk: which kernel a level runs.
  template <class P>
  int reduce_2d(const Plan& pl, const Split2d& sp, const ReduceKnobs& rk, const uint32_t* d_points, bool basic = false,
                bool summed = false) {
    const R2Geom g = r2_geom(pl, sp);
    int rows = 0;
    if (int st = line_sums_2d<P>(g, rk, d_points, basic, summed, &rows)) return st;
    return weighted_sums_2d<P>(g, rk, rows);
  }
  static R2Geom r2_geom(const Plan& pl, const Split2d& sp) {
    R2Geom g;
    g.L = pl.L;
    g.H = sp.H;
    g.D = sp.D;
    g.NC = sp.NC;
    g.chr = sp.D / sp.NC;
    g.chc = sp.H / sp.NC;
    g.nprob = 2u * pl.nprob * (uint32_t)pl.Keff;   // (all bucket sets of a batch)
    return g;
  }
  // first half: the partial sums of every line's chunks, then their pair sums; *rows = the red_ buffer (0 or 2) that
  // holds the g.nprob * g.H line sums
  template <class P>
  int line_sums_2d(const R2Geom& g, const ReduceKnobs& rk, const uint32_t* d_points, bool basic, bool summed, int* rows) {
    const uint32_t lines = g.nprob * g.H;
    const uint32_t total = lines * g.NC;
    int st;
    // ping-pong between red_[0] and red_[2] (rows of the level machinery); C inputs of the first level = infinity
    if ((st = red_[0].ensure((size_t)total * XW * 4))) return st;
    if ((st = red_[2].ensure((size_t)total * XW * 4))) return st;
    if (basic && summed) {   // one accumulator per bucket in bsum_ (k_bucket_sums)
      hipLaunchKernelGGL((k_reduce2d_partial_acc<P>), dim3((total + 127) / 128), dim3(128), 0, stream_,
                         red_[0].as<uint32_t>(), bsum_.as<uint32_t>(), (const uint32_t*)nullptr, g, total);
    } else if (basic) {
      hipLaunchKernelGGL((k_reduce2d_partial_acc<P>), dim3((total + 127) / 128), dim3(128), 0, stream_,
                         red_[0].as<uint32_t>(), slots_.as<uint32_t>(), rscan_.as<uint32_t>(), g, total);
    } else {
      if constexpr (!TE)
        hipLaunchKernelGGL((k_reduce2d_partial<F>), dim3((total + 127) / 128), dim3(128), 0, stream_,
                           red_[0].as<uint32_t>(), slots_.as<uint32_t>(), d_points, bfin_.as<uint4>(), g, total);
    }
    int src = 0;
    for (uint32_t n = total / 2; n >= lines && g.NC > 1; n /= 2) {
      const int dst = src ^ 2;
      if (n <= rk.pairsum_x4_max) {
        hipLaunchKernelGGL((k_pairsum_x4<P>), dim3((n * 4 + 63) / 64), dim3(64), 0, stream_, red_[dst].as<uint32_t>(),
                           red_[src].as<uint32_t>(), n);
      } else {
        hipLaunchKernelGGL((k_pairsum<P>), dim3((n + 127) / 128), dim3(128), 0, stream_, red_[dst].as<uint32_t>(),
                           red_[src].as<uint32_t>(), n);
      }
      src = dst;
      if (n == lines) break;
    }
    *rows = src;
    return MSMZ_OK;
  }
  // second half, the upper levels: rows = the line sums in red_[crow] (weight unit 1), C = infinity (all-zero records)
  template <class P>
  int weighted_sums_2d(const R2Geom& g, const ReduceKnobs& rk, int crow) {
    const uint32_t lines = g.nprob * g.H;
    const int ccol = crow + 1;
    int st;
    if ((st = red_[ccol].ensure((size_t)lines * XW * 4))) return st;
    hipLaunchKernelGGL((k_fill_neutral<P>), dim3((lines + 255) / 256), dim3(256), 0, stream_, red_[ccol].as<uint32_t>(), lines);
    int cur = crow >> 1;   // reduce_levels addresses rows as red_[cur * 2], C as red_[cur * 2 + 1]
    if ((st = reduce_levels<P>(rk, cur, g.H, g.nprob))) return st;
    MSMZ_HIP(hipGetLastError());
    return MSMZ_OK;
  }
  // the log of one MSM (or sub-batch): its plan, its run's totals and (timed) its stage events.  scatter_kernel_ms: the
  // scatter kernel alone (k_coarse / k_scatter), without k_fine.
  static void fill_log(msmz_log* log, const Plan& pl, const Run& run, float host_ms) {
    if (!log) return;
    log->c = pl.c;
    log->K = pl.K;
    log->rounds = (int)run.rounds;
    log->glv = pl.glv ? 1 : 0;
    log->n_entries = run.n_entries;
    log->n_pairs = run.n_pairs;
    log->max_bucket = run.max_bucket;
    log->stage_ms[MSMZ_ST_FINAL] = host_ms;
    if (!run.timing) return;
    const StageEvents& ev = run.ev;
    log->stage_ms[MSMZ_ST_DIGITS] = elapsed(ev.sort0, ev.hist_end);
    log->stage_ms[MSMZ_ST_SCAN] = elapsed(ev.hist_end, ev.scan_end);
    log->stage_ms[MSMZ_ST_SCATTER] = elapsed(ev.scan_end, ev.sort_end);
    log->scatter_kernel_ms = elapsed(ev.scan_end, ev.coarse_end);
    log->scatter_launches = 1;
    log->stage_ms[MSMZ_ST_PLAN] = elapsed(ev.plan0, ev.plan_end);
    log->stage_ms[MSMZ_ST_ACCUMULATE] = elapsed(ev.plan_end, ev.acc_end);
    log->stage_ms[MSMZ_ST_REDUCE] = elapsed(ev.acc_end, ev.red_end);
    hipEvent_t prev = ev.plan_end;
    for (uint32_t r = 0; r < run.rounds && r < 32; r++) {
      if (run.round_pairs[r] == 0) continue;
      log->batch_add_ms[r] = elapsed(prev, ev.round_end[r]);
      prev = ev.round_end[r];
    }
  }

  // The schedule of the tree rounds (plan_kernels.h) for the sorted buckets in off_ / refs_ (nb of them, all problems'),
  // cut into workgroups as pc says: desc_ <- one descriptor per addition of every round (room for desc_records), bfin_ <-
  // what the rounds leave of each bucket, meta <- rounds, entries, round sizes and bases.  Reads meta->max_bucket, which
  // the sort left.  No host round trip.
  int plan_phase(const PlanChunks& pc, uint32_t nb, int tail_skip, size_t desc_records, Run& run) {
    int st;
    MsmMeta* d_meta = meta_.as<MsmMeta>();
    mark(run, run.ev.plan0);
    const uint32_t n_chunks = pc.n_main + (nb - pc.nb_main + pc.chunk_top - 1) / pc.chunk_top;
    // chunk totals per round, then the per-workgroup scratch of the rounds beyond PLAN_RL
    const size_t pair_words = (size_t)n_chunks * (PLAN_RMAX - PLAN_RL) * PLAN_T;
    if ((st = rscan_.ensure(((size_t)PLAN_RMAX * n_chunks + pair_words) * 4 + kTraceBytes * n_chunks))) return st;
    if ((st = desc_.ensure(desc_records * 8))) return st;
    if ((st = bfin_.ensure((size_t)nb * 16))) return st;
    hipLaunchKernelGGL(k_plan_count, dim3(n_chunks), dim3(PLAN_T), 0, stream_, rscan_.as<uint32_t>(), off_.as<uint32_t>(),
                       nb, n_chunks, d_meta, tail_skip, pc);
    hipLaunchKernelGGL(k_plan_emit, dim3(n_chunks), dim3(PLAN_T), 0, stream_, desc_.as<uint2>(), bfin_.as<uint4>(),
                       d_meta, rscan_.as<uint32_t>(), off_.as<uint32_t>(), refs_.as<uint32_t>(), nb, n_chunks,
                       tail_skip, rscan_.as<uint32_t>() + (size_t)PLAN_RMAX * n_chunks, pc);
    MSMZ_HIP(hipGetLastError());
#ifdef MSMZ_TRACE
    if ((st = trace_dump("k_plan_emit", rscan_.as<uint32_t>() + (size_t)PLAN_RMAX * n_chunks + pair_words, n_chunks, false))) return st;
#endif
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ Weierstrass, affine buckets
  // nprob > 1: a batched MSM of nprob problems over the same points (scalars of problem p at d_scalars + p n 8, results
  // at out + p 2 FE_BYTES / out_inf[p]): one sort, one plan, one train of tree rounds and one two-dimensional reduction
  // over nprob * Keff bucket sets.  *redo: Redo::PER_PROBLEM when this plan does not batch (the two-level sort only),
  // Redo::PROVEN_BITS when a GLV half is longer than the windows were sized for (glv_retry).
  // d_segs (run_segments): the nprob problems are segments of the scalar and point sets; n64 is the longest, d_points and
  // d_scalars the sets' starts.  Only the sort reads the table: what follows sees one dense sort, as for a batch.
  int msm_weierstrass_affine(const Handle& pts, const uint32_t* d_points, const uint32_t* d_scalars, uint64_t n64,
                             const msmz_opts& opt, uint8_t* out, int* out_inf, msmz_log* log, int extra_bits,
                             uint32_t nprob, Redo* redo, const SegDesc* d_segs = nullptr) {
    const bool glv = opt.glv != 0;
    if (glv && (!Fr::HAS_GLV || !pts.has_endo)) return MSMZ_ERR_UNSUPPORTED;
    Plan pl;
    const bool want_2d = opt.reserved[0] != 1;   // else reduceAffine: the batched-affine first level (reduce_affine.h)
    // precomputed point set: its copies carry windows [j F, (j + 1) F) into one bucket set (two-level sort, 2-D reduction)
    const uint32_t fac = pts.factor > 1 ? pts.factor : 1;
    if (fac > 1 && (!want_2d || glv != (pts.glv != 0))) return MSMZ_ERR_UNSUPPORTED;
    int st = planner_.make_plan(pl, n64, glv, opt, (uint32_t)pts.n, true, extra_bits, want_2d, nprob, fac);
    if (st) return st;
    const SortLayout sl = planner_.sort_layout(pl);
    if (fac > 1 && !sl.two_level) return MSMZ_ERR_ARG;   // (msmz_precompute_points refuses such sets)
    if (nprob > 1 && (!want_2d || !sl.two_level)) {
      *redo = Redo::PER_PROBLEM;
      return MSMZ_OK;
    }
    // location words hold a record index in 30 bits
    if ((uint64_t)nprob * pl.K * pl.M >= (1ull << 30)) return MSMZ_ERR_ARG;
    // whole groups of 64 records; + the records of the batched-affine first reduction level when it is selected
    const size_t f2_records = opt.reserved[0] == 1 ? (size_t)13 * pl.Keff * ((pl.L + 1) / 2) + 256 : 0;
    if ((st = slots_.ensure(((size_t)nprob * pl.K * pl.M + 64 + f2_records) * SlotFmt<F>::WORDS * 4))) return st;
    Run run = new_run(opt);
    if ((st = sort_phase(pl, sl, d_scalars, run, (uint32_t)pts.copy_stride, d_segs))) return st;
    const uint32_t nb = pl.nb * nprob;   // buckets of all problems
    MsmMeta* d_meta = meta_.as<MsmMeta>();

    // ---- plan: descriptors of every pair of every round + what is left of each bucket (plan_kernels.h)
    // the batched-affine first reduction level (opt.reserved[0] = 1) wants ONE sum per bucket: no rounds skipped
    const int tail_skip = want_2d ? tail_skip_2d_ : 0;
    if ((st = plan_phase(planner_.plan_chunks(pl), nb, tail_skip, (size_t)nprob * pl.K * pl.M, run))) return st;
    if ((st = fetch_meta(run))) return st;      // the ONE host round trip before the final fetch
    if (h_meta_->error & 4u) return MSMZ_ERR_RANGE;
    if (h_meta_->error & 2u) {
      *redo = Redo::PROVEN_BITS;
      return MSMZ_OK;
    }
    // (a plain set's bucket holds <= M <= 2^24 entries; a precomputed set's up to W M < 2^PLAN_RMAX, which pre_fits checked)
    if (run.max_bucket > (pl.F > 1 ? (1u << PLAN_RMAX) - 1u : (1u << 24))) return MSMZ_ERR_ARG;
    mark(run, run.ev.plan_end);
    const uint32_t R = run.rounds;
    for (uint32_t r = 0; r < R; r++) run.n_pairs += run.round_pairs[r];
    for (uint32_t r = 0; r < R; r++) {
      const uint32_t pairs = run.round_pairs[r];
      if (pairs == 0) continue;
      launch_batch_add(pairs, opt.safe != 0, d_points, desc_.as<uint2>() + run.round_base[r], run.round_base[r], d_meta);
#ifdef MSMZ_TRACE
      {
        char nm[32];
        snprintf(nm, sizeof nm, "k_batch_add round %d", r);
        const int B = batch_b(pairs);
        const uint32_t wgs = (pairs + MSMZ_BATCH_T * B - 1) / (MSMZ_BATCH_T * B);
        if ((st = trace_dump(nm, d_meta + 1, wgs < 65536 ? wgs : 65536, false))) return st;
      }
#endif
      mark(run, run.ev.round_end[r]);
    }
    mark(run, run.ev.acc_end);

    // ---- bucket reduction
    if (want_2d) {
      // two-dimensional: row / column sums of the buckets, then two half-length weighted sums per bucket set
      if ((st = reduce_2d<WeierPolicy<F>>(pl, planner_.split_2d(pl), reduce_knobs_, d_points))) return st;
    } else {
      // level 1 from affine bucket sums, then XYZZ levels down to one entry per window.  The weight-L bucket is folded
      // into element L/2, which must be the FIRST element of its group
      uint32_t S1 = planner_.first_group_size(pl);
      if (S1 > 8) S1 = 8;
      while (S1 > 1 && S1 * 2 > pl.L) S1 >>= 1;
      const uint32_t groups = (pl.L + S1 - 1) / S1;   // elements are weights 0..L-1 (weight L folded into L/2)
      if ((st = red_[0].ensure((size_t)pl.Keff * groups * XW * 4))) return st;
      if ((st = red_[1].ensure((size_t)pl.Keff * groups * XW * 4))) return st;
      if ((st = reduce_first_affine(pl, d_points, S1, groups, run.n_pairs, d_meta))) return st;
      int cur = 0;
      if ((st = reduce_levels<WeierPolicy<F>>(reduce_knobs_, cur, groups, (uint32_t)pl.Keff))) return st;
    }
    return finish_msm(pl, run, want_2d, out, out_inf, log);
  }

  // ------------------------------------------------------------------------------------------ msmBasic: projective / extended buckets
  // (msm-basic.ts:45-176; Weierstrass "projective fallback" parallel.ts:69-87 and the twisted-Edwards MSM)
  int msm_basic(const Handle& pts, const uint32_t* d_points, const uint32_t* d_scalars, uint64_t n64, const msmz_opts& opt,
                uint8_t* out, int* out_inf, msmz_log* log) {
    using P = typename std::conditional<TE, TePolicy<F>, WeierPolicy<F>>::type;
    // neither msmProjective (parallel.ts:69-87) nor the twisted-Edwards path (msm-basic.ts:4) uses the endomorphism
    if (opt.glv) return MSMZ_ERR_UNSUPPORTED;
    Plan pl;
    int st = planner_.make_plan(pl, n64, false, opt, (uint32_t)pts.n, false);
    if (st) return st;
    Run run = new_run(opt);
    if ((st = sort_phase(pl, planner_.sort_layout(pl), d_scalars, run, 0)) || (st = fetch_meta(run))) return st;
    if (h_meta_->error & 4u) return MSMZ_ERR_RANGE;
    run.n_pairs = run.n_entries;   // (no tree rounds: every entry is added into its chunk's accumulator)
    if ((st = partials_.ensure((size_t)32 * pl.nblocks * 4))) return st;
    constexpr int AW = P::ACC_WORDS;
    const uint32_t nb = pl.nb, nblocks = pl.nblocks;
    MsmMeta* d_meta = meta_.as<MsmMeta>();
    mark(run, run.ev.plan0);
    // chunk offsets: cscan[g] = sum_{g' < g} ceil(size / 2^chunk_shift); chunks of 64 entries unless some bucket is
    // very long (then ~sqrt of it: bounds both the chunk and the number of partial sums one reduction thread adds)
    int chunk_shift = chunk_shift_override_ > 0 ? chunk_shift_override_ : ACC_CHUNK_SHIFT;
    while ((1ull << (2 * chunk_shift)) < run.max_bucket) chunk_shift++;
    const int scan_mode = 2 | (chunk_shift << 4);
    if ((st = rscan_.ensure(((size_t)nb + 1) * 4))) return st;
    hipLaunchKernelGGL(k_scan_partials, dim3(nblocks, 1), dim3(SCAN_T), 0, stream_, partials_.as<uint32_t>(),
                       off_.as<uint32_t>(), nb, scan_mode, nblocks);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(SCAN_T), 0, stream_, partials_.as<uint32_t>(), nblocks,
                       d_meta->round_pairs);
    hipLaunchKernelGGL(k_scan_apply, dim3(nblocks, 1), dim3(SCAN_T), 0, stream_, rscan_.as<uint32_t>(),
                       partials_.as<uint32_t>(), off_.as<uint32_t>(), nb, scan_mode, nblocks, (size_t)0, (uint32_t*)nullptr);
    MSMZ_HIP(hipMemcpyAsync(h_meta_, d_meta, sizeof(MsmMeta), hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    const uint32_t n_chunks = h_meta_->round_pairs[0];
    mark(run, run.ev.plan_end);
    if ((st = slots_.ensure((size_t)(n_chunks + 1) * AW * 4))) return st;
    if (n_chunks > 0) {
      hipLaunchKernelGGL((k_bucket_accumulate<P>), dim3((n_chunks + 127) / 128), dim3(128), 0, stream_,
                         slots_.as<uint32_t>(), d_points, refs_.as<uint32_t>(), off_.as<uint32_t>(),
                         rscan_.as<uint32_t>(), nb, n_chunks, chunk_shift);
    }
    mark(run, run.ev.acc_end);
    // every bucket is visited twice: buckets of several chunk accumulators (large inputs: Pallas 2^22 has 4,
    // ed-on-bls12-377 2^24 has 8) are first summed into one accumulator each, in bucket order
    const bool summed = (uint64_t)n_chunks * 2 > (uint64_t)nb * 3 && !no_bucket_sums_;
    if (summed && (st = bucket_sums<P>(nb))) return st;
    if ((st = reduce_2d<P>(pl, planner_.split_2d(pl), reduce_knobs_, d_points, true, summed))) return st;
    return finish_msm(pl, run, true, out, out_inf, log);
  }
  // bsum_[g] = sum of the chunk accumulators slots_[rscan_[g] .. rscan_[g+1]) of bucket g < nb
  template <class P>
  int bucket_sums(uint32_t nb) {
    if (int st = bsum_.ensure((size_t)nb * P::ACC_WORDS * 4)) return st;
    hipLaunchKernelGGL((k_bucket_sums<P>), dim3((nb + 127) / 128), dim3(128), 0, stream_, bsum_.as<uint32_t>(),
                       slots_.as<uint32_t>(), rscan_.as<uint32_t>(), nb);
    return MSMZ_OK;
  }

  // Batched-affine first level of the bucket reduction (reduce_affine.h): S - 1 chain steps and
  // a short pair tree, every launch over Keff * groups (x pairs per group) additions; results behind the tree rounds'
  // records.  Leaves the scaled (row, tri) XYZZ records in red_[0] / red_[1] for reduce_levels.
  int reduce_first_affine(const Plan& pl, const uint32_t* d_points, uint32_t S, uint32_t groups, uint64_t tree_pairs,
                          MsmMeta* d_meta) {
    F2Geom g;
    memset(&g, 0, sizeof(g));
    g.L = pl.L;
    g.S = S;
    g.groups = groups;
    g.NG = (uint32_t)pl.Keff * groups;
    g.inf_slot = (uint32_t)((tree_pairs + 63) / 64 * 64);
    g.out0 = g.inf_slot + 64;
    uint32_t n_launch = 0, dsum = 0, osum = 0;
    for (uint32_t step = 1; step < S; step++) {
      g.ppg[n_launch] = 1;
      g.desc_off[n_launch] = dsum;
      g.out_off[n_launch] = osum;
      dsum += g.NG;
      osum += g.NG;
      n_launch++;
    }
    for (uint32_t n = S - 1; n > 1; n = n / 2 + (n & 1)) {
      g.ppg[n_launch] = n / 2;
      g.desc_off[n_launch] = dsum;
      g.out_off[n_launch] = osum;
      dsum += g.NG * (n / 2);
      osum += g.NG * (n / 2);
      n_launch++;
    }
    g.n_launches = n_launch;
    g.desc_off[n_launch] = dsum;   // (row, tri) locations of every group
    dsum += g.NG;
    if ((uint64_t)g.out0 + osum + 64 >= (1ull << 30)) return MSMZ_ERR_ARG;
    int st;
    if ((st = f2desc_.ensure((size_t)dsum * 8))) return st;
    // slots_ may have to grow: its contents (the tree rounds' results) must survive -> it was sized for this in advance
    if (((size_t)g.out0 + osum + 64) * SlotFmt<F>::WORDS * 4 > slots_.bytes) return MSMZ_ERR_HIP;
    MSMZ_HIP(hipMemsetAsync(slots_.as<uint32_t>() + slot_words(g.inf_slot), 0, (size_t)64 * SlotFmt<F>::WORDS * 4, stream_));
    hipLaunchKernelGGL(k_reduce_affine_desc, dim3((g.NG + 255) / 256), dim3(256), 0, stream_, f2desc_.as<uint2>(),
                       bfin_.as<uint4>(), g);
    for (uint32_t i = 0; i < n_launch; i++)
      launch_batch_add(g.NG * g.ppg[i], true, d_points, f2desc_.as<uint2>() + g.desc_off[i], g.out0 + g.out_off[i], d_meta);
    hipLaunchKernelGGL((k_reduce_affine_finish<F>), dim3((g.NG + 127) / 128), dim3(128), 0, stream_, red_[0].as<uint32_t>(),
                       red_[1].as<uint32_t>(), slots_.as<uint32_t>(), d_points, f2desc_.as<uint2>() + g.desc_off[n_launch],
                       bfin_.as<uint4>(), g);
    MSMZ_HIP(hipGetLastError());
    return MSMZ_OK;
  }
  static size_t slot_words(uint32_t rec) {   // host twin of slot_offset<F> (rec a multiple of 64)
    return (size_t)(rec >> 6) * (SlotFmt<F>::CH * 64) * 4;
  }

  // pairs per thread of a launch of `pairs` batched-affine additions: as many as keep >= ~2 workgroups per CU in
  // flight, capped at BMAX = 16 (measured per round at 2^20: 7.6 M pairs B = 8..16, 3.7 M: 16, 1.8 M: 8, 0.9 M: 4,
  // < 0.3 M: 2; 32 is slower everywhere)
  int batch_b(uint32_t pairs) const {
    constexpr int T = MSMZ_BATCH_T, BMAX = MSMZ_BATCH_BMAX;
    int B = 1;
    while (B < BMAX && (uint64_t)pairs >= (uint64_t)T * (B * 2) * batch_min_wgs_) B *= 2;
    if (batch_b_override_ > 0) B = batch_b_override_ < BMAX ? batch_b_override_ : BMAX;
    return B;
  }

  // one launch of batched-affine additions: pairs `dsc[0 .. pairs)`, results in slot records out_base + t
  void launch_batch_add(uint32_t pairs, bool safe, const uint32_t* d_points, const uint2* dsc, uint32_t out_base,
                        MsmMeta* d_meta) {
    launch_batch_add_b(batch_b(pairs), pairs, safe, d_points, dsc, out_base, d_meta);
  }
  // ... with B pairs per thread (1 <= B <= MSMZ_BATCH_BMAX)
  void launch_batch_add_b(int B, uint32_t pairs, bool safe, const uint32_t* d_points, const uint2* dsc,
                          uint32_t out_base, MsmMeta* d_meta) {
    constexpr int T = MSMZ_BATCH_T, OCC = MSMZ_BATCH_OCC, BMAX = MSMZ_BATCH_BMAX;
    dim3 grid((pairs + T * B - 1) / (T * B)), block(T);
    if constexpr (!TE) {
      if (safe) {
        hipLaunchKernelGGL((k_batch_add<F, T, true, OCC, BMAX>), grid, block, 0, stream_, slots_.as<uint32_t>(),
                           d_points, dsc, out_base, pairs, B, d_meta);
      } else {
        hipLaunchKernelGGL((k_batch_add<F, T, false, OCC, BMAX>), grid, block, 0, stream_, slots_.as<uint32_t>(),
                           d_points, dsc, out_base, pairs, B, d_meta);
      }
    }
  }

  int ensure_gen_table() {
    if (gen_table_.p) return MSMZ_OK;
    int st = gen_table_.ensure((size_t)GEN_WINDOWS * GEN_TABLE * RW * 4);
    if (st) return st;
    // bases 2^(13 k) * G computed on the host, multiples on the device
    uint32_t bases[GEN_WINDOWS * RW];
    Affine<F> ga;
    fe_set_const<F>(ga.x, F::GX);
    fe_set_const<F>(ga.y, F::GY);
    if constexpr (TE) {
      TeExt<F> g;
      g.X = ga.x;
      g.Y = ga.y;
      fe_set_const<F>(g.Z, F::ONE);
      fe_mul(g.T, ga.x, ga.y);
      for (int k = 0; k < GEN_WINDOWS; k++) {
        Fe<F> zi, x, y;
        fe_inverse(zi, g.Z);
        fe_mul(x, g.X, zi);
        fe_mul(y, g.Y, zi);
        fe_store<F>(bases + k * RW, x);
        fe_store<F>(bases + k * RW + NW, y);
        for (int j = 0; j < GEN_BITS; j++) {
          TeExt<F> t;
          te_add(t, g, g);
          g = t;
        }
      }
    } else {
      Xyzz<F> g;
      xyzz_from_affine(g, ga);
      for (int k = 0; k < GEN_WINDOWS; k++) {
        Affine<F> a;
        host_xyzz_to_affine_mont(a, g);
        fe_store<F>(bases + k * RW, a.x);
        fe_store<F>(bases + k * RW + NW, a.y);
        for (int j = 0; j < GEN_BITS; j++) {
          Xyzz<F> t;
          xyzz_dbl(t, g);
          g = t;
        }
      }
    }
    st = stage_.ensure(sizeof(bases));
    if (st) return st;
    MSMZ_HIP(hipMemcpyAsync(stage_.p, bases, sizeof(bases), hipMemcpyHostToDevice, stream_));
    if constexpr (TE) {
      hipLaunchKernelGGL((k_te_gen_table<F>), dim3((GEN_WINDOWS * GEN_TABLE + 127) / 128), dim3(128), 0, stream_,
                         gen_table_.as<uint32_t>(), stage_.as<uint32_t>());
    } else {
      hipLaunchKernelGGL((k_gen_table<F>), dim3((GEN_WINDOWS * GEN_TABLE + 127) / 128), dim3(128), 0, stream_,
                         gen_table_.as<uint32_t>(), stage_.as<uint32_t>());
    }
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return MSMZ_OK;
  }

  static void host_xyzz_to_affine_mont(Affine<F>& a, const Xyzz<F>& p) {
    Fe<F> zi3, t, zi2;
    fe_inverse(zi3, p.ZZZ);
    fe_mul(t, zi3, p.ZZ);
    fe_sqr(zi2, t);
    fe_mul(a.x, p.X, zi2);
    fe_mul(a.y, p.Y, zi3);
  }

  // shared state -------------------------------------------------------------------------------
  int curve_id_, device_;
  hipStream_t stream_ = nullptr;
  StageEvents ev_{};
  hipEvent_t import_ev_ = nullptr;      // orders stream_ behind the stream that produces an imported device source
  std::vector<uint8_t> import_pack_;    // host packing of a strided host source
  std::map<uint64_t, Handle> handles_;
  uint64_t next_handle_ = 1;
  // Tuning knobs (the planning ones: PlanKnobs, plan.h).  A release build uses the constants; a development build
  // (-DMSMZ_DEV, tools/build_variant.sh) reads MSMZ_* environment variables when the context is created.  None of them
  // changes a result.
#ifdef MSMZ_DEV
  static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
#else
  static int env_int(const char*, int dflt) { return dflt; }
#endif
  uint32_t batch_min_wgs_ = (uint32_t)env_int("MSMZ_BATCH_WGS", 512);
  int chunk_shift_override_ = env_int("MSMZ_CHUNK_SHIFT", 0);
  const ReduceKnobs reduce_knobs_{(uint32_t)env_int("MSMZ_TAIL_N", REDUCE_TAIL_N), (uint32_t)env_int("MSMZ_QUAD16", 8192),
                                  (uint32_t)env_int("MSMZ_PAIRSUM_X4", 16384)};
  Host64<F> host64_;
  bool no_bucket_sums_ = env_int("MSMZ_NO_BUCKET_SUMS", 0) != 0;
  // rounds left to the 2-D reduction's loader: at most 2 (a bucket's final-location record holds 4 partial sums)
  int tail_skip_2d_ = env_int("MSMZ_TAIL_SKIP_2D", 1) > 2 ? 2 : env_int("MSMZ_TAIL_SKIP_2D", 1);
  int batch_b_override_ = env_int("MSMZ_BATCH_B", 0);
  int retries_ = 0;            // MSMs redone with the proven GLV bound (test hook reads it)
  // (half-)scalars one index-range pass of run_problems takes: kMaxEntriesPerPass unless msmz_test_set_limits lowered
  // it (the capacity checks keep the constant); what msmz_test_passes reports
  uint64_t pass_entries_ = kMaxEntriesPerPass;
  uint64_t range_passes_ = 0, sub_batches_ = 0;
  // window sizes, geometry, sort layout (plan.h), PlanKnobs in declaration order
  Planner<Fr> planner_{{env_int("MSMZ_NO_SPREAD", 0) != 0, env_int("MSMZ_NO_FOLD", 0) != 0,
                        env_int("MSMZ_NO_WINDOW_MODEL", 0) != 0, env_int("MSMZ_ATOMIC_SORT", 0) != 0,
                        env_int("MSMZ_NO_FBT", 0) != 0, env_int("MSMZ_NO_PLAN_TOP", 0) != 0,
                        env_int("MSMZ_NO_SORT_SPECIAL", 0) != 0, env_int("MSMZ_FB", 0), (uint32_t)env_int("MSMZ_S1", 0),
                        (uint32_t)env_int("MSMZ_R2_NC", 0)}};
  DevBuf bsum_, f2desc_, tilecnt_, tileoff_, final_, desc_, bfin_, packed_, bins_, digits_, counts_, off_, cursor_, refs_, rscan_, partials_, slots_, red_[4], meta_, stage_, gen_table_;
  MsmMeta* h_meta_ = nullptr;
  DevBuf sdot_;                      // scalars_dot: its result record, then one partial sum per tile
  DevBuf sscan_;                     // scalars_recurrence / _inverse: the result record, then aggregates and incoming values
  DevBuf check_;                     // check_points: its result record, then one verdict byte per point
  CheckResult* h_check_ = nullptr;   // pinned, grow-only landing of the result record and the verdict bytes behind it
  size_t h_check_bytes_ = 0;
  int ensure_host_check(size_t verdict_bytes) {
    const size_t need = sizeof(CheckResult) + verdict_bytes;
    if (need <= h_check_bytes_) return MSMZ_OK;
    if (h_check_) (void)hipHostFree(h_check_);
    h_check_ = nullptr;
    h_check_bytes_ = 0;
    MSMZ_HIP(hipHostMalloc(&h_check_, need));
    h_check_bytes_ = need;
    return MSMZ_OK;
  }
  DevBuf segs_;                  // run_segments: the descriptor table of a sub-batch ...
  SegDesc* h_segs_ = nullptr;    // ... and its pinned, grow-only host copy (rewritten only after the sub-batch's final fetch)
  size_t h_segs_n_ = 0;
  int ensure_host_segs(size_t n) {
    if (n <= h_segs_n_) return MSMZ_OK;
    if (h_segs_) (void)hipHostFree(h_segs_);
    h_segs_ = nullptr;
    h_segs_n_ = 0;
    MSMZ_HIP(hipHostMalloc(&h_segs_, n * sizeof(SegDesc)));
    h_segs_n_ = n;
    return MSMZ_OK;
  }
  uint32_t* h_res_ = nullptr;   // pinned, grow-only: the window results of every problem of an MSM (fetch_window_sums)
  size_t h_res_words_ = 0;
  int ensure_host_results(size_t words) {
    if (words <= h_res_words_) return MSMZ_OK;
    if (h_res_) (void)hipHostFree(h_res_);
    h_res_ = nullptr;
    h_res_words_ = 0;
    MSMZ_HIP(hipHostMalloc(&h_res_, words * 4));
    h_res_words_ = words;
    return MSMZ_OK;
  }
  TestHooks<Cfg> hooks_{*this};
};

}  // namespace msmz

// The resident sets of one engine: point and scalar sets kept on one GPU under handles, and every operation on them
// that is not an MSM -- uploads, imports from host or device memory, generators, downloads, the point checks, per-point
// multiplication and the arithmetic mod q over scalar sets.  One HIP stream; every entry point returns with the stream
// drained.  Engine<Cfg> (engine.h) derives from this and adds the MSM pipeline, which runs on the same stream and reports
// through the same error word.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <deque>
#include <new>
#include <vector>

#include "../../include/msmz.h"
#include "kernels.h"
#include "gen_kernels.h"
#include "fixed_kernels.h"
#include "import_kernels.h"
#include "export_kernels.h"
#include "check_kernels.h"
#include "mul_kernels.h"
#include "scalar_kernels.h"
#include "lookup_kernels.h"
#include "matrix_kernels.h"
#include "mle_kernels.h"
#include "ntt_kernels.h"
#include "iengine.h"
#include "store.h"

namespace msmz {

template <class Cfg>
class ResidentSets : public IEngine {
 protected:
  using F = typename Cfg::F;
  using Fr = typename Cfg::Fr;
  static constexpr int NW = F::NW;
  static constexpr int RW = 2 * NW;      // affine record words
  static constexpr int FE_BYTES = NW * 4;
  using P = typename Cfg::P;             // the group policy: formulas and record formats (kernels.h)
  static constexpr bool TE = Cfg::TE;
  static constexpr int PW_WORDS = P::IN_WORDS;   // words between the records of a resident point set

  explicit ResidentSets(int device) : device_(device) {}

  // the device, the stream, and the pinned landing of the meta block (Engine::init goes on from here)
  int init_sets() {
    MSMZ_HIP(hipSetDevice(device_));
    MSMZ_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    MSMZ_HIP(hipEventCreateWithFlags(&import_ev_, hipEventDisableTiming));
    poison_.stream = stream_;
    gen_table_.poison = &poison_;   // (the scratch buffers: bound by Engine::init, through its each_scratch)
    return h_meta_.ensure(sizeof(MsmMeta));
  }

  // f(buffer) for every scratch buffer of the operations here: undefined at the start of every call.  Not
  // among them, because they hold what stays valid across calls: the records of the handles, gen_table_ and the two
  // caches -- those are bound to poison_ too, so a NEW one is filled when the engine is armed, but never refilled.
  template <class Fn>
  void each_scratch(Fn f) {
    f(stage_), f(meta_), f(sdot_), f(mat_carry_), f(sscan_), f(ntt_scratch_), f(ntt_coset_), f(check_);
    f(lookup_slots_), f(lookup_count_), f(lookup_res_);
  }

 public:
  ~ResidentSets() override {   // (the device buffers and handles free themselves after this, on this device)
    (void)hipSetDevice(device_);
    if (import_ev_) (void)hipEventDestroy(import_ev_);
    if (stream_) (void)hipStreamDestroy(stream_);
  }

  // ------------------------------------------------------------------------------------------ data
  int upload_points(const uint8_t* xy, const uint8_t* inf, uint64_t n, uint64_t* h, const GenMap* split = nullptr) override {
    if (!xy || !h || !points_fit(n)) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    int st = stage_.ensure(n * RW * 4 + n);
    if (st) return st;
    if ((st = copy_h2d(stage_.p, xy, (size_t)RW * 4, n, split))) return st;
    uint8_t* d_inf = nullptr;
    if (inf) {
      d_inf = stage_.as<uint8_t>() + n * RW * 4;
      if ((st = copy_h2d(d_inf, inf, 1, n, split))) return st;
    }
    Handle hd;
    if ((st = new_points(n, &hd))) return st;
    st = checked([&](uint32_t* d_err) {   // a coordinate >= p
      hipLaunchKernelGGL((k_points_to_resident<P>), dim3((n + 255) / 256), dim3(256), 0, stream_, hd.mem.as<uint32_t>(),
                         stage_.as<uint32_t>(), d_inf, (uint32_t)n, hd.has_endo ? 1 : 0, d_err);
    });
    return st ? st : add_handle(std::move(hd), h);
  }

  int upload_scalars(const uint8_t* s, uint64_t n, uint64_t* h, const GenMap* split = nullptr) override {
    if (!s || !h || n == 0) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    int st;
    if ((st = new_scalars(n, &hd)) || (st = copy_h2d(hd.mem.p, s, 32, n, split))) return st;
    st = checked([&](uint32_t* d_err) {   // a scalar >= group order
      hipLaunchKernelGGL((k_check_scalars<Fr>), dim3((n + 255) / 256), dim3(256), 0, stream_, d_err,
                         hd.mem.as<const uint32_t>(), (uint32_t)n);
    });
    return st ? st : add_handle(std::move(hd), h);
  }

  // ------------------------------------------------------------------------------------------ imports
  int import_scalars(const msmz_src& s, uint64_t n, uint64_t* h, const GenMap* split = nullptr) override {
    if (!h || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    ImportView v;
    int st;   // (the source is checked before the allocation, which comes before any copy is queued)
    if ((st = src_check(&s, 0, &v.width, &v.stride)) || (st = new_scalars(n, &hd)) || (st = import_view(s, 0, n, split, &v)))
      return st;
    if ((st = import_scalars_to(hd.mem.as<uint32_t>(), s, v, n))) return st;
    return add_handle(std::move(hd), h);
  }

  // a new scalar set of n zeros: the target of import_scalars_into when a batch is assembled vector by vector
  int alloc_scalars(uint64_t n, uint64_t* h) override {
    if (!h || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    if (int st = new_scalars(n, &hd)) return st;
    MSMZ_HIP(hipMemsetAsync(hd.mem.p, 0, n * 32, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return add_handle(std::move(hd), h);
  }

  int import_scalars_into(uint64_t h, uint64_t first, const msmz_src& s, uint64_t n) override {
    uint32_t* dst = handles_.range(h, 1, first, n, 8);
    if (!dst || n == 0) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    ImportView v;
    if (int st = import_view(s, 0, n, nullptr, &v)) return st;
    return import_scalars_to(dst, s, v, n);
  }

  int import_points(const msmz_src& s, uint64_t n, uint64_t* h, const GenMap* split = nullptr) override {
    if (!h || !points_fit(n)) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    ImportView v;
    int st;
    const int mont = (s.flags & MSMZ_SRC_MONTGOMERY) ? 1 : 0;
    Handle hd;   // (the source is checked before the allocation, which comes before any copy is queued)
    if ((st = src_check(&s, FE_BYTES, &v.width, &v.stride)) || (st = new_points(n, &hd)) ||
        (st = import_view(s, FE_BYTES, n, split, &v)))
      return st;
    st = checked([&](uint32_t* d_err) {   // a coordinate (either form) >= p; a compressed record that is no point
      if (s.flags & MSMZ_SRC_COMPRESSED)
        hipLaunchKernelGGL((k_import_points_compressed<P>), dim3((n + 255) / 256), dim3(256), 0, stream_,
                           hd.mem.as<uint32_t>(), v.ptr, v.stride, v.is_inf, (uint32_t)n, hd.has_endo ? 1 : 0,
                           (s.flags & MSMZ_SRC_SIGN_PARITY) ? 1 : 0, d_err);
      else
        hipLaunchKernelGGL((k_import_points<P>), dim3((n + 255) / 256), dim3(256), 0, stream_, hd.mem.as<uint32_t>(), v.ptr,
                           v.stride, v.is_inf, (uint32_t)n, hd.has_endo ? 1 : 0, mont, d_err);
    });
    return st ? st : add_handle(std::move(hd), h);
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

  int random_points(uint64_t n, uint64_t seed, const GenMap& map, uint64_t* h) override {
    if (!h || !points_fit(n)) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    int st = ensure_gen_table();
    if (st) return st;
    Handle hd;
    if ((st = new_points(n, &hd))) return st;
    hipLaunchKernelGGL((k_gen_points<P>), dim3((n + 127) / 128), dim3(128), 0, stream_, hd.mem.as<uint32_t>(),
                       gen_table_.as<uint32_t>(), (uint32_t)n, seed, hd.has_endo ? 1 : 0, map);
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return add_handle(std::move(hd), h);
  }

  int random_scalars(uint64_t n, uint64_t seed, const GenMap& map, uint64_t* h) override {
    if (!h || n == 0) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    if (int st = new_scalars(n, &hd)) return st;
    hipLaunchKernelGGL((k_gen_scalars<Fr>), dim3((n + 255) / 256), dim3(256), 0, stream_, hd.mem.as<uint32_t>(),
                       (uint32_t)n, seed, map);
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return add_handle(std::move(hd), h);
  }

  int download_points(uint64_t hd, uint64_t first, uint64_t count, uint8_t* xy, uint8_t* inf) override {
    const Handle* pts = handles_.get(hd, 0);
    if (!pts || !xy) return MSMZ_ERR_ARG;
    // the endomorphism images stay readable; a precomputed set: all its copies
    const uint64_t have = pts->factor ? pts->copy_stride * pts->factor : pts->n * (pts->has_endo ? 2 : 1);
    if (!in_range(first, count, have)) return MSMZ_ERR_ARG;
    if (count == 0) return MSMZ_OK;
    MSMZ_HIP(hipSetDevice(device_));
    int st = stage_.ensure(count * RW * 4);
    if (st) return st;
    const uint32_t* recs = pts->mem.template as<const uint32_t>() + first * PW_WORDS;
    hipLaunchKernelGGL((k_points_from_resident<P>), dim3((count + 255) / 256), dim3(256), 0, stream_,
                       stage_.as<uint32_t>(), recs, (uint32_t)count);
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

  // the records of download_points as one coordinate + sign bit each (k_points_compress); the infinity flags come from
  // the kernel, behind the records in the staging buffer
  int download_points_compressed(uint64_t hd, uint64_t first, uint64_t count, uint8_t* out, uint8_t* inf,
                                 uint32_t flags) override {
    const Handle* pts = handles_.get(hd, 0);
    if (!pts || !out || (flags & ~(uint32_t)MSMZ_SRC_SIGN_PARITY)) return MSMZ_ERR_ARG;
    const uint64_t have = pts->factor ? pts->copy_stride * pts->factor : pts->n * (pts->has_endo ? 2 : 1);
    if (!in_range(first, count, have)) return MSMZ_ERR_ARG;
    if (count == 0) return MSMZ_OK;
    MSMZ_HIP(hipSetDevice(device_));
    if (int st = stage_.ensure(count * FE_BYTES + count)) return st;
    const uint32_t* recs = pts->mem.template as<const uint32_t>() + first * PW_WORDS;
    uint8_t* d_inf = stage_.as<uint8_t>() + count * FE_BYTES;
    hipLaunchKernelGGL((k_points_compress<P>), dim3((count + 255) / 256), dim3(256), 0, stream_, stage_.as<uint32_t>(),
                       d_inf, recs, (uint32_t)count, flags ? 1 : 0);
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipMemcpyAsync(out, stage_.p, count * FE_BYTES, hipMemcpyDeviceToHost, stream_));
    if (inf) MSMZ_HIP(hipMemcpyAsync(inf, d_inf, count, hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return MSMZ_OK;
  }

  int download_scalars(uint64_t hd, uint64_t first, uint64_t count, uint8_t* s) override {
    const uint32_t* src = handles_.range(hd, 1, first, count, 8);
    if (!src || !s) return MSMZ_ERR_ARG;
    if (count == 0) return MSMZ_OK;
    MSMZ_HIP(hipSetDevice(device_));
    MSMZ_HIP(hipMemcpy(s, src, count * 32, hipMemcpyDeviceToHost));
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ exports
  // msmz_export_scalars: entries [first, first + n) of a scalar set, `width` bytes each, where the destination says.
  // One launch (k_export_scalars); its error word (an entry >= q, or one that does not fit the width) comes back behind
  // the ONE host wait, after which everything has been written.
  int export_scalars(uint64_t hd, uint64_t first, uint64_t n, const msmz_dst& d) override {
    ExportView v;
    if (int st = dst_check(&d, 0, &v.width, &v.stride)) return st;
    const uint32_t* src = handles_.range(hd, 1, first, n, 8);
    if (!src || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    if (int st = export_view(d, n, &v)) return st;
    return export_run(d, n, v, [&](uint32_t* d_err) {
      hipLaunchKernelGGL((k_export_scalars<Fr>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream_, v.ptr, v.stride,
                         (int)(v.width / 4), src, (uint32_t)n, (d.flags & MSMZ_SRC_MONTGOMERY) ? 1 : 0, d_err);
    });
  }

  // msmz_export_points: records [first, first + n) of a point set under the range rules of download_points, as x || y
  // (canonical or Montgomery) or compressed, with the flag bytes if the destination has room for them.  One launch
  // (k_export_points); no kernel raises an error bit here, the fetch of the error word is the host wait.
  int export_points(uint64_t hd, uint64_t first, uint64_t n, const msmz_dst& d) override {
    ExportView v;
    if (int st = dst_check(&d, FE_BYTES, &v.width, &v.stride)) return st;
    const Handle* pts = handles_.get(hd, 0);
    if (!pts || n == 0) return MSMZ_ERR_ARG;
    // the endomorphism images stay readable; a precomputed set: all its copies
    const uint64_t have = pts->factor ? pts->copy_stride * pts->factor : pts->n * (pts->has_endo ? 2 : 1);
    if (!in_range(first, n, have)) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    if (int st = export_view(d, n, &v)) return st;
    const uint32_t* recs = pts->mem.template as<const uint32_t>() + first * PW_WORDS;
    const int form = (int)(d.flags & (MSMZ_SRC_MONTGOMERY | MSMZ_SRC_COMPRESSED | MSMZ_SRC_SIGN_PARITY));
    return export_run(d, n, v, [&](uint32_t*) {
      hipLaunchKernelGGL((k_export_points<P>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream_, v.ptr, v.stride,
                         v.is_inf, recs, (uint32_t)n, form);
    });
  }

  int free_handle(uint64_t hd) override {
    if (!handles_.known(hd)) return MSMZ_ERR_ARG;
    (void)hipSetDevice(device_);
    handles_.erase(hd);
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ validation
  // msmz_check_points: the curve equation, then (if asked, and unless the curve has cofactor 1) [q]P = O, over base
  // points [first, first + count) of a plain point handle.  A query: bad points are reported, not refused.  Two launches,
  // then the result record and the verdict bytes come back behind ONE host wait, like the error word of an upload.
  int check_points(uint64_t hd, uint64_t first, uint64_t count, uint32_t what, msmz_check_result* out,
                   uint8_t* verdicts) override {
    if (!out || count == 0 || what == 0 || (what & ~(uint32_t)(MSMZ_CHECK_CURVE | MSMZ_CHECK_SUBGROUP))) return MSMZ_ERR_ARG;
    const Handle* pts = handles_.get(hd, 0);
    if (!pts) return MSMZ_ERR_ARG;
    if (pts->factor) return MSMZ_ERR_UNSUPPORTED;   // derived data: the source set is what a caller checks
    const uint32_t* recs = handles_.range(hd, 0, first, count, PW_WORDS);   // (base points only)
    if (!recs) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    if (int st = h_check_.ensure(sizeof(CheckResult) + (verdicts ? count : 0))) return st;
    if (int st = check_.ensure(sizeof(CheckResult) + count)) return st;
    CheckResult* d_res = check_.as<CheckResult>();
    uint8_t* d_verdicts = check_.as<uint8_t>() + sizeof(CheckResult);
    const dim3 grid((uint32_t)((count + 255) / 256)), block(256);
    MSMZ_HIP(hipMemsetAsync(d_res, 0, 8, stream_));
    MSMZ_HIP(hipMemsetAsync(&d_res->first_bad, 0xff, 4, stream_));
    const bool chain = (what & MSMZ_CHECK_SUBGROUP) && !Fr::PRIME_ORDER;   // cofactor 1: the curve is the subgroup
    hipLaunchKernelGGL((k_check_curve<P>), grid, block, 0, stream_, d_verdicts, d_res, recs, (uint32_t)count, (uint32_t)first);
    if (chain)
      hipLaunchKernelGGL((k_check_subgroup<P, Fr>), grid, block, 0, stream_, d_verdicts, d_res, recs, (uint32_t)count, (uint32_t)first);
    MSMZ_HIP(hipGetLastError());
    // both land in pinned memory (a copy into the caller's pageable buffer would block the host a second time)
    MSMZ_HIP(hipMemcpyAsync(h_check_.p, d_res, sizeof(CheckResult) + (verdicts ? count : 0), hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    const CheckResult* res = h_check_.as<const CheckResult>();
    if (verdicts) memcpy(verdicts, h_check_.as<const uint8_t>() + sizeof(CheckResult), count);
    out->off_curve = res->off_curve;
    out->off_subgroup = res->off_subgroup;
    out->first_bad = res->first_bad == 0xffffffffu ? UINT64_MAX : res->first_bad;
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ per-point multiplication
  // msmz_points_mul(_opts): a new plain point handle, record i = [s_i] P_i (+ Q_i).  One launch of the chain that
  // points_mul_chain picks from the options (mul_kernels.h); the error word (a resident scalar >= q or >= the caller's
  // bound) comes back behind the ONE host wait, like that of an upload.  (msmz.hip has checked the options' ranges.)
  int points_mul(const msmz_mul& m, const msmz_mul_opts& o, uint64_t n, uint64_t* h) override {
    if (!h || !points_fit(n)) return MSMZ_ERR_ARG;
    const Handle* pts = handles_.get(m.points_handle, 0);
    const Handle* add = m.addend_handle ? handles_.get(m.addend_handle, 0) : nullptr;
    if (!pts || (m.addend_handle && !add)) return MSMZ_ERR_ARG;
    if (m.scalars_handle ? !handles_.get(m.scalars_handle, 1) : !m.scalar) return MSMZ_ERR_ARG;
    if (pts->factor || (add && add->factor)) return MSMZ_ERR_UNSUPPORTED;   // derived data
    const uint32_t* d_p = handles_.range(m.points_handle, 0, m.first_p, n, PW_WORDS);
    const uint32_t* d_q = add ? handles_.range(m.addend_handle, 0, m.first_q, n, PW_WORDS) : nullptr;
    const uint32_t* S = m.scalars_handle ? handles_.range(m.scalars_handle, 1, m.first_s, n, 8) : nullptr;
    if (!d_p || (add && !d_q) || (m.scalars_handle && !S)) return MSMZ_ERR_ARG;
    const MulChain chain = points_mul_chain<Fr>((o.flags & MSMZ_MUL_SUBGROUP) != 0, o.scalar_bits);
    const int bound = o.scalar_bits == 0 || o.scalar_bits >= Fr::BITS ? Fr::BITS : o.scalar_bits;
    MulScalar bc{};
    if (!S) {
      if (int st = read_fr(m.scalar, bc.w, false)) return st;
      if (words_geq_pow2(bc.w, bound)) return MSMZ_ERR_RANGE;
    }
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    if (int st = new_points(n, &hd)) return st;
    const dim3 grid((uint32_t)((n + 255) / 256)), block(256);   // whole blocks: every wave reaches the inversion entire
    const int st = checked([&](uint32_t* d_err) {   // a resident scalar >= group order, or >= 2^bound
      if constexpr (Fr::HAS_GLV) {
        if (chain.kind == MUL_CHAIN_GLV) {
          MulGlvScalar g{};
          if (!S) glv_decompose<Fr>(g.k0, g.k1, g.neg0, g.neg1, bc.w);
          hipLaunchKernelGGL((k_points_mul_glv<P, Fr>), grid, block, 0, stream_, hd.mem.as<uint32_t>(), d_p, S, g, d_q,
                             (uint32_t)n, hd.has_endo ? 1 : 0, bound, d_err);
          return;
        }
      }
      if (chain.steps == Fr::BITS)   // no bound: the instance with compile-time loop bounds
        hipLaunchKernelGGL((k_points_mul<P, Fr, false>), grid, block, 0, stream_, hd.mem.as<uint32_t>(), d_p, S, bc, d_q,
                           (uint32_t)n, hd.has_endo ? 1 : 0, chain.steps, d_err);
      else
        hipLaunchKernelGGL((k_points_mul<P, Fr, true>), grid, block, 0, stream_, hd.mem.as<uint32_t>(), d_p, S, bc, d_q,
                           (uint32_t)n, hd.has_endo ? 1 : 0, chain.steps, d_err);
    });
    return st ? st : add_handle(std::move(hd), h);
  }

  // ------------------------------------------------------------------------------------------ fixed-base multiplication
  // msmz_points_fixed_base: a new plain point handle, record i = [s_(first_s + i)] B.  The base becomes canonical bytes
  // (a resident one: one record downloaded), the planner (fixed_base.h) picks the window width for n and the bound, the
  // table comes from the cache or is built now, and ONE launch of k_fixed_mul makes the points; its error word (a
  // resident scalar >= q or >= the caller's bound) comes back behind the ONE host wait, like that of msmz_points_mul.
  int points_fixed_base(const msmz_fixed_base& f, uint64_t n, uint64_t* h) override {
    if (!h || !points_fit(n)) return MSMZ_ERR_ARG;
    if (f.base_handle ? f.base_xy_le != nullptr : f.base_index != 0) return MSMZ_ERR_ARG;
    const uint32_t* S = handles_.range(f.scalars_handle, 1, f.first_s, n, 8);
    if (!S) return MSMZ_ERR_ARG;
    FixedKey key{};
    if (f.base_handle) {
      const Handle* b = handles_.get(f.base_handle, 0);
      if (!b) return MSMZ_ERR_ARG;
      if (b->factor) return MSMZ_ERR_UNSUPPORTED;   // derived data
      if (!in_range(f.base_index, 1, b->n)) return MSMZ_ERR_ARG;   // (base points only)
      if (int st = download_points(f.base_handle, f.base_index, 1, reinterpret_cast<uint8_t*>(key.xy), nullptr)) return st;
    } else if (f.base_xy_le) {
      memcpy(key.xy, f.base_xy_le, sizeof(key.xy));
      if (words_geq<NW>(key.xy, F::PW) || words_geq<NW>(key.xy + NW, F::PW)) return MSMZ_ERR_RANGE;
    } else {
      Fe<F> g, t;
      fe_set_const<F>(g, F::GX);
      fe_from_mont(t, g);
      fe_to_canon_words<F>(key.xy, t);
      fe_set_const<F>(g, F::GY);
      fe_from_mont(t, g);
      fe_to_canon_words<F>(key.xy + NW, t);
    }
    const int bits = fixed_base_bits(f.scalar_bits, Fr::BITS);
    const FixedPlan plan = fixed_window_ ? fixed_base_plan_forced(fixed_window_, bits, RW * 4)
                                         : fixed_base_plan(n, bits, TE, RW * 4);
    if (plan.c == 0) return MSMZ_ERR_ARG;   // (a forced width only: the planner always finds one)
    key.c = plan.c;
    key.K = plan.K;
    MSMZ_HIP(hipSetDevice(device_));
    const uint32_t* table = nullptr;
    if (int st = fixed_table(key, plan, &table)) return st;
    Handle hd;
    if (int st = new_points(n, &hd)) return st;
    const dim3 grid((uint32_t)((n + 255) / 256)), block(256);   // whole blocks: every wave reaches the inversion entire
    const int st = checked([&](uint32_t* d_err) {   // a resident scalar >= group order, or >= 2^bits
      if (bits == Fr::BITS)
        hipLaunchKernelGGL((k_fixed_mul<P, Fr, false>), grid, block, 0, stream_, hd.mem.as<uint32_t>(), table, S, (uint32_t)n,
                           hd.has_endo ? 1 : 0, plan.c, plan.K, bits, d_err);
      else
        hipLaunchKernelGGL((k_fixed_mul<P, Fr, true>), grid, block, 0, stream_, hd.mem.as<uint32_t>(), table, S, (uint32_t)n,
                           hd.has_endo ? 1 : 0, plan.c, plan.K, bits, d_err);
    });
    return st ? st : add_handle(std::move(hd), h);
  }

  int test_set_fixed_base_window(int c) override {
    if (c != 0 && fixed_base_plan_forced(c, Fr::BITS, RW * 4).c == 0) return MSMZ_ERR_ARG;
    fixed_window_ = c;
    return MSMZ_OK;
  }
  uint64_t test_fixed_base_tables() override { return fixed_built_; }

  // ------------------------------------------------------------------------------------------ scalar-set arithmetic
  // msmz_scalars_combine: out_i = x.c_i x.v_i (+ y.c_i y.v_i) into a new scalar handle or over a range of an existing
  // one.  One launch; the error word (a resident record >= q) comes back behind the ONE host wait.
  int scalars_combine(const msmz_scalar_term& x, const msmz_scalar_term* y, uint64_t n, uint64_t first_out,
                      uint64_t* out_handle) override {
    if (!out_handle || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    ScalarTerm t[2] = {};
    const msmz_scalar_term* in[2] = {&x, y};
    std::vector<Source> srcs;
    for (int k = 0; k < 2; k++) {
      if (!in[k]) continue;
      srcs.push_back({in[k]->handle, in[k]->first, &t[k].v});
      if (in[k]->coeff_handle) srcs.push_back({in[k]->coeff_handle, in[k]->coeff_first, &t[k].c});
    }
    uint32_t* out = nullptr;
    if (int st = resolve(srcs, n, first_out, *out_handle, &out)) return st;
    for (int k = 0; k < 2; k++) {
      if (!in[k] || in[k]->coeff_handle) continue;
      if (!in[k]->coeff) t[k].unit = 1;
      else if (int st = read_fr(in[k]->coeff, t[k].k.w, true)) return st;
    }
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    if (int st = fresh_out(n, &hd, &out)) return st;
    const int st = checked([&](uint32_t* d_err) {   // a resident record >= group order
      hipLaunchKernelGGL((k_scalars_combine<Fr>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream_, out, t[0], t[1],
                         (uint32_t)n, d_err);
    });
    return st || !hd.mem.p ? st : add_handle(std::move(hd), out_handle);
  }

  // msmz_scalars_dot: one partial sum per tile, one workgroup folds them; the result and the error word share a
  // 64-byte record in front of the partial sums and come back in ONE copy behind ONE host wait.
  int scalars_dot(uint64_t xh, uint64_t first_x, uint64_t yh, uint64_t first_y, uint64_t n, uint8_t* out) override {
    if (!out || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    if (!handles_.get(xh, 1) || (yh ? !handles_.get(yh, 1) : first_y != 0)) return MSMZ_ERR_ARG;
    const uint32_t* X = handles_.range(xh, 1, first_x, n, 8);
    const uint32_t* Y = yh ? handles_.range(yh, 1, first_y, n, 8) : nullptr;
    if (!X || (yh && !Y)) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    const uint32_t tiles = (uint32_t)((n + SDOT_TILE - 1) / SDOT_TILE);
    // words 0..7: the result, word 8: the error word, from word 16: the partial sums
    const int st = recorded(sdot_, 64 + (size_t)tiles * 32, [&](uint32_t* d_res) {
      hipLaunchKernelGGL((k_scalars_dot<Fr>), dim3(tiles), dim3(SDOT_THREADS), 0, stream_, d_res + 16, X, Y, (uint32_t)n, d_res + 8);
      hipLaunchKernelGGL((k_scalars_dot_fold<Fr>), dim3(1), dim3(SDOT_THREADS), 0, stream_, d_res, d_res + 16, tiles, Y ? 1 : 0);
    });
    if (st) return st;
    memcpy(out, h_res_.p, 32);
    return MSMZ_OK;
  }

  // msmz_scalars_powers: a new scalar handle, local entry i = base ratio^(set index of i).  The host builds the table of
  // ratio^(2^k) with fr.h; it travels as a kernel argument.
  int scalars_powers(const uint8_t* base, const uint8_t* ratio, uint64_t n, const GenMap& map, uint64_t* h) override {
    if (!h || !ratio || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    FrConst b{};
    uint32_t r[8];
    b.w[0] = 1;
    int st;
    if ((base && (st = read_fr(base, b.w, false))) || (st = read_fr(ratio, r, false))) return st;
    FrPowTable table;
    fr_pow_table<Fr>(table, r);
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    if ((st = new_scalars(n, &hd))) return st;
    const uint64_t threads = (n + SPOW_RUN - 1) / SPOW_RUN;
    hipLaunchKernelGGL((k_scalars_powers<Fr>), dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream_,
                       hd.mem.as<uint32_t>(), b, table, (uint32_t)n, map);
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return add_handle(std::move(hd), h);
  }

  // msmz_scalars_recurrence: three launches (tile aggregates, ONE workgroup of carries, apply); the final value and the
  // error word share a 64-byte record in front of the scratch and come back in ONE copy behind ONE host wait.
  int scalars_recurrence(const msmz_scalar_rec& r, uint64_t n, uint64_t first_out, uint64_t* out_handle,
                         uint8_t* last) override {
    if (!out_handle || n == 0 || n >> 32 || (r.flags & ~(uint32_t)(MSMZ_REC_REVERSE | MSMZ_REC_EXCLUSIVE)))
      return MSMZ_ERR_ARG;
    if (!r.a_handle && !r.a && !r.b_handle) return MSMZ_ERR_ARG;   // y_i = y_(i-1): nothing to do
    const uint32_t *A = nullptr, *B = nullptr;
    std::vector<Source> srcs;
    if (r.a_handle) srcs.push_back({r.a_handle, r.a_first, &A});
    if (r.b_handle) srcs.push_back({r.b_handle, r.b_first, &B});
    uint32_t* out = nullptr;
    if (int st = resolve(srcs, n, first_out, *out_handle, &out)) return st;
    FrConst k{}, init{};
    if (!r.a_handle && r.a)
      if (int st = read_fr(r.a, k.w, true)) return st;
    if (r.init) {
      if (int st = read_fr(r.init, init.w, false)) return st;
    } else if (!B) {
      init.w[0] = 1;
    }
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    if (int st = fresh_out(n, &hd, &out)) return st;
    const uint32_t tiles = (uint32_t)((n + SREC_TILE - 1) / SREC_TILE);
    // words 0..7: the final value, word 8: the error word; then the aggregates' A, their B, and tiles + 1 incoming values
    const int st = recorded(sscan_, 64 + ((size_t)tiles * 3 + 1) * 32, [&](uint32_t* d_res) {
      uint32_t* aggA = d_res + 16;
      uint32_t* aggB = aggA + (size_t)tiles * 8;
      uint32_t* incoming = aggB + (size_t)tiles * 8;
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
    });
    if (st) return st;
    if (last) memcpy(last, h_res_.p, 32);
    return hd.mem.p ? add_handle(std::move(hd), out_handle) : (int)MSMZ_OK;
  }

  // msmz_scalars_inverse: one launch; the error word and the zero count share the record
  int scalars_inverse(uint64_t h, uint64_t first, uint64_t n, uint64_t first_out, uint64_t* out_handle,
                      uint64_t* n_zero) override {
    if (!out_handle || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    const uint32_t* X = nullptr;
    uint32_t* out = nullptr;
    if (int st = resolve({{h, first, &X}}, n, first_out, *out_handle, &out)) return st;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    if (int st = fresh_out(n, &hd, &out)) return st;
    const uint64_t per_block = (uint64_t)SINV_THREADS * SINV_E;
    const int st = recorded(sscan_, 64, [&](uint32_t* d_res) {   // word 8: the error word, word 9: the zeros
      hipLaunchKernelGGL((k_scalars_inverse<Fr>), dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(SINV_THREADS), 0,
                         stream_, out, X, (uint32_t)n, d_res);
    });
    if (st) return st;
    if (n_zero) *n_zero = h_res_.template as<const uint32_t>()[9];
    return hd.mem.p ? add_handle(std::move(hd), out_handle) : (int)MSMZ_OK;
  }

  // msmz_scalars_ntt: one launch per pass of the plan (ntt_plan.h), in stream order, from the source through scratch to
  // the destination; the error word (a resident record >= q, raised by the first pass) comes back behind the ONE host
  // wait.  Twiddle tables: built on the device by k_scalars_powers in the same stream, cached per (log_n, root as used).
  int scalars_ntt(const msmz_ntt& t, uint64_t first_out, uint64_t* out_handle) override {
    const bool inverse = t.flags & MSMZ_NTT_INVERSE, coset = t.flags & MSMZ_NTT_COSET;
    if (!out_handle || t.count == 0 || (t.flags & ~(uint32_t)(MSMZ_NTT_INVERSE | MSMZ_NTT_COSET)) || coset != (t.shift != nullptr))
      return MSMZ_ERR_ARG;
    if (t.log_n > (uint32_t)Fr::TWO_ADICITY) return MSMZ_ERR_UNSUPPORTED;
    if (t.log_n >= 32) return MSMZ_ERR_ARG;
    const uint64_t n = 1ull << t.log_n, total = n * t.count, n_in = t.n_in ? t.n_in : n;
    if (total >> 32 || n_in > n || (inverse && n_in != n)) return MSMZ_ERR_ARG;
    const uint32_t* X = nullptr;
    uint32_t* out = nullptr;
    if (int st = resolve({{t.handle, t.first, &X, n_in * t.count}}, total, first_out, *out_handle, &out)) return st;
    uint32_t w[8], g[8];
    if (t.root) {
      if (int st = read_fr(t.root, w, false)) return st;
      if (!fr_is_primitive_root<Fr>(w, t.log_n)) return MSMZ_ERR_ARG;
    } else {
      fr_root_of_unity<Fr>(w, t.log_n);
    }
    if (coset) {
      if (int st = read_fr(t.shift, g, false)) return st;
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
    MSMZ_HIP(hipSetDevice(device_));
    const uint32_t P = call.plan.n_passes;
    // every allocation first: once a table build is queued nothing below returns before the stream is drained
    NttTableSpec lo, hi;
    if (coset) ntt_two_level_specs<Fr>(call.plan, g, inverse ? call.ninv.w : Fr::ONE, &lo, &hi);
    if (int st = ntt_scratch_.ensure((size_t)(P > 2 ? 2 : P - 1) * total * 32)) return st;
    if (int st = sscan_.ensure(64)) return st;
    if (coset)
      if (int st = ntt_coset_.ensure((size_t)(lo.count + hi.count) * 32)) return st;
    Handle hd;
    if (int st = fresh_out(total, &hd, &out)) return st;
    if (int st = ntt_twiddles(call.plan, w, &call.twiddles)) return st;
    if (coset) {
      ntt_fill(ntt_coset_.as<uint32_t>(), lo);
      ntt_fill(ntt_coset_.as<uint32_t>() + lo.count * 8, hi);
      call.coset = ntt_coset_.as<const uint32_t>();
    }
    const int st = recorded(sscan_, 64, [&](uint32_t* d_res) {   // word 8: the error word
      call.err = d_res + 8;
      uint32_t* scratch[2] = {ntt_scratch_.as<uint32_t>(), ntt_scratch_.as<uint32_t>() + (size_t)total * 8};
      const uint32_t* src = X;
      uint64_t stride = n_in;
      for (uint32_t j = 0; j < P; j++) {
        uint32_t* dst = j + 1 == P ? out : scratch[j & 1];
        const NttArgs a = ntt_pass_args(call, j, src, stride, dst);
        const dim3 grid(ntt_pass_tiles(a.pass), t.count < 65535u ? t.count : 65535u);
        hipLaunchKernelGGL((k_ntt_pass<Fr>), grid, dim3(NTT_THREADS), 0, stream_, a);
        src = dst;
        stride = n;
      }
    });
    return st || !hd.mem.p ? st : add_handle(std::move(hd), out_handle);
  }

  // ------------------------------------------------------------------------------------------ multilinear polynomials
  // msmz_scalars_eq_table: a new scalar handle, entry i = scale eq(r, i).  The host brings the point to Montgomery form;
  // it travels as a kernel argument (k_scalars_eq_table, mle_kernels.h).  One launch, no error word: nothing is read.
  int scalars_eq_table(const uint8_t* point, uint32_t n_vars, const uint8_t* scale, uint64_t* h) override {
    if (!h || n_vars > (uint32_t)MLE_MAX_VARS || (n_vars && !point)) return MSMZ_ERR_ARG;
    FrConst s{};
    FrEqPoint pt;
    s.w[0] = 1;
    int st;
    if ((scale && (st = read_fr(scale, s.w, false))) || (st = read_point(point, n_vars, &pt))) return st;
    const uint64_t n = 1ull << n_vars;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    if ((st = new_scalars(n, &hd))) return st;
    const uint64_t threads = (n + MLE_RUN - 1) / MLE_RUN;
    hipLaunchKernelGGL((k_scalars_eq_table<Fr>), dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream_,
                       hd.mem.as<uint32_t>(), s, pt, n_vars);
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return add_handle(std::move(hd), h);
  }

  // msmz_scalars_mle_eval: scalars_dot with the second operand generated -- one partial sum per tile of MLE_TILE
  // entries, the same fold, the same result record behind ONE host wait.
  int scalars_mle_eval(uint64_t xh, uint64_t first, uint32_t n_vars, const uint8_t* point, uint8_t* out) override {
    if (!out || n_vars > (uint32_t)MLE_MAX_VARS || (n_vars && !point)) return MSMZ_ERR_ARG;
    const uint64_t n = 1ull << n_vars;
    const uint32_t* X = handles_.range(xh, 1, first, n, 8);
    if (!X) return MSMZ_ERR_ARG;
    FrEqPoint pt;
    if (int st = read_point(point, n_vars, &pt)) return st;
    MSMZ_HIP(hipSetDevice(device_));
    const uint32_t tiles = (uint32_t)((n + MLE_TILE - 1) / MLE_TILE);
    // words 0..7: the result, word 8: the error word, from word 16: the partial sums
    const int st = recorded(sdot_, 64 + (size_t)tiles * 32, [&](uint32_t* d_res) {
      hipLaunchKernelGGL((k_scalars_mle_eval<Fr>), dim3(tiles), dim3(SDOT_THREADS), 0, stream_, d_res + 16, X, pt, n_vars, d_res + 8);
      hipLaunchKernelGGL((k_scalars_dot_fold<Fr>), dim3(1), dim3(SDOT_THREADS), 0, stream_, d_res, d_res + 16, tiles, 1);
    });
    if (st) return st;
    memcpy(out, h_res_.p, 32);
    return MSMZ_OK;
  }

  // msmz_scalars_mle_bind: one launch, one thread per output; the error word (a resident record >= q) comes back behind
  // the ONE host wait.  One table and the high variable: the two halves are two sources of `resolve`, so the destination
  // may be a half exactly or apart from both -- and the high half is refused here, as the header says.  Any other shape:
  // the whole source is one range of another length than the destination, which `resolve` lets meet nowhere.
  int scalars_mle_bind(const msmz_mle_bind& b, uint64_t first_out, uint64_t* out_handle) override {
    if (!out_handle || !b.r || b.n_vars == 0 || b.n_vars > (uint32_t)MLE_MAX_VARS || b.count == 0 ||
        (b.flags & ~(uint32_t)MSMZ_MLE_LOW))
      return MSMZ_ERR_ARG;
    const uint64_t n = 1ull << b.n_vars, h = n >> 1, total_in = n * b.count, total_out = h * b.count;
    if (total_in >> 32) return MSMZ_ERR_ARG;
    const bool low = (b.flags & MSMZ_MLE_LOW) != 0;
    const uint32_t* in = nullptr;
    uint32_t* out = nullptr;
    if (b.count == 1 && !low) {
      const uint32_t* hi = nullptr;
      if (!handles_.range(b.handle, 1, b.first, n, 8)) return MSMZ_ERR_ARG;   // (the whole source: first + h cannot wrap)
      if (*out_handle == b.handle && first_out == b.first + h) return MSMZ_ERR_ARG;
      if (int st = resolve({{b.handle, b.first, &in}, {b.handle, b.first + h, &hi}}, h, first_out, *out_handle, &out)) return st;
    } else if (int st = resolve({{b.handle, b.first, &in, total_in}}, total_out, first_out, *out_handle, &out)) {
      return st;
    }
    FrConst r{};
    if (int st = read_fr(b.r, r.w, true)) return st;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    if (int st = fresh_out(total_out, &hd, &out)) return st;
    const int st = checked([&](uint32_t* d_err) {   // a resident record >= group order
      hipLaunchKernelGGL((k_scalars_mle_bind<Fr>), dim3((uint32_t)((total_out + 255) / 256)), dim3(256), 0, stream_, out, in, r,
                         b.n_vars, (uint32_t)total_out, low ? 1 : 0, d_err);
    });
    return st || !hd.mem.p ? st : add_handle(std::move(hd), out_handle);
  }

  // msmz_scalars_sumcheck_round: degree + 1 partial sums per tile of MSC_TILE pair indices, one workgroup of the fold per
  // value; the values and the error word share a record of MSC_HEAD_BYTES in front of the partial sums and come back in
  // ONE copy behind ONE host wait.  The coefficients go to c 2^(256 f) here (fr_sc_coeff), f the factors of the term.
  int scalars_sumcheck_round(const msmz_sumcheck& s, uint32_t* degree, uint8_t* evals) override {
    if (!degree || !evals || !s.tables || !s.terms || s.n_tables < 1 || s.n_tables > (uint32_t)MSC_MAX_TABLES ||
        s.n_terms < 1 || s.n_terms > (uint32_t)MSC_MAX_TERMS || s.n_vars == 0 || s.n_vars > (uint32_t)MLE_MAX_VARS ||
        (s.flags & ~(uint32_t)MSMZ_MLE_LOW))
      return MSMZ_ERR_ARG;
    const uint64_t n = 1ull << s.n_vars;
    ScTables tab{};
    for (uint32_t j = 0; j < s.n_tables; j++)
      if (!(tab.p[j] = handles_.range(s.tables[j].handle, 1, s.tables[j].first, n, 8))) return MSMZ_ERR_ARG;
    FrScTerms T{};
    T.n_terms = s.n_terms;
    for (uint32_t k = 0; k < s.n_terms; k++) {
      const uint32_t m = s.terms[k].mask, f = (uint32_t)__builtin_popcount(m);
      if (m == 0 || (m >> s.n_tables) || f > (uint32_t)MSC_MAX_DEGREE) return MSMZ_ERR_ARG;
      T.mask[k] = m;
      if (f > T.degree) T.degree = f;
    }
    for (uint32_t k = 0; k < s.n_terms; k++) {
      uint32_t c[8] = {1, 0, 0, 0, 0, 0, 0, 0};
      if (s.terms[k].coeff)
        if (int st = read_fr(s.terms[k].coeff, c, false)) return st;
      fr_sc_coeff<Fr>(T.coeff[k], c, __builtin_popcount(T.mask[k]));
    }
    MSMZ_HIP(hipSetDevice(device_));
    const uint32_t half = (uint32_t)(n >> 1), tiles = (half + MSC_TILE - 1) / MSC_TILE, values = T.degree + 1;
    const int low = (s.flags & MSMZ_MLE_LOW) ? 1 : 0;
    const int st = recorded(sdot_, MSC_HEAD_BYTES + (size_t)values * tiles * 32, [&](uint32_t* d_res) {
      uint32_t* partial = d_res + MSC_HEAD_BYTES / 4;
      uint32_t* d_err = d_res + MSC_ERR_WORD;
#define MSMZ_SC_LAUNCH(NT)                                                                                           \
  case NT:                                                                                                           \
    hipLaunchKernelGGL((k_scalars_sumcheck_round<Fr, NT>), dim3(tiles), dim3(SDOT_THREADS), 0, stream_, partial, tab, T, \
                       half, low, d_err);                                                                            \
    break
      switch (s.n_tables) {
        MSMZ_SC_LAUNCH(1);
        MSMZ_SC_LAUNCH(2);
        MSMZ_SC_LAUNCH(3);
        MSMZ_SC_LAUNCH(4);
        MSMZ_SC_LAUNCH(5);
        MSMZ_SC_LAUNCH(6);
      }
#undef MSMZ_SC_LAUNCH
      static_assert(MSC_MAX_TABLES == 6, "one instance per table count");
      hipLaunchKernelGGL((k_scalars_dot_fold<Fr>), dim3(values), dim3(SDOT_THREADS), 0, stream_, d_res, (const uint32_t*)partial,
                         tiles, 0);
    }, MSC_HEAD_BYTES, MSC_ERR_WORD);
    if (st) return st;
    *degree = T.degree;
    memcpy(evals, h_res_.p, (size_t)values * 32);
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ sparse matrices
  // msmz_matrix_create: the host sorts the triples into the forms asked for (mat_sort_form), the device keeps them and
  // k_matrix_pack brings the values out of the caller's scalar set, in sorted order and in Montgomery form.  The error
  // word (a value >= q) comes back behind the ONE host wait, which also ends the copies out of the host vectors.
  int matrix_create(const msmz_sparse& s, uint64_t* h) override {
    if (!h || !s.row || !s.col || s.nnz == 0 || s.nnz >> 32 || s.n_rows == 0 || s.n_cols == 0 ||
        (s.flags & ~(uint32_t)(MSMZ_MAT_ROWS | MSMZ_MAT_COLS)))
      return MSMZ_ERR_ARG;
    const uint64_t nnz = s.nnz;
    const uint32_t* vals = nullptr;
    if (s.val_handle ? !(vals = handles_.range(s.val_handle, 1, s.val_first, nnz, 8)) : s.val_first != 0) return MSMZ_ERR_ARG;
    if (mat_first_bad_index(s.row, s.col, nnz, s.n_rows, s.n_cols) != nnz) return MSMZ_ERR_ARG;
    const uint32_t flags = s.flags ? s.flags : (uint32_t)MSMZ_MAT_ROWS;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    hd.form[0].poison = hd.form[1].poison = &poison_;
    hd.kind = 2, hd.n = nnz, hd.n_rows = s.n_rows, hd.n_cols = s.n_cols, hd.mat_flags = flags, hd.has_vals = vals != nullptr;
    std::vector<uint32_t> host[2];   // per form: seg, gidx, perm in a row; alive until the wait below
    const size_t val_off = mat_val_offset(nnz);
    if (int st = stage_.ensure(2 * nnz * 4)) return st;
    for (int f = 0; f < 2; f++) {
      if (!(flags & (f ? MSMZ_MAT_COLS : MSMZ_MAT_ROWS))) continue;
      try {
        host[f].resize(3 * nnz);
        mat_sort_form(f ? s.col : s.row, f ? s.row : s.col, nnz, f ? s.n_cols : s.n_rows, host[f].data(),
                      host[f].data() + nnz, host[f].data() + 2 * nnz);
      } catch (const std::bad_alloc&) {
        return MSMZ_ERR_HIP;   // (out of host memory: the sort needs 12 nnz + 8 n_rows bytes)
      }
      if (int st = hd.form[f].ensure(val_off + (vals ? nnz * 32 : 0))) return st;
    }
    // (everything that can fail without the device has been done: from here the stream reads the host vectors, and no
    // path leaves before a wait)
    hipError_t e = hipSuccess;
    for (int f = 0; f < 2 && e == hipSuccess; f++) {
      if (!hd.form[f].p) continue;
      const uint32_t* seg = host[f].data();
      e = hipMemcpyAsync(hd.form[f].p, seg, 2 * nnz * 4, hipMemcpyHostToDevice, stream_);
      if (e == hipSuccess && vals)
        e = hipMemcpyAsync(stage_.as<uint32_t>() + f * nnz, seg + 2 * nnz, nnz * 4, hipMemcpyHostToDevice, stream_);
    }
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(stream_);
      MSMZ_HIP(e);
    }
    const int st = checked([&](uint32_t* d_err) {   // a value >= group order
      for (int f = 0; f < 2 && vals; f++) {
        if (!hd.form[f].p) continue;
        hipLaunchKernelGGL((k_matrix_pack<Fr>), dim3((uint32_t)((nnz + 255) / 256)), dim3(256), 0, stream_,
                           (uint32_t*)(hd.form[f].template as<uint8_t>() + val_off), vals,
                           (const uint32_t*)(stage_.as<uint32_t>() + f * nnz), (uint32_t)nnz, d_err);
      }
    });
    return st ? st : add_handle(std::move(hd), h);
  }

  int matrix_info(uint64_t h, uint32_t* n_rows, uint32_t* n_cols, uint64_t* nnz, uint32_t* flags) override {
    const Handle* m = handles_.get(h, 2);
    if (!m) return MSMZ_ERR_ARG;
    if (n_rows) *n_rows = m->n_rows;
    if (n_cols) *n_cols = m->n_cols;
    if (nnz) *nnz = m->n;
    if (flags) *flags = m->mat_flags;
    return MSMZ_OK;
  }

  // msmz_matrix_mul: a clear of the destination, one tile per workgroup (k_matrix_mul), ONE workgroup that folds the tile
  // carries in (k_matrix_fold); the error word (an entry of x >= q that a non-zero reads) comes back behind the ONE host
  // wait.  x is gathered, so the destination may not meet its range at all.
  int matrix_mul(const msmz_matvec& v, uint64_t first_out, uint64_t* out_handle) override {
    if (!out_handle || (v.flags & ~(uint32_t)MSMZ_MATVEC_TRANSPOSE)) return MSMZ_ERR_ARG;
    const Handle* m = handles_.get(v.matrix, 2);
    const int f = (v.flags & MSMZ_MATVEC_TRANSPOSE) ? 1 : 0;
    if (!m || !m->form[f].p) return MSMZ_ERR_ARG;
    const uint64_t n_in = f ? m->n_rows : m->n_cols, n_out = f ? m->n_cols : m->n_rows, nnz = m->n;
    if (*out_handle && *out_handle == v.x_handle && ranges_meet(v.x_first, n_in, first_out, n_out)) return MSMZ_ERR_ARG;
    const uint32_t* X = nullptr;
    uint32_t* out = nullptr;
    if (int st = resolve({{v.x_handle, v.x_first, &X, n_in}}, n_out, first_out, *out_handle, &out)) return st;
    MSMZ_HIP(hipSetDevice(device_));
    const uint32_t tiles = (uint32_t)((nnz + MAT_TILE - 1) / MAT_TILE);
    if (int st = mat_carry_.ensure((size_t)tiles * MAT_CARRY_WORDS * 4)) return st;
    Handle hd;
    if (int st = fresh_out(n_out, &hd, &out)) return st;
    const uint8_t* base = m->form[f].template as<const uint8_t>();
    const MatView view = {(const uint32_t*)base + nnz, (const uint32_t*)base,
                          m->has_vals ? (const uint32_t*)(base + mat_val_offset(nnz)) : nullptr};
    const int st = checked([&](uint32_t* d_err) {   // an entry of x >= group order
      if (hipMemsetAsync(out, 0, n_out * 32, stream_) != hipSuccess) return;   // (fetch_error reports it)
      hipLaunchKernelGGL((k_matrix_mul<Fr>), dim3(tiles), dim3(MAT_THREADS), 0, stream_, out, view, X, (uint32_t)nnz,
                         mat_carry_.as<uint32_t>(), d_err);
      hipLaunchKernelGGL((k_matrix_fold<Fr>), dim3(1), dim3(MAT_THREADS), 0, stream_, out,
                         (const uint32_t*)mat_carry_.as<uint32_t>(), tiles);
    });
    return st || !hd.mem.p ? st : add_handle(std::move(hd), out_handle);
  }

  // ------------------------------------------------------------------------------------------ lookup arguments
  // msmz_scalars_lookup: the index and the counts are cleared (scratch is undefined at the start of a call), then
  // k_lookup_insert, k_lookup_count (k_lookup_count_small for a table of at most LK_SMALL_TABLE entries) and k_lookup_emit; the error word, the three result words and, if asked for, the
  // positions behind them come back in ONE copy behind the ONE host wait.  Both inputs are gathered, so the destination
  // may meet neither range at all.
  int scalars_lookup(const msmz_lookup& l, uint64_t first_out, uint64_t* out_handle, msmz_lookup_result* res) override {
    if (!out_handle || l.flags || l.table_n == 0 || l.col_n == 0 || l.table_n > LK_MAX_TABLE || l.col_n >> 32) return MSMZ_ERR_ARG;
    const uint64_t tn = l.table_n, cn = l.col_n;
    if (*out_handle && ((*out_handle == l.table_handle && ranges_meet(l.table_first, tn, first_out, tn)) ||
                        (*out_handle == l.col_handle && ranges_meet(l.col_first, cn, first_out, tn))))
      return MSMZ_ERR_ARG;
    const uint32_t* T = nullptr;
    const uint32_t* Fc = nullptr;
    uint32_t* out = nullptr;
    if (int st = resolve({{l.table_handle, l.table_first, &T, tn}, {l.col_handle, l.col_first, &Fc, cn}}, tn, first_out,
                         *out_handle, &out))
      return st;
    MSMZ_HIP(hipSetDevice(device_));
    const uint32_t slots = lk_slots(tn);
    const size_t res_bytes = (size_t)LK_RES_WORDS * 4 + (l.positions ? cn * 4 : 0);
    if (int st = lookup_slots_.ensure((size_t)slots * 4)) return st;
    if (int st = lookup_count_.ensure(tn * 4)) return st;
    if (int st = lookup_res_.ensure(res_bytes)) return st;
    if (int st = h_lookup_.ensure(res_bytes)) return st;
    Handle hd;
    if (int st = fresh_out(tn, &hd, &out)) return st;
    uint32_t* d_res = lookup_res_.as<uint32_t>();
    uint32_t* d_pos = l.positions ? d_res + LK_RES_WORDS : nullptr;
    MSMZ_HIP(hipMemsetAsync(lookup_slots_.p, 0xff, (size_t)slots * 4, stream_));
    MSMZ_HIP(hipMemsetAsync(lookup_count_.p, 0, tn * 4, stream_));
    MSMZ_HIP(hipMemsetAsync(d_res, 0, LK_RES_WORDS * 4, stream_));
    MSMZ_HIP(hipMemsetAsync(d_res + LK_RES_FIRST, 0xff, 4, stream_));
    const dim3 block(LK_THREADS), tgrid((uint32_t)((tn + LK_THREADS - 1) / LK_THREADS)),
        cgrid((uint32_t)((cn + LK_THREADS - 1) / LK_THREADS));
    hipLaunchKernelGGL((k_lookup_insert<Fr>), tgrid, block, 0, stream_, lookup_slots_.as<uint32_t>(), slots - 1, T, (uint32_t)tn, d_res);
    if (tn <= LK_SMALL_TABLE)
      hipLaunchKernelGGL((k_lookup_count_small<Fr>), dim3(lk_small_groups(cn)), block, 0, stream_, lookup_count_.as<uint32_t>(),
                         d_res, d_pos, lookup_slots_.as<uint32_t>(), slots - 1, T, (uint32_t)tn, Fc, (uint32_t)cn);
    else
      hipLaunchKernelGGL((k_lookup_count<Fr>), cgrid, block, 0, stream_, lookup_count_.as<uint32_t>(), d_res, d_pos,
                         lookup_slots_.as<uint32_t>(), slots - 1, T, Fc, (uint32_t)cn);
    hipLaunchKernelGGL((k_lookup_emit<Fr>), tgrid, block, 0, stream_, out, (const uint32_t*)lookup_count_.as<uint32_t>(), (uint32_t)tn);
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipMemcpyAsync(h_lookup_.p, d_res, res_bytes, hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    const uint32_t* w = h_lookup_.as<const uint32_t>();
    if (w[LK_RES_ERR]) return MSMZ_ERR_RANGE;   // (hd frees a fresh destination)
    if (l.positions) memcpy(l.positions, w + LK_RES_WORDS, cn * 4);
    if (res) {
      res->n_missing = w[LK_RES_MISSING];
      res->first_missing = w[LK_RES_FIRST] == LK_EMPTY ? UINT64_MAX : w[LK_RES_FIRST];
      res->n_distinct = w[LK_RES_DISTINCT];
    }
    return hd.mem.p ? add_handle(std::move(hd), out_handle) : MSMZ_OK;
  }

 protected:
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

  // record indices of a point set (incl. the endomorphism images) fit 30 bits
  static bool points_fit(uint64_t n) { return n != 0 && n < (1ull << (Cfg::HAS_ENDO ? 29 : 30)); }

  // a new handle and its device memory (owned by it: an error before add_handle frees it)
  int new_handle(Handle* hd, int kind, uint64_t n, bool endo, size_t bytes) {
    *hd = Handle{kind, n, endo};
    hd->mem.poison = hd->form[0].poison = hd->form[1].poison = &poison_;
    return hd->mem.alloc_exact(bytes);
  }
  int new_points(uint64_t n, Handle* hd) {
    if (!points_fit(n)) return MSMZ_ERR_ARG;
    return new_handle(hd, 0, n, Cfg::HAS_ENDO, (size_t)n * PW_WORDS * 4 * (Cfg::HAS_ENDO ? 2 : 1));
  }
  int new_scalars(uint64_t n, Handle* hd) { return new_handle(hd, 1, n, false, n * 32); }
  // the memory of a fresh destination (resolve left *out null): hd owns it until add_handle
  int fresh_out(uint64_t n, Handle* hd, uint32_t** out) {
    if (*out) return MSMZ_OK;
    if (int st = new_scalars(n, hd)) return st;
    *out = hd->mem.template as<uint32_t>();
    return MSMZ_OK;
  }
  int add_handle(Handle&& hd, uint64_t* h) {
    *h = handles_.add(std::move(hd));
    return MSMZ_OK;
  }

 private:
  // zeroes the error word, runs launch(its device address), fetches it: MSMZ_ERR_RANGE if a kernel raised a bit; bit 3
  // alone (k_import_points_compressed: a record that is no point) is MSMZ_ERR_POINT, so RANGE wins when both occur
  template <class Launch>
  int checked(Launch launch) {
    uint32_t* d_err = &meta_.as<MsmMeta>()->error;
    MSMZ_HIP(hipMemsetAsync(d_err, 0, 4, stream_));
    launch(d_err);
    uint32_t err = 0;
    if (int st = fetch_error(&err)) return st;
    return (err & ~8u) ? MSMZ_ERR_RANGE : err ? MSMZ_ERR_POINT : MSMZ_OK;
  }

  // The 64-byte result record of dot, recurrence and inverse at the head of `buf` (`bytes` with its scratch): zeroed in
  // stream order, written by launch(its device address), copied to h_res_ (pinned: Engine::init sized it for far more)
  // behind ONE wait.  Word 8 is the error word: MSMZ_ERR_RANGE if a resident record was >= the group order.  (A
  // sumcheck round has several values to bring back: its record is `head` bytes with the error word at `err_word`.)
  template <class Launch>
  int recorded(DevBuf& buf, size_t bytes, Launch launch, size_t head = 64, int err_word = 8) {
    if (int st = buf.ensure(bytes)) return st;
    MSMZ_HIP(hipMemsetAsync(buf.p, 0, head, stream_));
    launch(buf.as<uint32_t>());
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipMemcpyAsync(h_res_.p, buf.p, head, hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return h_res_.template as<const uint32_t>()[err_word] ? MSMZ_ERR_RANGE : MSMZ_OK;
  }

  // a broadcast scalar of the caller's (32 bytes, canonical): out = its words, or its Montgomery form; >= q is refused
  static int read_fr(const uint8_t* src, uint32_t out[8], bool to_mont) {
    uint32_t c[8];
    memcpy(c, src, 32);
    if (words_geq<8>(c, Fr::Q)) return MSMZ_ERR_RANGE;
    if (to_mont) fr_to_mont<Fr>(out, c);
    else memcpy(out, c, 32);
    return MSMZ_OK;
  }

  // the point of an eq table or an evaluation (n_vars values of 32 bytes, each < q) in the form the kernels take
  static int read_point(const uint8_t* point, uint32_t n_vars, FrEqPoint* pt) {
    memset(pt, 0, sizeof(*pt));
    for (uint32_t j = 0; j < n_vars; j++)
      if (int st = read_fr(point + (size_t)32 * j, pt->r[j], true)) return st;
    return MSMZ_OK;
  }
  static_assert(MSC_MAX_TABLES == MSMZ_SUMCHECK_MAX_TABLES && MSC_MAX_DEGREE == MSMZ_SUMCHECK_MAX_DEGREE &&
                    MSC_MAX_TERMS == MSMZ_SUMCHECK_MAX_TERMS,
                "the limits of include/msmz.h are those of mle_kernels.h");

  // The operands of combine, recurrence, inverse and ntt.  Every source is a range of n records of a scalar set that does
  // not overlap the destination in part (entry i is read, then written: equal starts are in place).  The destination:
  // records [first_out, first_out + n) of `out_handle`, or, for out_handle == 0, a fresh set -- first_out must be 0 and
  // *out stays null, for the caller to allocate once every check has passed.
  struct Source {
    uint64_t handle, first;
    const uint32_t** p;
    uint64_t n = 0;   // records, where they differ from the destination's (a transform of zero-padded vectors); 0 = n
  };
  int resolve(const std::vector<Source>& srcs, uint64_t n, uint64_t first_out, uint64_t out_handle, uint32_t** out) {
    if (out_handle == 0 && first_out != 0) return MSMZ_ERR_ARG;
    for (const Source& s : srcs) {
      const uint64_t len = s.n ? s.n : n;
      if (s.handle == out_handle && ranges_clash(s.first, len, first_out, n)) return MSMZ_ERR_ARG;
      if (!(*s.p = handles_.range(s.handle, 1, s.first, len, 8))) return MSMZ_ERR_ARG;
    }
    if (out_handle && !(*out = handles_.range(out_handle, 1, first_out, n, 8))) return MSMZ_ERR_ARG;
    return MSMZ_OK;
  }

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
    return checked([&](uint32_t* d_err) {   // a scalar (either form) >= group order
      hipLaunchKernelGGL((k_import_scalars<Fr>), dim3((n + 255) / 256), dim3(256), 0, stream_, dst, v.ptr, v.stride,
                         (int)(v.width / 4), (uint32_t)n, (s.flags & MSMZ_SRC_MONTGOMERY) ? 1 : 0, d_err);
    });
  }

  // where the export kernel writes: the caller's device memory, or the packed staging records of a host destination
  struct ExportView {
    uint8_t* ptr = nullptr;
    uint64_t stride = 0;
    uint32_t width = 0;
    uint8_t* is_inf = nullptr;
  };

  // import_view mirrored (the descriptor has passed dst_check, which filled width and stride).  Device destination: the
  // pointers are vouched for -- the (n - 1) * stride + width bytes the kernel will write, n flag bytes -- and stream_
  // waits for an event recorded on the stream that last touches the destination (no host wait); the kernel writes in
  // place.  Host destination: the kernel writes packed records into stage_, the flag bytes behind them.
  int export_view(const msmz_dst& d, uint64_t n, ExportView* v) {
    if (d.flags & MSMZ_SRC_DEVICE) {
      const void* dp = nullptr;
      int st;
      if ((st = vouch(d.ptr, (n - 1) * v->stride + v->width, false, &dp))) return st;
      v->ptr = (uint8_t*)dp;
      if (d.is_inf) {
        if ((st = vouch(d.is_inf, n, false, &dp))) return st;
        v->is_inf = (uint8_t*)dp;
      }
      if (d.stream || (d.flags & MSMZ_SRC_DEFAULT_STREAM)) {
        MSMZ_HIP(hipEventRecord(import_ev_, (hipStream_t)d.stream));
        MSMZ_HIP(hipStreamWaitEvent(stream_, import_ev_, 0));
      }
      return MSMZ_OK;
    }
    if (int st = stage_.ensure((size_t)n * v->width + n)) return st;
    v->ptr = stage_.as<uint8_t>();
    v->stride = v->width;   // (the caller's stride is the host scatter's: export_run)
    if (d.is_inf) v->is_inf = v->ptr + (size_t)n * v->width;
    return MSMZ_OK;
  }

  // the export kernel over a view, then the way home of a host destination -- ONE device-to-host copy of the packed
  // records (and flag bytes), straight into a packed destination without flags, else into a host landing from which the
  // records are scattered at the caller's stride (bytes between records are not touched) -- behind the error-word fetch
  // of checked(): when it returns everything has been written.  After an error nothing is scattered.
  template <class Launch>
  int export_run(const msmz_dst& d, uint64_t n, const ExportView& v, Launch launch) {
    const bool host = !(d.flags & MSMZ_SRC_DEVICE);
    const size_t w = v.width, bytes = (size_t)n * w + (d.is_inf ? n : 0);
    const uint64_t stride = d.stride ? d.stride : w;
    const bool direct = host && stride == w && !d.is_inf;
    if (host && !direct) import_pack_.resize(bytes);
    hipError_t copied = hipSuccess;
    const int st = checked([&](uint32_t* d_err) {
      launch(d_err);
      if (host) copied = hipMemcpyAsync(direct ? d.ptr : (void*)import_pack_.data(), stage_.p, bytes, hipMemcpyDeviceToHost, stream_);
    });
    if (st) return st;
    if (copied != hipSuccess) return MSMZ_ERR_HIP;
    if (host && !direct) {
      uint8_t* out = (uint8_t*)d.ptr;
      if (stride == w) memcpy(out, import_pack_.data(), (size_t)n * w);
      else
        for (uint64_t i = 0; i < n; i++) memcpy(out + i * stride, import_pack_.data() + i * w, w);
      if (d.is_inf) memcpy(d.is_inf, import_pack_.data() + (size_t)n * w, n);
    }
    return MSMZ_OK;
  }

  // a table of powers (ntt_kernels.h) into device memory, queued on stream_: k_scalars_powers from the spec's base
  void ntt_fill(uint32_t* dst, const NttTableSpec& s) {
    FrPowTable table;
    fr_pow_table<Fr>(table, s.ratio);
    FrConst base;
    memcpy(base.w, s.base, 32);
    const uint64_t threads = (s.count + SPOW_RUN - 1) / SPOW_RUN;
    hipLaunchKernelGGL((k_scalars_powers<Fr>), dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream_, dst, base,
                       table, (uint32_t)s.count, GenMap{});
  }

  // *tables = the three twiddle tables of `plan` for the root w (the inverse root of an inverse transform), from the
  // cache or built now.  At most NTT_CACHE sets are kept, the oldest goes first; all are freed with the engine.
  static constexpr size_t NTT_CACHE = 8;
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
    c.mem.poison = &poison_;
    c.log_n = plan.log_n;
    memcpy(c.w, w, 32);
    if (int st = c.mem.ensure((size_t)ntt_twiddle_entries(plan) * 32)) return st;
    NttTableSpec spec[3];
    ntt_twiddle_specs<Fr>(plan, w, spec);
    uint32_t* at = c.mem.template as<uint32_t>();
    for (int k = 0; k < 3; k++) {
      ntt_fill(at, spec[k]);
      at += spec[k].count * 8;
    }
    if (hipGetLastError() != hipSuccess) return (void)hipStreamSynchronize(stream_), MSMZ_ERR_HIP;   // (c frees its memory)
    if (ntt_cache_.size() == NTT_CACHE) {
      // (the set that leaves may still be read by a transform in flight only if the stream has work: every entry point
      // returns with the stream drained, so it has none)
      ntt_cache_.pop_front();
    }
    ntt_cache_.push_back(std::move(c));
    *tables = ntt_cache_.back().mem.template as<const uint32_t>();
    return MSMZ_OK;
  }

  // The window table of a base (k_fixed_table) from the cache or built now.  The key: the base's canonical words (on the
  // Weierstrass curves all zero = the point at infinity), the window width and the number of windows.  At most
  // FIXED_CACHE tables are kept, the one unused longest goes first; all are freed with the engine.
  static constexpr size_t FIXED_CACHE = 4;
  struct FixedKey {
    uint32_t xy[RW];
    int c, K;
  };
  struct FixedTable {
    FixedKey key;
    DevBuf mem;
  };
  int fixed_table(const FixedKey& key, const FixedPlan& plan, const uint32_t** table) {
    for (auto it = fixed_cache_.begin(); it != fixed_cache_.end(); ++it) {
      if (it->key.c == key.c && it->key.K == key.K && !memcmp(it->key.xy, key.xy, sizeof(key.xy))) {
        FixedTable hit = std::move(*it);   // to the back: the table that leaves is the one unused longest
        fixed_cache_.erase(it);
        fixed_cache_.push_back(std::move(hit));
        *table = fixed_cache_.back().mem.template as<const uint32_t>();
        return MSMZ_OK;
      }
    }
    // the bases 2^(ck) B on the host (as ensure_gen_table does for G), the multiples on the device; a base that has
    // reached infinity (B at infinity or of small order) is the all-zero record
    std::vector<uint32_t> bases((size_t)plan.K * RW, 0);
    Fe<F> cx, cy, x, y;
    fe_unpack<F>(cx, key.xy);
    fe_unpack<F>(cy, key.xy + NW);
    fe_to_mont(x, cx);
    fe_to_mont(y, cy);
    typename P::Acc g, t;
    if (!TE && words_point_is_inf<F>(key.xy)) P::set_identity(g);
    else P::from_affine(g, x, y);
    for (int k = 0; k < plan.K; k++) {
      if (TE || !fe_is_zero_mod_p(P::denominator(g))) {
        Fe<F> inv;
        fe_inverse(inv, P::denominator(g));
        P::affine_from_inverse(x, y, g, inv);
        fe_store<F>(bases.data() + (size_t)k * RW, x);
        fe_store<F>(bases.data() + (size_t)k * RW + NW, y);
      }
      for (int j = 0; j < plan.c; j++) {
        P::dbl(t, g);
        g = t;
      }
    }
    FixedTable ft;
    ft.mem.poison = &poison_;
    ft.key = key;
    if (int st = ft.mem.ensure((size_t)plan.entries * RW * 4)) return st;
    if (int st = stage_.ensure(bases.size() * 4)) return st;
    MSMZ_HIP(hipMemcpyAsync(stage_.p, bases.data(), bases.size() * 4, hipMemcpyHostToDevice, stream_));
    hipLaunchKernelGGL((k_fixed_table<P>), dim3((uint32_t)((plan.entries + 255) / 256)), dim3(256), 0, stream_,
                       ft.mem.template as<uint32_t>(), stage_.as<const uint32_t>(), (uint32_t)plan.entries, plan.c);
    // (`bases` is pageable: the copy has left it when the call returns; the wait keeps the cache free of a table whose
    // build failed, and frees the entry that leaves with nothing in flight)
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess) return MSMZ_ERR_HIP;
    fixed_built_++;
    if (fixed_cache_.size() == FIXED_CACHE) fixed_cache_.pop_front();
    fixed_cache_.push_back(std::move(ft));
    *table = fixed_cache_.back().mem.template as<const uint32_t>();
    return MSMZ_OK;
  }

  int ensure_gen_table() {
    if (gen_table_.p) return MSMZ_OK;
    int st = gen_table_.ensure((size_t)GEN_WINDOWS * GEN_TABLE * RW * 4);
    if (st) return st;
    // bases 2^(13 k) * G computed on the host, multiples on the device
    uint32_t bases[GEN_WINDOWS * RW];
    Fe<F> gx, gy;
    fe_set_const<F>(gx, F::GX);
    fe_set_const<F>(gy, F::GY);
    typename P::Acc g, t;
    P::from_affine(g, gx, gy);
    for (int k = 0; k < GEN_WINDOWS; k++) {
      Fe<F> inv, x, y;
      fe_inverse(inv, P::denominator(g));
      P::affine_from_inverse(x, y, g, inv);
      fe_store<F>(bases + k * RW, x);
      fe_store<F>(bases + k * RW + NW, y);
      for (int j = 0; j < GEN_BITS; j++) {
        P::dbl(t, g);
        g = t;
      }
    }
    st = stage_.ensure(sizeof(bases));
    if (st) return st;
    MSMZ_HIP(hipMemcpyAsync(stage_.p, bases, sizeof(bases), hipMemcpyHostToDevice, stream_));
    hipLaunchKernelGGL((k_gen_table<P>), dim3((GEN_WINDOWS * GEN_TABLE + 127) / 128), dim3(128), 0, stream_,
                       gen_table_.as<uint32_t>(), stage_.as<uint32_t>());
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return MSMZ_OK;
  }

 protected:
  int device_;
  hipStream_t stream_ = nullptr;
  HandleTable handles_;
  Poison poison_;                      // msmz_test_poison: armed or not; every device buffer of the engine points here
  DevBuf stage_;                       // host data on its way to a kernel, results on their way back
  DevBuf meta_;                        // MsmMeta: the error word every kernel here reports through; the pipeline's totals
  PinnedOne<MsmMeta> h_meta_;          // ... and its pinned landing
  PinnedBuf h_res_;                    // pinned landing of a result record here, of the window results of an MSM

 private:
  hipEvent_t import_ev_ = nullptr;     // orders stream_ behind the stream that produces an imported device source (or last touches an export's destination)
  std::vector<uint8_t> import_pack_;   // host packing of a strided host source; the packed landing of a host export
  DevBuf gen_table_;
  std::deque<FixedTable> fixed_cache_;  // points_fixed_base: the window tables of the last FIXED_CACHE (base, c, K)
  uint64_t fixed_built_ = 0;           // ... the tables built so far, and the forced window width (0 = the planner's)
  int fixed_window_ = 0;
  DevBuf sdot_;                        // scalars_dot: its result record, then one partial sum per tile
  DevBuf mat_carry_;                   // matrix_mul: one carry record per tile
  DevBuf sscan_;                       // scalars_recurrence / _inverse: the result record, then aggregates and incoming values
  DevBuf ntt_scratch_;                 // scalars_ntt: one or two copies of the batch between the passes of a plan
  DevBuf ntt_coset_;                   // ... and the two-level powers of the coset shift of the call in progress
  std::deque<NttTwiddles> ntt_cache_;  // ... and the twiddle tables of the last NTT_CACHE (log_n, root) pairs
  DevBuf check_;                       // check_points: its result record, then one verdict byte per point
  PinnedBuf h_check_;                  // pinned landing of the result record and the verdict bytes behind it
  DevBuf lookup_slots_;                // scalars_lookup: the hash index, one table index or LK_EMPTY per slot
  DevBuf lookup_count_;                // ... one count per table entry
  DevBuf lookup_res_;                  // ... the error word and the three result words, then one position per column entry
  PinnedBuf h_lookup_;                 // pinned landing of the result words and the positions behind them
};

}  // namespace msmz

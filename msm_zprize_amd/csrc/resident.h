// The resident sets of one engine: point and scalar sets kept on one GPU under handles, and how they come and go --
// uploads, imports from host or device memory, generators, downloads and exports.  What every operation on them shares
// (the ONE HIP stream, the handle table, the result-record path) is SetsCore (sets_core.h), from which this derives; the
// operations that are not data movement are family stages it holds and forwards to (point_ops.h, scalar_ops.h, ntt_ops.h,
// matrix_ops.h, lookup_ops.h, expr_ops.h).  Every entry point returns with the stream drained.  Engine<Cfg> (engine.h) derives from
// this and adds the MSM pipeline, which runs on the same stream and reports through the same error word.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/msmz.h"
#include "kernels.h"
#include "gen_kernels.h"
#include "import_kernels.h"
#include "export_kernels.h"
#include "sets_core.h"
#include "point_ops.h"
#include "scalar_ops.h"
#include "ntt_ops.h"
#include "matrix_ops.h"
#include "lookup_ops.h"
#include "expr_ops.h"

namespace msmz {

template <class Cfg>
class ResidentSets : public SetsCore<Cfg> {
 protected:
  using Core = SetsCore<Cfg>;
  using typename Core::F;
  using typename Core::Fr;
  using typename Core::P;
  using Core::NW, Core::RW, Core::FE_BYTES, Core::TE, Core::PW_WORDS, Core::kBlock;
  using Core::device_, Core::stream_, Core::handles_, Core::poison_, Core::stage_;
  using Core::blocks_of, Core::drained, Core::checked, Core::copy_h2d, Core::fetch_points, Core::point_records;
  using Core::points_fit, Core::new_points, Core::new_scalars, Core::add_handle, Core::wait_after;

  explicit ResidentSets(int device) : Core(device), point_ops_(*this), scalar_ops_(*this), ntt_ops_(*this, scalar_ops_),
                                      matrix_ops_(*this), lookup_ops_(*this), expr_ops_(*this) {}

  // the core, then the event that orders stream_ behind a caller's (Engine::init goes on from here)
  int init_sets() {
    if (int st = Core::init_core()) return st;
    MSMZ_HIP(hipEventCreateWithFlags(&import_ev_, hipEventDisableTiming));
    gen_table_.poison = &poison_;   // (the scratch buffers: bound by Engine::init, through its each_scratch)
    return MSMZ_OK;
  }

  // f(buffer) for every scratch buffer of the operations here and of every stage: undefined at the start of every call
  // (DESIGN.md).  Not among them, because they hold what stays valid across calls: the records of the handles,
  // gen_table_ and the stages' caches -- those are bound to poison_ too, so a NEW one is filled when the engine is
  // armed, but never refilled.
  template <class Fn>
  void each_scratch(Fn f) {
    Core::each_scratch(f);
    point_ops_.each_scratch(f);
    scalar_ops_.each_scratch(f);
    ntt_ops_.each_scratch(f);
    matrix_ops_.each_scratch(f);
    lookup_ops_.each_scratch(f);
  }

 public:
  ~ResidentSets() override {   // (the stages' buffers free themselves after this, on this device; then the core's turn)
    (void)hipSetDevice(device_);
    if (import_ev_) (void)hipEventDestroy(import_ev_);
  }

  // ------------------------------------------------------------------------------------------ data
  int upload_points(const uint8_t* xy, const uint8_t* inf, uint64_t n, uint64_t* h, const GenMap* split = nullptr) override {
    if (!xy || !h || !points_fit(n)) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    int st = stage_.ensure(n * RW * 4 + n);
    if (st) return st;
    Handle hd;   // (every allocation comes before any copy is queued)
    if ((st = new_points(n, &hd))) return st;
    if ((st = copy_h2d(stage_.p, xy, (size_t)RW * 4, n, split))) return st;
    uint8_t* d_inf = nullptr;
    if (inf) {
      d_inf = stage_.template as<uint8_t>() + n * RW * 4;
      if ((st = copy_h2d(d_inf, inf, 1, n, split))) return st;
    }
    st = checked([&](uint32_t* d_err) {   // a coordinate >= p
      hipLaunchKernelGGL((k_points_to_resident<P>), blocks_of(n), dim3(kBlock), 0, stream_, hd.mem.as<uint32_t>(),
                         stage_.template as<uint32_t>(), d_inf, (uint32_t)n, hd.has_endo ? 1 : 0, d_err);
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
      hipLaunchKernelGGL((k_check_scalars<Fr>), blocks_of(n), dim3(kBlock), 0, stream_, d_err, hd.mem.as<const uint32_t>(),
                         (uint32_t)n);
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
    if (int st = drained()) return st;
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
        hipLaunchKernelGGL((k_import_points_compressed<P>), blocks_of(n), dim3(kBlock), 0, stream_, hd.mem.as<uint32_t>(),
                           v.ptr, v.stride, v.is_inf, (uint32_t)n, hd.has_endo ? 1 : 0,
                           (s.flags & MSMZ_SRC_SIGN_PARITY) ? 1 : 0, d_err);
      else
        hipLaunchKernelGGL((k_import_points<P>), blocks_of(n), dim3(kBlock), 0, stream_, hd.mem.as<uint32_t>(), v.ptr,
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
    // (the caller's streams, and blocking copies: nothing is queued on stream_ here)
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
    if ((st = drained())) return st;
    return add_handle(std::move(hd), h);
  }

  int random_scalars(uint64_t n, uint64_t seed, const GenMap& map, uint64_t* h) override {
    if (!h || n == 0) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    Handle hd;
    if (int st = new_scalars(n, &hd)) return st;
    hipLaunchKernelGGL((k_gen_scalars<Fr>), blocks_of(n), dim3(kBlock), 0, stream_, hd.mem.as<uint32_t>(), (uint32_t)n, seed,
                       map);
    if (int st = drained()) return st;
    return add_handle(std::move(hd), h);
  }

  int download_points(uint64_t hd, uint64_t first, uint64_t count, uint8_t* xy, uint8_t* inf) override {
    const uint32_t* recs = nullptr;
    if (!xy || point_records(hd, first, count, &recs)) return MSMZ_ERR_ARG;
    if (count == 0) return MSMZ_OK;
    if (int st = fetch_points(recs, count, xy)) return st;
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
    const uint32_t* recs = nullptr;
    if (!out || (flags & ~(uint32_t)MSMZ_SRC_SIGN_PARITY) || point_records(hd, first, count, &recs)) return MSMZ_ERR_ARG;
    if (count == 0) return MSMZ_OK;
    MSMZ_HIP(hipSetDevice(device_));
    if (int st = stage_.ensure(count * FE_BYTES + count)) return st;
    uint8_t* d_inf = stage_.template as<uint8_t>() + count * FE_BYTES;
    hipLaunchKernelGGL((k_points_compress<P>), blocks_of(count), dim3(kBlock), 0, stream_, stage_.template as<uint32_t>(), d_inf,
                       recs, (uint32_t)count, flags ? 1 : 0);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, stage_.p, count * FE_BYTES, hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess && inf) e = hipMemcpyAsync(inf, d_inf, count, hipMemcpyDeviceToHost, stream_);
    return wait_after(e);
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
      hipLaunchKernelGGL((k_export_scalars<Fr>), blocks_of(n), dim3(kBlock), 0, stream_, v.ptr, v.stride, (int)(v.width / 4), src,
                         (uint32_t)n, (d.flags & MSMZ_SRC_MONTGOMERY) ? 1 : 0, d_err);
    });
  }

  // msmz_export_points: records [first, first + n) of a point set under the range rules of download_points, as x || y
  // (canonical or Montgomery) or compressed, with the flag bytes if the destination has room for them.  One launch
  // (k_export_points); no kernel raises an error bit here, the fetch of the error word is the host wait.
  int export_points(uint64_t hd, uint64_t first, uint64_t n, const msmz_dst& d) override {
    ExportView v;
    if (int st = dst_check(&d, FE_BYTES, &v.width, &v.stride)) return st;
    const uint32_t* recs = nullptr;
    if (n == 0 || point_records(hd, first, n, &recs)) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    if (int st = export_view(d, n, &v)) return st;
    const int form = (int)(d.flags & (MSMZ_SRC_MONTGOMERY | MSMZ_SRC_COMPRESSED | MSMZ_SRC_SIGN_PARITY));
    return export_run(d, n, v, [&](uint32_t*) {
      hipLaunchKernelGGL((k_export_points<P>), blocks_of(n), dim3(kBlock), 0, stream_, v.ptr, v.stride, v.is_inf, recs,
                         (uint32_t)n, form);
    });
  }

  int free_handle(uint64_t hd) override {
    if (!handles_.known(hd)) return MSMZ_ERR_ARG;
    (void)hipSetDevice(device_);
    handles_.erase(hd);
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ the stages' methods
  int check_points(uint64_t h, uint64_t first, uint64_t count, uint32_t what, msmz_check_result* out, uint8_t* verdicts) override {
    return point_ops_.check_points(h, first, count, what, out, verdicts);
  }
  int points_mul(const msmz_mul& m, const msmz_mul_opts& o, uint64_t n, uint64_t* h) override { return point_ops_.points_mul(m, o, n, h); }
  int points_fixed_base(const msmz_fixed_base& f, uint64_t n, uint64_t* h) override { return point_ops_.points_fixed_base(f, n, h); }
  int test_set_fixed_base_window(int c) override { return point_ops_.test_set_fixed_base_window(c); }
  uint64_t test_fixed_base_tables() override { return point_ops_.test_fixed_base_tables(); }
  uint64_t test_ntt_tables() override { return ntt_ops_.test_ntt_tables(); }
  int scalars_combine(const msmz_scalar_term& x, const msmz_scalar_term* y, uint64_t n, uint64_t first_out, uint64_t* out) override {
    return scalar_ops_.scalars_combine(x, y, n, first_out, out);
  }
  int scalars_dot(uint64_t xh, uint64_t first_x, uint64_t yh, uint64_t first_y, uint64_t n, uint8_t* out) override {
    return scalar_ops_.scalars_dot(xh, first_x, yh, first_y, n, out);
  }
  int scalars_powers(const uint8_t* base, const uint8_t* ratio, uint64_t n, const GenMap& map, uint64_t* h) override {
    return scalar_ops_.scalars_powers(base, ratio, n, map, h);
  }
  int scalars_recurrence(const msmz_scalar_rec& r, uint64_t n, uint64_t first_out, uint64_t* out, uint8_t* last) override {
    return scalar_ops_.scalars_recurrence(r, n, first_out, out, last);
  }
  int scalars_inverse(uint64_t h, uint64_t first, uint64_t n, uint64_t first_out, uint64_t* out, uint64_t* n_zero) override {
    return scalar_ops_.scalars_inverse(h, first, n, first_out, out, n_zero);
  }
  int scalars_eq_table(const uint8_t* point, uint32_t n_vars, const uint8_t* scale, uint64_t* h) override {
    return scalar_ops_.scalars_eq_table(point, n_vars, scale, h);
  }
  int scalars_mle_eval(uint64_t xh, uint64_t first, uint32_t n_vars, const uint8_t* point, uint8_t* out) override {
    return scalar_ops_.scalars_mle_eval(xh, first, n_vars, point, out);
  }
  int scalars_mle_bind(const msmz_mle_bind& b, uint64_t first_out, uint64_t* out) override { return scalar_ops_.scalars_mle_bind(b, first_out, out); }
  int scalars_sumcheck_round(const msmz_sumcheck& s, uint32_t* degree, uint8_t* evals) override {
    return scalar_ops_.scalars_sumcheck_round(s, degree, evals);
  }
  int scalars_sumcheck_step(const msmz_sumcheck_step& s, uint32_t* degree, uint8_t* evals) override {
    return scalar_ops_.scalars_sumcheck_step(s, degree, evals);
  }
  int scalars_dot_many(const msmz_dot_many& d, uint8_t* out_le32, uint64_t first_out, uint64_t* out) override {
    return scalar_ops_.scalars_dot_many(d, out_le32, first_out, out);
  }
  int test_set_dot_many_groups(uint32_t g) override { return scalar_ops_.test_set_dot_many_groups(g); }
  int scalars_ntt(const msmz_ntt& t, uint64_t first_out, uint64_t* out) override { return ntt_ops_.scalars_ntt(t, first_out, out); }
  int matrix_create(const msmz_sparse& s, uint64_t* h) override { return matrix_ops_.matrix_create(s, h); }
  int matrix_info(uint64_t h, uint32_t* n_rows, uint32_t* n_cols, uint64_t* nnz, uint32_t* flags) override {
    return matrix_ops_.matrix_info(h, n_rows, n_cols, nnz, flags);
  }
  int matrix_mul(const msmz_matvec& v, uint64_t first_out, uint64_t* out) override { return matrix_ops_.matrix_mul(v, first_out, out); }
  int scalars_lookup(const msmz_lookup& l, uint64_t first_out, uint64_t* out, msmz_lookup_result* res) override {
    return lookup_ops_.scalars_lookup(l, first_out, out, res);
  }
  int scalars_expr(const msmz_expr& e, uint64_t first_out, uint64_t* out) override {
    return expr_ops_.scalars_expr(e, first_out, out);
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

  // The device branch of a view, import or export (msmz_dst mirrors msmz_src: iengine.h): the pointers are vouched for
  // -- the (n - 1) * stride + width bytes a kernel will touch, n flag bytes -- and stream_ waits for an event recorded on
  // the caller's stream (no host wait).  *dp, *di: the device-side addresses (di stays as it is without flag bytes).
  template <class Desc>
  int device_view(const Desc& s, uint64_t n, uint64_t stride, uint32_t width, const void** dp, const void** di) {
    if (int st = vouch(s.ptr, (n - 1) * stride + width, false, dp)) return st;
    if (s.is_inf)
      if (int st = vouch(s.is_inf, n, false, di)) return st;
    if (s.stream || (s.flags & MSMZ_SRC_DEFAULT_STREAM)) {   // (only a wait is queued: nothing to drain if it fails)
      MSMZ_HIP(hipEventRecord(import_ev_, (hipStream_t)s.stream));
      MSMZ_HIP(hipStreamWaitEvent(stream_, import_ev_, 0));
    }
    return MSMZ_OK;
  }

  // Checks the source and makes it readable for the import kernel, in stream order.  Device source: device_view.  Host
  // source: `width` bytes per record go to stage_ (a strided source is packed on the host first; `split`: this engine's
  // blocks of a packed source), the flag bytes behind them.
  int import_view(const msmz_src& s, int point_fe_bytes, uint64_t n, const GenMap* split, ImportView* v) {
    if (int st = src_check(&s, point_fe_bytes, &v->width, &v->stride)) return st;
    const uint8_t* p = (const uint8_t*)s.ptr;
    if (s.flags & MSMZ_SRC_DEVICE) {
      if (split) return MSMZ_ERR_ARG;   // (a multi-device context hands its engines host copies)
      const void *dp = nullptr, *di = nullptr;
      if (int st = device_view(s, n, v->stride, v->width, &dp, &di)) return st;
      v->ptr = (const uint8_t*)dp;
      v->is_inf = (const uint8_t*)di;
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
    // (copy_h2d drains the stream if it fails: when the call returns the source is no longer read)
    if ((st = copy_h2d(stage_.p, p, w, n, split))) return st;
    if (s.is_inf) {
      uint8_t* d_inf = stage_.template as<uint8_t>() + (size_t)n * w;
      if ((st = copy_h2d(d_inf, s.is_inf, 1, n, split))) return st;
      v->is_inf = d_inf;
    }
    v->ptr = stage_.template as<const uint8_t>();
    v->stride = w;
    return MSMZ_OK;
  }

  // the conversion kernel over a view, then the error-word fetch: when it returns the source has been read
  int import_scalars_to(uint32_t* dst, const msmz_src& s, const ImportView& v, uint64_t n) {
    return checked([&](uint32_t* d_err) {   // a scalar (either form) >= group order
      hipLaunchKernelGGL((k_import_scalars<Fr>), blocks_of(n), dim3(kBlock), 0, stream_, dst, v.ptr, v.stride,
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

  // import_view mirrored (the descriptor has passed dst_check, which filled width and stride).  Device destination:
  // device_view, on the stream that last touches the destination; the kernel writes in place.  Host destination: the
  // kernel writes packed records into stage_, the flag bytes behind them.
  int export_view(const msmz_dst& d, uint64_t n, ExportView* v) {
    if (d.flags & MSMZ_SRC_DEVICE) {
      const void *dp = nullptr, *di = nullptr;
      if (int st = device_view(d, n, v->stride, v->width, &dp, &di)) return st;
      v->ptr = (uint8_t*)dp;
      v->is_inf = (uint8_t*)di;
      return MSMZ_OK;
    }
    if (int st = stage_.ensure((size_t)n * v->width + n)) return st;
    v->ptr = stage_.template as<uint8_t>();
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

  // the generator's window table, built once: the bases 2^(GEN_BITS k) G on the host (PointOps::window_bases), the
  // multiples on the device
  int ensure_gen_table() {
    if (gen_table_.p) return MSMZ_OK;
    uint32_t bases[GEN_WINDOWS * RW];
    int st = stage_.ensure(sizeof(bases));
    if (st || (st = gen_table_.ensure((size_t)GEN_WINDOWS * GEN_TABLE * RW * 4))) return st;
    Fe<F> gx, gy;
    fe_set_const<F>(gx, F::GX);
    fe_set_const<F>(gy, F::GY);
    typename P::Acc g;
    P::from_affine(g, gx, gy);
    PointOps<Cfg>::window_bases(g, GEN_WINDOWS, GEN_BITS, bases);
    hipError_t e = hipMemcpyAsync(stage_.p, bases, sizeof(bases), hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) {
      hipLaunchKernelGGL((k_gen_table<P>), dim3((GEN_WINDOWS * GEN_TABLE + 127) / 128), dim3(128), 0, stream_,
                         gen_table_.as<uint32_t>(), stage_.template as<uint32_t>());
      e = hipGetLastError();
    }
    if ((st = wait_after(e))) gen_table_.release();   // (no table: the next call builds it again)
    return st;
  }

  PointOps<Cfg> point_ops_;
  ScalarOps<Cfg> scalar_ops_;
  NttOps<Cfg> ntt_ops_;
  MatrixOps<Cfg> matrix_ops_;
  LookupOps<Cfg> lookup_ops_;
  ExprOps<Cfg> expr_ops_;   // (owns no buffer: nothing for each_scratch)
  hipEvent_t import_ev_ = nullptr;     // orders stream_ behind the stream that produces an imported device source (or last touches an export's destination)
  std::vector<uint8_t> import_pack_;   // host packing of a strided host source; the packed landing of a host export
  DevBuf gen_table_;
};

}  // namespace msmz

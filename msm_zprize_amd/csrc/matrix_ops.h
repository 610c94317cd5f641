// Sparse matrices against resident scalar sets, as one stage: create, info, y = M x and y = M^T x.  MatrixOps owns
// mat_carry_ and reaches the engine through the SetsCore it is built with (sets_core.h); the matrices themselves are
// handles of kind 2 (store.h).  ResidentSets (resident.h) forwards the IEngine methods here.
#pragma once
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "../../include/msmz.h"
#include "matrix_kernels.h"
#include "sets_core.h"

namespace msmz {

template <class Cfg>
class MatrixOps {
  using Core = SetsCore<Cfg>;
  using Fr = typename Cfg::Fr;

 public:
  explicit MatrixOps(Core& core) : core_(core) {}

  // f(buffer) for every device buffer of the stage: all scratch, undefined at the start of every call
  template <class Fn>
  void each_scratch(Fn f) {
    f(mat_carry_);
  }

  // msmz_matrix_create: the host sorts the triples into the forms asked for (mat_sort_form), the device keeps them and
  // k_matrix_pack brings the values out of the caller's scalar set, in sorted order and in Montgomery form.  The error
  // word (a value >= q) comes back behind the ONE host wait, which also ends the copies out of the host vectors.
  int matrix_create(const msmz_sparse& s, uint64_t* h) {
    if (!h || !s.row || !s.col || s.nnz == 0 || s.nnz >> 32 || s.n_rows == 0 || s.n_cols == 0 ||
        (s.flags & ~(uint32_t)(MSMZ_MAT_ROWS | MSMZ_MAT_COLS)))
      return MSMZ_ERR_ARG;
    const uint64_t nnz = s.nnz;
    const uint32_t* vals = nullptr;
    if (s.val_handle ? !(vals = core_.handles_.range(s.val_handle, 1, s.val_first, nnz, 8)) : s.val_first != 0) return MSMZ_ERR_ARG;
    if (mat_first_bad_index(s.row, s.col, nnz, s.n_rows, s.n_cols) != nnz) return MSMZ_ERR_ARG;
    const uint32_t flags = s.flags ? s.flags : (uint32_t)MSMZ_MAT_ROWS;
    MSMZ_HIP(hipSetDevice(core_.device_));
    hipStream_t stream = core_.stream_;
    DevBuf& stage = core_.stage_;
    Handle hd;
    hd.form[0].poison = hd.form[1].poison = &core_.poison_;
    hd.kind = 2, hd.n = nnz, hd.n_rows = s.n_rows, hd.n_cols = s.n_cols, hd.mat_flags = flags, hd.has_vals = vals != nullptr;
    std::vector<uint32_t> host[2];   // per form: seg, gidx, perm in a row; alive until the wait below
    const size_t val_off = mat_val_offset(nnz);
    if (int st = stage.ensure(2 * nnz * 4)) return st;
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
      e = hipMemcpyAsync(hd.form[f].p, seg, 2 * nnz * 4, hipMemcpyHostToDevice, stream);
      if (e == hipSuccess && vals)
        e = hipMemcpyAsync(stage.template as<uint32_t>() + f * nnz, seg + 2 * nnz, nnz * 4, hipMemcpyHostToDevice, stream);
    }
    if (e != hipSuccess) return core_.wait_after(e);
    const int st = core_.checked([&](uint32_t* d_err) {   // a value >= group order
      for (int f = 0; f < 2 && vals; f++) {
        if (!hd.form[f].p) continue;
        hipLaunchKernelGGL((k_matrix_pack<Fr>), Core::blocks_of(nnz), dim3(Core::kBlock), 0, stream,
                           (uint32_t*)(hd.form[f].template as<uint8_t>() + val_off), vals,
                           (const uint32_t*)(stage.template as<uint32_t>() + f * nnz), (uint32_t)nnz, d_err);
      }
    });
    return st ? st : core_.add_handle(std::move(hd), h);
  }

  int matrix_info(uint64_t h, uint32_t* n_rows, uint32_t* n_cols, uint64_t* nnz, uint32_t* flags) {
    const Handle* m = core_.handles_.get(h, 2);
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
  int matrix_mul(const msmz_matvec& v, uint64_t first_out, uint64_t* out_handle) {
    if (!out_handle || (v.flags & ~(uint32_t)MSMZ_MATVEC_TRANSPOSE)) return MSMZ_ERR_ARG;
    const Handle* m = core_.handles_.get(v.matrix, 2);
    const int f = (v.flags & MSMZ_MATVEC_TRANSPOSE) ? 1 : 0;
    if (!m || !m->form[f].p) return MSMZ_ERR_ARG;
    const uint64_t n_in = f ? m->n_rows : m->n_cols, n_out = f ? m->n_cols : m->n_rows, nnz = m->n;
    if (*out_handle && *out_handle == v.x_handle && ranges_meet(v.x_first, n_in, first_out, n_out)) return MSMZ_ERR_ARG;
    const uint32_t* X = nullptr;
    uint32_t* out = nullptr;
    if (int st = core_.resolve({{v.x_handle, v.x_first, &X, n_in}}, n_out, first_out, *out_handle, &out)) return st;
    MSMZ_HIP(hipSetDevice(core_.device_));
    hipStream_t stream = core_.stream_;
    const uint32_t tiles = (uint32_t)((nnz + MAT_TILE - 1) / MAT_TILE);
    if (int st = mat_carry_.ensure((size_t)tiles * MAT_CARRY_WORDS * 4)) return st;
    Handle hd;
    if (int st = core_.fresh_out(n_out, &hd, &out)) return st;
    const uint8_t* base = m->form[f].template as<const uint8_t>();
    const MatView view = {(const uint32_t*)base + nnz, (const uint32_t*)base,
                          m->has_vals ? (const uint32_t*)(base + mat_val_offset(nnz)) : nullptr};
    const int st = core_.checked([&](uint32_t* d_err) {   // an entry of x >= group order
      if (hipMemsetAsync(out, 0, n_out * 32, stream) != hipSuccess) return;   // (fetch_error reports it)
      hipLaunchKernelGGL((k_matrix_mul<Fr>), dim3(tiles), dim3(MAT_THREADS), 0, stream, out, view, X, (uint32_t)nnz,
                         mat_carry_.as<uint32_t>(), d_err);
      hipLaunchKernelGGL((k_matrix_fold<Fr>), dim3(1), dim3(MAT_THREADS), 0, stream, out,
                         (const uint32_t*)mat_carry_.as<uint32_t>(), tiles);
    });
    return st || !hd.mem.p ? st : core_.add_handle(std::move(hd), out_handle);
  }

 private:
  Core& core_;
  DevBuf mat_carry_;   // matrix_mul: one carry record per tile
};

}  // namespace msmz

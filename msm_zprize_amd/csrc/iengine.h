// What a context is to the C ABI (msmz.hip): the interface one engine (Engine, engine.h, over resident.h and sets_core.h) and
// the multi-device context (MultiEngine, multi.h) both implement, with the two small things its signatures need -- how a
// device-side generator maps local to global indices, and the checks of an import source that need no device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/msmz.h"

namespace msmz {

class ITestHooks;   // the stage-level test hooks of one engine (test_hooks.h)

constexpr int MULTI_BLOCK_SHIFT = 16;

// how device-side generators map a local index to the global (seeded) index
struct GenMap {
  uint32_t nshards = 1, shard = 0;
  int blk_shift = MULTI_BLOCK_SHIFT;
};

// The checks of an import source (msmz_src, include/msmz.h) that need no device: flags, pointer alignment, width and
// stride.  points: fe_bytes of the curve, 0 for a scalar source.  *width / *stride: the record's bytes and the bytes
// from one record to the next, defaults resolved.  What the pointer points at is the engine's to ask (ResidentSets::vouch).
// (msmz_dst is msmz_src read in the other direction -- the same fields at the same offsets, asserted here -- so one body
// checks both: src_check and dst_check below)
static_assert(sizeof(msmz_dst) == sizeof(msmz_src) && offsetof(msmz_dst, ptr) == offsetof(msmz_src, ptr) &&
                  offsetof(msmz_dst, stride) == offsetof(msmz_src, stride) && offsetof(msmz_dst, width) == offsetof(msmz_src, width) &&
                  offsetof(msmz_dst, flags) == offsetof(msmz_src, flags) && offsetof(msmz_dst, stream) == offsetof(msmz_src, stream) &&
                  offsetof(msmz_dst, is_inf) == offsetof(msmz_src, is_inf),
              "msmz_dst mirrors msmz_src");
template <class Desc>
static inline int desc_check(const Desc* s, int point_fe_bytes, uint32_t* width, uint64_t* stride) {
  if (!s || !s->ptr) return MSMZ_ERR_ARG;
  const uint32_t point_flags = point_fe_bytes ? MSMZ_SRC_COMPRESSED | MSMZ_SRC_SIGN_PARITY : 0u;   // (refused on scalars)
  if (s->flags & ~(uint32_t)(MSMZ_SRC_DEVICE | MSMZ_SRC_MONTGOMERY | MSMZ_SRC_DEFAULT_STREAM | point_flags)) return MSMZ_ERR_ARG;
  const bool compressed = (s->flags & MSMZ_SRC_COMPRESSED) != 0;
  if (compressed ? (s->flags & MSMZ_SRC_MONTGOMERY) != 0 : (s->flags & MSMZ_SRC_SIGN_PARITY) != 0) return MSMZ_ERR_ARG;
  const bool dev = (s->flags & MSMZ_SRC_DEVICE) != 0;
  if (!dev && (s->stream || (s->flags & MSMZ_SRC_DEFAULT_STREAM))) return MSMZ_ERR_ARG;
  if (s->stream && (s->flags & MSMZ_SRC_DEFAULT_STREAM)) return MSMZ_ERR_ARG;
  uint32_t w = s->width;
  if (point_fe_bytes) {
    const uint32_t rec = (compressed ? 1u : 2u) * (uint32_t)point_fe_bytes;   // one coordinate + sign bit, or x || y
    if (w != 0 && w != rec) return MSMZ_ERR_ARG;
    w = rec;
  } else {
    if (w < 4 || w > 32 || (w & 3u) || s->is_inf) return MSMZ_ERR_ARG;
    if ((s->flags & MSMZ_SRC_MONTGOMERY) && w != 32) return MSMZ_ERR_ARG;
  }
  if (s->stride != 0 && (s->stride < w || (s->stride & 3u) || (s->stride >> 24))) return MSMZ_ERR_ARG;   // (n * stride cannot wrap)
  if ((uintptr_t)s->ptr & 3u) return MSMZ_ERR_ARG;
  *width = w;
  *stride = s->stride ? s->stride : w;
  return MSMZ_OK;
}
static inline int src_check(const msmz_src* s, int point_fe_bytes, uint32_t* width, uint64_t* stride) {
  return desc_check(s, point_fe_bytes, width, stride);
}
// The same checks of an export destination (msmz_dst): the descriptor faults are those of a source.
static inline int dst_check(const msmz_dst* d, int point_fe_bytes, uint32_t* width, uint64_t* stride) {
  return desc_check(d, point_fe_bytes, width, stride);
}

class IEngine {
 public:
  virtual ~IEngine() {}
  // imports (msmz_import_*): `split` as for uploads, and then the source is packed host memory
  virtual int import_scalars(const msmz_src& s, uint64_t n, uint64_t* h, const GenMap* split = nullptr) = 0;
  virtual int import_scalars_into(uint64_t h, uint64_t first, const msmz_src& s, uint64_t n) = 0;
  virtual int alloc_scalars(uint64_t, uint64_t*) { return MSMZ_ERR_UNSUPPORTED; }   // (_into's target: single-device contexts)
  virtual int import_points(const msmz_src& s, uint64_t n, uint64_t* h, const GenMap* split = nullptr) = 0;
  // packed host copy of the n records (and flag bytes, if the source has them) of a source in either memory space
  virtual int gather_src(const msmz_src& s, int point_fe_bytes, uint64_t n, std::vector<uint8_t>* recs,
                         std::vector<uint8_t>* flags) = 0;
  // `split` (uploads and host-scalar MSMs): the engine is one shard of a multi-device context and `n` counts its LOCAL
  // records; the host buffer is the caller's whole array, from which the engine copies its own blocks (SetsCore::copy_h2d)
  virtual int upload_points(const uint8_t* xy, const uint8_t* inf, uint64_t n, uint64_t* h, const GenMap* split = nullptr) = 0;
  virtual int upload_scalars(const uint8_t* s, uint64_t n, uint64_t* h, const GenMap* split = nullptr) = 0;
  virtual int random_points(uint64_t n, uint64_t seed, const GenMap& map, uint64_t* h) = 0;
  virtual int random_scalars(uint64_t n, uint64_t seed, const GenMap& map, uint64_t* h) = 0;
  virtual int download_points(uint64_t h, uint64_t first, uint64_t count, uint8_t* xy, uint8_t* inf) = 0;
  // msmz_download_points_compressed: count records of fe_bytes, flags = 0 or MSMZ_SRC_SIGN_PARITY
  virtual int download_points_compressed(uint64_t h, uint64_t first, uint64_t count, uint8_t* out, uint8_t* inf,
                                         uint32_t flags) = 0;
  virtual int download_scalars(uint64_t h, uint64_t first, uint64_t count, uint8_t* s) = 0;
  // msmz_export_scalars / msmz_export_points: entries [first, first + n) into the caller's memory, host or device, in
  // the form the destination names (the defaults: an engine that has no exports)
  virtual int export_scalars(uint64_t, uint64_t, uint64_t, const msmz_dst&) { return MSMZ_ERR_UNSUPPORTED; }
  virtual int export_points(uint64_t, uint64_t, uint64_t, const msmz_dst&) { return MSMZ_ERR_UNSUPPORTED; }
  virtual int free_handle(uint64_t h) = 0;
  // `batch` MSMs over the same first n points (msmz_msm_batch): vector k = resident entries [k n, (k + 1) n), or host
  // buffer entries [k host_stride, k host_stride + n) (host_stride 0 = n); out: batch results, out_inf: batch flags
  virtual int msm_batch(uint64_t ph, const uint8_t* host_scalars, uint64_t sh, uint64_t n, uint32_t batch,
                        const msmz_opts* o, uint8_t* out, int* out_inf, msmz_log* log, const GenMap* split = nullptr,
                        uint64_t host_stride = 0) = 0;
  // msmz_msm_segments: problem k = scalars [first_s, first_s + n) of `sh` times base points [first_p, first_p + n) of `ph`
  virtual int msm_segments(uint64_t ph, uint64_t sh, const msmz_segment* segs, uint32_t n_segs, const msmz_opts* o,
                           uint8_t* out, int* out_inf, msmz_log* log) = 0;
  // precomputed point sets (msmz_precompute_points): the parameters a set of n points is built with, then the copies
  // (sbits: the scalar bit bound of opts->reserved[1] as the planner normalizes it, 0 = none)
  virtual int precompute_params(uint64_t n, const msmz_opts* o, uint32_t factor, int* c, int* glv, uint32_t* copies,
                                int* K, int* sbits) const = 0;
  virtual int precompute_points(uint64_t ph, uint64_t n, int c, int glv, uint32_t copies, int sbits, uint64_t* h) = 0;
  virtual int precomputed_info(uint64_t h, int32_t* c, int32_t* glv, uint32_t* factor, uint32_t* K, uint64_t* records,
                               int32_t* sbits) = 0;
  // msmz_check_points over base points [first, first + count) of a plain point handle
  virtual int check_points(uint64_t h, uint64_t first, uint64_t count, uint32_t what, msmz_check_result* out,
                           uint8_t* verdicts) = 0;
  // msmz_points_mul / msmz_points_mul_opts: a new plain point handle, record i = [s_i] P_i (+ Q_i); o: all zero = none
  virtual int points_mul(const msmz_mul& m, const msmz_mul_opts& o, uint64_t n, uint64_t* h) = 0;
  // msmz_points_fixed_base: a new plain point handle, record i = [s_i] B (msmz.hip has checked flags and scalar_bits)
  virtual int points_fixed_base(const msmz_fixed_base&, uint64_t, uint64_t*) { return MSMZ_ERR_UNSUPPORTED; }
  // msmz_scalars_combine / _dot / _powers: arithmetic mod q over resident scalar sets (scalar_kernels.h); `map` as for
  // random_scalars
  virtual int scalars_combine(const msmz_scalar_term& x, const msmz_scalar_term* y, uint64_t n, uint64_t first_out,
                              uint64_t* out_handle) = 0;
  virtual int scalars_dot(uint64_t xh, uint64_t first_x, uint64_t yh, uint64_t first_y, uint64_t n, uint8_t* out) = 0;
  virtual int scalars_powers(const uint8_t* base, const uint8_t* ratio, uint64_t n, const GenMap& map, uint64_t* h) = 0;
  // msmz_scalars_recurrence / _inverse: a scan of affine maps and Montgomery's trick (scan_kernels.h)
  virtual int scalars_recurrence(const msmz_scalar_rec& r, uint64_t n, uint64_t first_out, uint64_t* out_handle,
                                 uint8_t* last) = 0;
  virtual int scalars_inverse(uint64_t h, uint64_t first, uint64_t n, uint64_t first_out, uint64_t* out_handle,
                              uint64_t* n_zero) = 0;
  // msmz_scalars_ntt: number-theoretic transforms over ranges of a scalar set (ntt_kernels.h)
  virtual int scalars_ntt(const msmz_ntt& t, uint64_t first_out, uint64_t* out_handle) = 0;
  // msmz_scalars_eq_table / _mle_eval / _mle_bind / _sumcheck_round / _sumcheck_step: multilinear polynomials over ranges
  // of a scalar set (mle_kernels.h).  The defaults: a context that has none -- a multi-device one, where the two halves of every pair
  // live in different blocks of 2^16 entries.
  virtual int scalars_eq_table(const uint8_t*, uint32_t, const uint8_t*, uint64_t*) { return MSMZ_ERR_UNSUPPORTED; }
  virtual int scalars_mle_eval(uint64_t, uint64_t, uint32_t, const uint8_t*, uint8_t*) { return MSMZ_ERR_UNSUPPORTED; }
  virtual int scalars_mle_bind(const msmz_mle_bind&, uint64_t, uint64_t*) { return MSMZ_ERR_UNSUPPORTED; }
  virtual int scalars_sumcheck_round(const msmz_sumcheck&, uint32_t*, uint8_t*) { return MSMZ_ERR_UNSUPPORTED; }
  virtual int scalars_sumcheck_step(const msmz_sumcheck_step&, uint32_t*, uint8_t*) { return MSMZ_ERR_UNSUPPORTED; }
  // msmz_matrix_create / _matrix_info / _matrix_mul: sparse matrices against ranges of a scalar set (matrix_kernels.h).
  // The defaults: a multi-device context has none -- a gather reads across every block of 2^16 entries.
  virtual int matrix_create(const msmz_sparse&, uint64_t*) { return MSMZ_ERR_UNSUPPORTED; }
  virtual int matrix_info(uint64_t, uint32_t*, uint32_t*, uint64_t*, uint32_t*) { return MSMZ_ERR_UNSUPPORTED; }
  virtual int matrix_mul(const msmz_matvec&, uint64_t, uint64_t*) { return MSMZ_ERR_UNSUPPORTED; }
  // msmz_scalars_lookup: the multiplicities of a column in a table (lookup_kernels.h).  The default: a multi-device
  // context has none -- a probe reads across every block of 2^16 entries.
  virtual int scalars_lookup(const msmz_lookup&, uint64_t, uint64_t*, msmz_lookup_result*) { return MSMZ_ERR_UNSUPPORTED; }
  // msmz_scalars_expr: a sum of products of rotated columns, entry by entry (expr_kernels.h).  The default: a context
  // that has none.
  virtual int scalars_expr(const msmz_expr&, uint64_t, uint64_t*) { return MSMZ_ERR_UNSUPPORTED; }
  // msmz_scalars_dot_many: every inner product of a family of row vectors with a family of column vectors
  // (dot_kernels.h).  The default: a context that has none -- a multi-device one.
  virtual int scalars_dot_many(const msmz_dot_many&, uint8_t*, uint64_t, uint64_t*) { return MSMZ_ERR_UNSUPPORTED; }
  // tests (include/msmz_test.h); the stage-level hooks are one engine's (a multi-device context: its first engine's)
  virtual int test_set_glv_bits(int) { return MSMZ_ERR_UNSUPPORTED; }
  virtual int test_retries() { return 0; }
  virtual int test_set_limits(uint64_t, uint64_t) { return MSMZ_ERR_UNSUPPORTED; }
  virtual void test_passes(uint64_t* range_passes, uint64_t* sub_batches) {
    if (range_passes) *range_passes = 0;
    if (sub_batches) *sub_batches = 0;
  }
  // msmz_test_set_fixed_base_window / msmz_test_fixed_base_tables: the forced window width, the tables built so far
  virtual int test_set_fixed_base_window(int) { return MSMZ_ERR_UNSUPPORTED; }
  virtual uint64_t test_fixed_base_tables() { return 0; }
  // msmz_test_set_dot_many_groups: the most workgroups along n of msmz_scalars_dot_many (0 = the built-in value)
  virtual int test_set_dot_many_groups(uint32_t) { return MSMZ_ERR_UNSUPPORTED; }
  // msmz_test_ntt_tables: the twiddle sets built so far
  virtual uint64_t test_ntt_tables() { return 0; }
  // msmz_test_poison: fill every scratch buffer with `pattern` and arm the allocations to come (-1: disarm)
  virtual int test_poison(int, uint64_t*, uint64_t*) { return MSMZ_ERR_UNSUPPORTED; }
  // msmz_test_scratch: the scratch buffers of engine `engine` of the context that hold memory, and their bytes
  virtual int test_scratch(int, uint64_t*, uint64_t*) { return MSMZ_ERR_UNSUPPORTED; }
  virtual ITestHooks* test_hooks() = 0;
};

}  // namespace msmz

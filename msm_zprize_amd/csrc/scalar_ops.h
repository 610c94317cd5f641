// The arithmetic mod q over resident scalar sets, as one stage: linear combinations, inner products, powers, recurrences,
// batch inversion, and the multilinear calls (eq table, evaluation, binding, sumcheck round and step), which share the
// inner product's record and fold (sdot_, k_scalars_dot_fold).  ScalarOps owns sdot_ and sscan_ and reaches the engine
// through the SetsCore it is built with (sets_core.h); ResidentSets (resident.h) forwards the IEngine methods here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/msmz.h"
#include "scalar_kernels.h"
#include "dot_kernels.h"
#include "mle_kernels.h"
#include "sets_core.h"

namespace msmz {

template <class Cfg>
class ScalarOps {
  using Core = SetsCore<Cfg>;
  using Fr = typename Cfg::Fr;
  using Source = typename Core::Source;
  static constexpr uint32_t kBlock = Core::kBlock;

 public:
  explicit ScalarOps(Core& core) : core_(core) {}

  // f(buffer) for every device buffer of the stage: all scratch, undefined at the start of every call
  template <class Fn>
  void each_scratch(Fn f) {
    f(sdot_), f(sscan_);
  }

  // msmz_scalars_combine: out_i = x.c_i x.v_i (+ y.c_i y.v_i) into a new scalar handle or over a range of an existing
  // one.  One launch; the error word (a resident record >= q) comes back behind the ONE host wait.
  int scalars_combine(const msmz_scalar_term& x, const msmz_scalar_term* y, uint64_t n, uint64_t first_out, uint64_t* out_handle) {
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
    if (int st = core_.resolve(srcs, n, first_out, *out_handle, &out)) return st;
    for (int k = 0; k < 2; k++) {
      if (!in[k] || in[k]->coeff_handle) continue;
      if (!in[k]->coeff) t[k].unit = 1;
      else if (int st = Core::read_fr(in[k]->coeff, t[k].k.w, true)) return st;
    }
    MSMZ_HIP(hipSetDevice(core_.device_));
    Handle hd;
    if (int st = core_.fresh_out(n, &hd, &out)) return st;
    const int st = core_.checked([&](uint32_t* d_err) {   // a resident record >= group order
      hipLaunchKernelGGL((k_scalars_combine<Fr>), Core::blocks_of(n), dim3(kBlock), 0, core_.stream_, out, t[0], t[1],
                         (uint32_t)n, d_err);
    });
    return st || !hd.mem.p ? st : core_.add_handle(std::move(hd), out_handle);
  }

  // msmz_scalars_dot: one partial sum per tile, one workgroup folds them; the result and the error word share a
  // 64-byte record in front of the partial sums and come back in ONE copy behind ONE host wait.
  int scalars_dot(uint64_t xh, uint64_t first_x, uint64_t yh, uint64_t first_y, uint64_t n, uint8_t* out) {
    HandleTable& handles = core_.handles_;
    if (!out || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    if (!handles.get(xh, 1) || (yh ? !handles.get(yh, 1) : first_y != 0)) return MSMZ_ERR_ARG;
    const uint32_t* X = handles.range(xh, 1, first_x, n, 8);
    const uint32_t* Y = yh ? handles.range(yh, 1, first_y, n, 8) : nullptr;
    if (!X || (yh && !Y)) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(core_.device_));
    hipStream_t stream = core_.stream_;
    const uint32_t tiles = (uint32_t)((n + SDOT_TILE - 1) / SDOT_TILE);
    // words 0..7: the result, word 8: the error word, from word 16: the partial sums
    const int st = core_.recorded(sdot_, 64 + (size_t)tiles * 32, [&](uint32_t* d_res) {
      hipLaunchKernelGGL((k_scalars_dot<Fr>), dim3(tiles), dim3(SDOT_THREADS), 0, stream, d_res + 16, X, Y, (uint32_t)n, d_res + 8);
      hipLaunchKernelGGL((k_scalars_dot_fold<Fr>), dim3(1), dim3(SDOT_THREADS), 0, stream, d_res, d_res + 16, tiles, Y ? 1 : 0);
    });
    if (st) return st;
    memcpy(out, core_.h_res_.p, 32);
    return MSMZ_OK;
  }

  // msmz_scalars_dot_many: every inner product of d.n_rows row vectors with d.n_cols column vectors.  ONE launch of
  // k_scalars_dot_many (dot_kernels.h; the grid of dot_many_plan) leaves `groups` partial sums per result, ONE launch
  // of k_scalars_dot_fold, one workgroup per result, folds them and converts; a resident destination gets a copy on
  // the stream.  The record is that of scalars_dot (word 8: the error word) with the results as its tail, so they and
  // the error word come back in ONE copy behind ONE host wait.  Every check comes before anything is queued.
  int scalars_dot_many(const msmz_dot_many& d, uint8_t* out_le32, uint64_t first_out, uint64_t* out_handle) {
    HandleTable& handles = core_.handles_;
    if (!d.rows || !d.cols || (!out_le32 && !out_handle)) return MSMZ_ERR_ARG;
    if (d.n_rows < 1 || d.n_rows > (uint32_t)DOT_MANY_MAX_ROWS || d.n_cols < 1 || d.n_cols > (uint32_t)DOT_MANY_MAX_COLS ||
        d.n == 0 || d.n >> 32 || d.flags)
      return MSMZ_ERR_ARG;
    const uint64_t dest = out_handle ? *out_handle : 0, results = (uint64_t)d.n_rows * d.n_cols;
    if (!dest && first_out != 0) return MSMZ_ERR_ARG;
    DotManyVecs V{};
    for (uint32_t r = 0; r < d.n_rows; r++)
      if (!(V.row[r] = handles.range(d.rows[r].handle, 1, d.rows[r].first, d.n, 8))) return MSMZ_ERR_ARG;
    for (uint32_t c = 0; c < d.n_cols; c++)
      if (!(V.col[c] = handles.range(d.cols[c].handle, 1, d.cols[c].first, d.n, 8))) return MSMZ_ERR_ARG;
    uint32_t* out = nullptr;
    if (dest) {
      if (!(out = handles.range(dest, 1, first_out, results, 8))) return MSMZ_ERR_ARG;
      for (uint32_t k = 0; k < d.n_rows + d.n_cols; k++) {   // no entry is both read and written, whatever the order
        const msmz_scalar_vec& v = k < d.n_rows ? d.rows[k] : d.cols[k - d.n_rows];
        if (v.handle == dest && ranges_meet(v.first, d.n, first_out, results)) return MSMZ_ERR_ARG;
      }
    }
    const DotManyPlan p = dot_many_plan(d.n, d.n_rows, d.n_cols, dot_many_groups_);
    MSMZ_HIP(hipSetDevice(core_.device_));
    Handle hd;
    if (out_handle)
      if (int st = core_.fresh_out(results, &hd, &out)) return st;
    hipStream_t stream = core_.stream_;
    typename Core::Record rec;
    rec.tail = (size_t)results * 32;
    // words 0..7: unused, word 8: the error word, from word 16: the results, behind them the partial sums
    const int st = core_.recorded(sdot_, (size_t)p.scratch_bytes, [&](uint32_t* d_res) {
      uint32_t* d_results = d_res + DOT_MANY_HEAD_BYTES / 4;
      uint32_t* partial = d_results + results * 8;
      const dim3 grid(p.groups, p.row_groups);
#define MSMZ_DOT_LAUNCH(NC)                                                                                            \
  case NC:                                                                                                             \
    hipLaunchKernelGGL((k_scalars_dot_many<Fr, NC>), grid, dim3(SDOT_THREADS), 0, stream, partial, V, d.n_rows,        \
                       (uint32_t)d.n, p.tiles, d_res + 8);                                                             \
    break
      switch (p.nc) {
        MSMZ_DOT_LAUNCH(1);
        MSMZ_DOT_LAUNCH(2);
        MSMZ_DOT_LAUNCH(3);
        MSMZ_DOT_LAUNCH(4);
        MSMZ_DOT_LAUNCH(5);
        MSMZ_DOT_LAUNCH(6);
        MSMZ_DOT_LAUNCH(7);
        MSMZ_DOT_LAUNCH(8);
      }
#undef MSMZ_DOT_LAUNCH
      static_assert(DOT_MANY_MAX_COLS == 8, "one instance per column count");
      hipLaunchKernelGGL((k_scalars_dot_fold<Fr>), dim3((uint32_t)results), dim3(SDOT_THREADS), 0, stream, d_results,
                         (const uint32_t*)partial, p.groups, 1);
      if (out) (void)hipMemcpyAsync(out, d_results, (size_t)results * 32, hipMemcpyDeviceToDevice, stream);
    }, rec);
    if (st) return st;
    if (out_le32) memcpy(out_le32, (const uint8_t*)core_.h_res_.p + DOT_MANY_HEAD_BYTES, (size_t)results * 32);
    return hd.mem.p ? core_.add_handle(std::move(hd), out_handle) : (int)MSMZ_OK;
  }

  // msmz_test_set_dot_many_groups: the most workgroups along n of scalars_dot_many, for later calls (0: the built-in value)
  int test_set_dot_many_groups(uint32_t g) {
    if (g > DOT_MANY_GROUPS) return MSMZ_ERR_ARG;
    dot_many_groups_ = g ? g : DOT_MANY_GROUPS;
    return MSMZ_OK;
  }

  // `count` entries at dst, entry i = base ratio^(set index of i), queued on the stream (k_scalars_powers).  The host
  // builds the table of ratio^(2^k) with fr.h; it travels as a kernel argument.  (ntt_ops.h fills its tables with this.)
  void launch_powers(uint32_t* dst, const FrConst& base, const uint32_t ratio[8], uint64_t count, const GenMap& map) {
    FrPowTable table;
    fr_pow_table<Fr>(table, ratio);
    hipLaunchKernelGGL((k_scalars_powers<Fr>), Core::blocks_of((count + SPOW_RUN - 1) / SPOW_RUN), dim3(kBlock), 0,
                       core_.stream_, dst, base, table, (uint32_t)count, map);
  }

  // msmz_scalars_powers: a new scalar handle, local entry i = base ratio^(set index of i)
  int scalars_powers(const uint8_t* base, const uint8_t* ratio, uint64_t n, const GenMap& map, uint64_t* h) {
    if (!h || !ratio || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    FrConst b{};
    uint32_t r[8];
    b.w[0] = 1;
    int st;
    if ((base && (st = Core::read_fr(base, b.w, false))) || (st = Core::read_fr(ratio, r, false))) return st;
    MSMZ_HIP(hipSetDevice(core_.device_));
    Handle hd;
    if ((st = core_.new_scalars(n, &hd))) return st;
    launch_powers(hd.mem.as<uint32_t>(), b, r, n, map);
    if ((st = core_.drained())) return st;
    return core_.add_handle(std::move(hd), h);
  }

  // msmz_scalars_recurrence: three launches (tile aggregates, ONE workgroup of carries, apply); the final value and the
  // error word share a 64-byte record in front of the scratch and come back in ONE copy behind ONE host wait.
  int scalars_recurrence(const msmz_scalar_rec& r, uint64_t n, uint64_t first_out, uint64_t* out_handle, uint8_t* last) {
    if (!out_handle || n == 0 || n >> 32 || (r.flags & ~(uint32_t)(MSMZ_REC_REVERSE | MSMZ_REC_EXCLUSIVE)))
      return MSMZ_ERR_ARG;
    if (!r.a_handle && !r.a && !r.b_handle) return MSMZ_ERR_ARG;   // y_i = y_(i-1): nothing to do
    const uint32_t *A = nullptr, *B = nullptr;
    std::vector<Source> srcs;
    if (r.a_handle) srcs.push_back({r.a_handle, r.a_first, &A});
    if (r.b_handle) srcs.push_back({r.b_handle, r.b_first, &B});
    uint32_t* out = nullptr;
    if (int st = core_.resolve(srcs, n, first_out, *out_handle, &out)) return st;
    FrConst k{}, init{};
    if (!r.a_handle && r.a)
      if (int st = Core::read_fr(r.a, k.w, true)) return st;
    if (r.init) {
      if (int st = Core::read_fr(r.init, init.w, false)) return st;
    } else if (!B) {
      init.w[0] = 1;
    }
    MSMZ_HIP(hipSetDevice(core_.device_));
    Handle hd;
    if (int st = core_.fresh_out(n, &hd, &out)) return st;
    hipStream_t stream = core_.stream_;
    const uint32_t tiles = (uint32_t)((n + SREC_TILE - 1) / SREC_TILE);
    // words 0..7: the final value, word 8: the error word; then the aggregates' A, their B, and tiles + 1 incoming values
    const int st = core_.recorded(sscan_, 64 + ((size_t)tiles * 3 + 1) * 32, [&](uint32_t* d_res) {
      uint32_t* aggA = d_res + 16;
      uint32_t* aggB = aggA + (size_t)tiles * 8;
      uint32_t* incoming = aggB + (size_t)tiles * 8;
      const uint32_t nn = (uint32_t)n, flags = r.flags;
      const dim3 grid(tiles), block(SREC_THREADS);
#define MSMZ_REC_LAUNCH(AM, HB)                                                                                          \
  do {                                                                                                                   \
    hipLaunchKernelGGL((k_scalars_rec_tile<Fr, AM, HB>), grid, block, 0, stream, aggA, aggB, A, B, k, nn, flags, d_res + 8); \
    hipLaunchKernelGGL((k_scalars_rec_carry<Fr, AM != SREC_A_NONE, HB>), dim3(1), block, 0, stream, incoming, d_res,     \
                       (const uint32_t*)aggA, (const uint32_t*)aggB, init, tiles);                                       \
    hipLaunchKernelGGL((k_scalars_rec_apply<Fr, AM, HB>), grid, block, 0, stream, out, A, B, k, (const uint32_t*)incoming, \
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
    if (last) memcpy(last, core_.h_res_.p, 32);
    return hd.mem.p ? core_.add_handle(std::move(hd), out_handle) : (int)MSMZ_OK;
  }

  // msmz_scalars_inverse: one launch; the error word and the zero count share the record
  int scalars_inverse(uint64_t h, uint64_t first, uint64_t n, uint64_t first_out, uint64_t* out_handle, uint64_t* n_zero) {
    if (!out_handle || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    const uint32_t* X = nullptr;
    uint32_t* out = nullptr;
    if (int st = core_.resolve({{h, first, &X}}, n, first_out, *out_handle, &out)) return st;
    MSMZ_HIP(hipSetDevice(core_.device_));
    Handle hd;
    if (int st = core_.fresh_out(n, &hd, &out)) return st;
    const uint64_t per_block = (uint64_t)SINV_THREADS * SINV_E;
    const int st = core_.recorded(sscan_, 64, [&](uint32_t* d_res) {   // word 8: the error word, word 9: the zeros
      hipLaunchKernelGGL((k_scalars_inverse<Fr>), dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(SINV_THREADS), 0,
                         core_.stream_, out, X, (uint32_t)n, d_res);
    });
    if (st) return st;
    if (n_zero) *n_zero = core_.h_res_.template as<const uint32_t>()[9];
    return hd.mem.p ? core_.add_handle(std::move(hd), out_handle) : (int)MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ multilinear polynomials
  // msmz_scalars_eq_table: a new scalar handle, entry i = scale eq(r, i).  The host brings the point to Montgomery form;
  // it travels as a kernel argument (k_scalars_eq_table, mle_kernels.h).  One launch, no error word: nothing is read.
  int scalars_eq_table(const uint8_t* point, uint32_t n_vars, const uint8_t* scale, uint64_t* h) {
    if (!h || n_vars > (uint32_t)MLE_MAX_VARS || (n_vars && !point)) return MSMZ_ERR_ARG;
    FrConst s{};
    FrEqPoint pt;
    s.w[0] = 1;
    int st;
    if ((scale && (st = Core::read_fr(scale, s.w, false))) || (st = read_point(point, n_vars, &pt))) return st;
    const uint64_t n = 1ull << n_vars;
    MSMZ_HIP(hipSetDevice(core_.device_));
    Handle hd;
    if ((st = core_.new_scalars(n, &hd))) return st;
    hipLaunchKernelGGL((k_scalars_eq_table<Fr>), Core::blocks_of((n + MLE_RUN - 1) / MLE_RUN), dim3(kBlock), 0, core_.stream_,
                       hd.mem.as<uint32_t>(), s, pt, n_vars);
    if ((st = core_.drained())) return st;
    return core_.add_handle(std::move(hd), h);
  }

  // msmz_scalars_mle_eval: scalars_dot with the second operand generated -- one partial sum per tile of MLE_TILE
  // entries, the same fold, the same result record behind ONE host wait.
  int scalars_mle_eval(uint64_t xh, uint64_t first, uint32_t n_vars, const uint8_t* point, uint8_t* out) {
    if (!out || n_vars > (uint32_t)MLE_MAX_VARS || (n_vars && !point)) return MSMZ_ERR_ARG;
    const uint64_t n = 1ull << n_vars;
    const uint32_t* X = core_.handles_.range(xh, 1, first, n, 8);
    if (!X) return MSMZ_ERR_ARG;
    FrEqPoint pt;
    if (int st = read_point(point, n_vars, &pt)) return st;
    MSMZ_HIP(hipSetDevice(core_.device_));
    hipStream_t stream = core_.stream_;
    const uint32_t tiles = (uint32_t)((n + MLE_TILE - 1) / MLE_TILE);
    // words 0..7: the result, word 8: the error word, from word 16: the partial sums
    const int st = core_.recorded(sdot_, 64 + (size_t)tiles * 32, [&](uint32_t* d_res) {
      hipLaunchKernelGGL((k_scalars_mle_eval<Fr>), dim3(tiles), dim3(SDOT_THREADS), 0, stream, d_res + 16, X, pt, n_vars, d_res + 8);
      hipLaunchKernelGGL((k_scalars_dot_fold<Fr>), dim3(1), dim3(SDOT_THREADS), 0, stream, d_res, d_res + 16, tiles, 1);
    });
    if (st) return st;
    memcpy(out, core_.h_res_.p, 32);
    return MSMZ_OK;
  }

  // msmz_scalars_mle_bind: one launch, one thread per output; the error word (a resident record >= q) comes back behind
  // the ONE host wait.  One table and the high variable: the two halves are two sources of `resolve`, so the destination
  // may be a half exactly or apart from both -- and the high half is refused here, as the header says.  Any other shape:
  // the whole source is one range of another length than the destination, which `resolve` lets meet nowhere.
  int scalars_mle_bind(const msmz_mle_bind& b, uint64_t first_out, uint64_t* out_handle) {
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
      if (!core_.handles_.range(b.handle, 1, b.first, n, 8)) return MSMZ_ERR_ARG;   // (the whole source: first + h cannot wrap)
      if (*out_handle == b.handle && first_out == b.first + h) return MSMZ_ERR_ARG;
      if (int st = core_.resolve({{b.handle, b.first, &in}, {b.handle, b.first + h, &hi}}, h, first_out, *out_handle, &out)) return st;
    } else if (int st = core_.resolve({{b.handle, b.first, &in, total_in}}, total_out, first_out, *out_handle, &out)) {
      return st;
    }
    FrConst r{};
    if (int st = Core::read_fr(b.r, r.w, true)) return st;
    MSMZ_HIP(hipSetDevice(core_.device_));
    Handle hd;
    if (int st = core_.fresh_out(total_out, &hd, &out)) return st;
    const int st = core_.checked([&](uint32_t* d_err) {   // a resident record >= group order
      hipLaunchKernelGGL((k_scalars_mle_bind<Fr>), Core::blocks_of(total_out), dim3(kBlock), 0, core_.stream_, out, in, r,
                         b.n_vars, (uint32_t)total_out, low ? 1 : 0, d_err);
    });
    return st || !hd.mem.p ? st : core_.add_handle(std::move(hd), out_handle);
  }

  // msmz_scalars_sumcheck_round: degree + 1 partial sums per tile of MSC_TILE pair indices, one workgroup of the fold per
  // value; the values and the error word share a record of MSC_HEAD_BYTES in front of the partial sums and come back in
  // ONE copy behind ONE host wait.  The coefficients go to c 2^(256 f) here (fr_sc_coeff), f the factors of the term.
  int scalars_sumcheck_round(const msmz_sumcheck& s, uint32_t* degree, uint8_t* evals) {
    if (!degree || !evals || !s.tables || !s.terms || s.n_tables < 1 || s.n_tables > (uint32_t)MSC_MAX_TABLES ||
        s.n_terms < 1 || s.n_terms > (uint32_t)MSC_MAX_TERMS || s.n_vars == 0 || s.n_vars > (uint32_t)MLE_MAX_VARS ||
        (s.flags & ~(uint32_t)MSMZ_MLE_LOW))
      return MSMZ_ERR_ARG;
    const uint64_t n = 1ull << s.n_vars;
    ScTables tab{};
    for (uint32_t j = 0; j < s.n_tables; j++)
      if (!(tab.p[j] = core_.handles_.range(s.tables[j].handle, 1, s.tables[j].first, n, 8))) return MSMZ_ERR_ARG;
    FrScTerms T{};
    if (int st = read_masks(s.terms, s.n_terms, s.n_tables, &T)) return st;
    if (int st = read_coeffs(s.terms, &T)) return st;
    MSMZ_HIP(hipSetDevice(core_.device_));
    hipStream_t stream = core_.stream_;
    const uint32_t half = (uint32_t)(n >> 1), tiles = (half + MSC_TILE - 1) / MSC_TILE, values = T.degree + 1;
    const int low = (s.flags & MSMZ_MLE_LOW) ? 1 : 0;
    typename Core::Record rec;   // several values to bring back: a longer head, the error word behind them
    rec.head = MSC_HEAD_BYTES, rec.err_word = MSC_ERR_WORD;
    const int st = core_.recorded(sdot_, MSC_HEAD_BYTES + (size_t)values * tiles * 32, [&](uint32_t* d_res) {
      uint32_t* partial = d_res + MSC_HEAD_BYTES / 4;
      uint32_t* d_err = d_res + MSC_ERR_WORD;
#define MSMZ_SC_LAUNCH(NT)                                                                                           \
  case NT:                                                                                                           \
    hipLaunchKernelGGL((k_scalars_sumcheck_round<Fr, NT>), dim3(tiles), dim3(SDOT_THREADS), 0, stream, partial, tab, T, \
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
      hipLaunchKernelGGL((k_scalars_dot_fold<Fr>), dim3(values), dim3(SDOT_THREADS), 0, stream, d_res, (const uint32_t*)partial,
                         tiles, 0);
    }, rec);
    if (st) return st;
    *degree = T.degree;
    memcpy(evals, core_.h_res_.p, (size_t)values * 32);
    return MSMZ_OK;
  }

  // msmz_scalars_sumcheck_step: mle_bind of every table and sumcheck_round over what it wrote, in ONE launch plus the
  // fold (k_scalars_sumcheck_step, mle_kernels.h; k_scalars_sumcheck_last for tables of one variable) -- the record, the
  // partial sums, the fold and the ONE host wait are the round's, over quarter = 2^(n_vars - 2) new pair indices.  Every
  // argument check, the overlap rules of the header among them, comes before the host values are read (MSMZ_ERR_RANGE)
  // and both before anything is queued.
  int scalars_sumcheck_step(const msmz_sumcheck_step& s, uint32_t* degree, uint8_t* evals) {
    if (!degree || !evals || !s.tables || !s.terms || !s.r || s.n_tables < 1 || s.n_tables > (uint32_t)MSC_MAX_TABLES ||
        s.n_terms < 1 || s.n_terms > (uint32_t)MSC_MAX_TERMS || s.n_vars == 0 || s.n_vars > (uint32_t)MLE_MAX_VARS ||
        (s.flags & ~(uint32_t)MSMZ_MLE_LOW))
      return MSMZ_ERR_ARG;
    const uint64_t n = 1ull << s.n_vars, h = n >> 1;
    const bool low = (s.flags & MSMZ_MLE_LOW) != 0, last = s.n_vars == 1;
    const msmz_sumcheck_table* dst = s.out ? s.out : s.tables;   // (in place: the low half starts where the source does)
    ScTables tab{};
    ScOuts out{};
    for (uint32_t j = 0; j < s.n_tables; j++) {
      if (!(tab.p[j] = core_.handles_.range(s.tables[j].handle, 1, s.tables[j].first, n, 8))) return MSMZ_ERR_ARG;
      if (!(out.p[j] = core_.handles_.range(dst[j].handle, 1, dst[j].first, h, 8))) return MSMZ_ERR_ARG;
    }
    for (uint32_t j = 0; j < s.n_tables; j++) {
      for (uint32_t k = 0; k < s.n_tables; k++) {
        if (k < j && dst[j].handle == dst[k].handle && ranges_meet(dst[j].first, h, dst[k].first, h)) return MSMZ_ERR_ARG;
        if (dst[j].handle != s.tables[k].handle || !ranges_meet(dst[j].first, h, s.tables[k].first, n)) continue;
        // a destination on a source: its own, as the low half, in the high order, and nothing else
        if (k != j || low || dst[j].first != s.tables[j].first) return MSMZ_ERR_ARG;
      }
    }
    FrScTerms T{};
    if (int st = read_masks(s.terms, s.n_terms, s.n_tables, &T)) return st;
    FrConst r{};
    if (int st = Core::read_fr(s.r, r.w, true)) return st;
    if (int st = read_coeffs(s.terms, &T)) return st;
    if (last) T.degree = 0;   // no variable is left: the one value is the terms over the one-entry tables
    MSMZ_HIP(hipSetDevice(core_.device_));
    hipStream_t stream = core_.stream_;
    const uint32_t quarter = last ? 1u : (uint32_t)(h >> 1), tiles = (quarter + MSC_TILE - 1) / MSC_TILE, values = T.degree + 1;
    typename Core::Record rec;
    rec.head = MSC_HEAD_BYTES, rec.err_word = MSC_ERR_WORD;
    const int st = core_.recorded(sdot_, MSC_HEAD_BYTES + (size_t)values * tiles * 32, [&](uint32_t* d_res) {
      uint32_t* partial = d_res + MSC_HEAD_BYTES / 4;
      uint32_t* d_err = d_res + MSC_ERR_WORD;
      if (last) {
        hipLaunchKernelGGL((k_scalars_sumcheck_last<Fr>), dim3(1), dim3(64), 0, stream, partial, out, tab, T, r, s.n_tables, d_err);
      } else if (s.n_tables > (uint32_t)MSC_STEP_FUSED_TABLES) {
        // the table counts the fused kernel does not have without scratch: the bind kernel per table and the round kernel
        // over the destinations, queued behind each other -- the same bytes written and returned, the same ONE wait
        ScTables bound{};
        for (uint32_t j = 0; j < s.n_tables; j++) {
          bound.p[j] = out.p[j];
          hipLaunchKernelGGL((k_scalars_mle_bind<Fr>), Core::blocks_of(h), dim3(kBlock), 0, stream, out.p[j], tab.p[j], r, s.n_vars,
                             (uint32_t)h, low ? 1 : 0, d_err);
        }
        hipLaunchKernelGGL((k_scalars_sumcheck_round<Fr, MSC_MAX_TABLES>), dim3(tiles), dim3(SDOT_THREADS), 0, stream, partial,
                           bound, T, quarter, low ? 1 : 0, d_err);
        static_assert(MSC_STEP_FUSED_TABLES + 1 == MSC_MAX_TABLES, "one table count takes this route");
      } else {
#define MSMZ_SC_LAUNCH(NT)                                                                                             \
  case NT:                                                                                                             \
    hipLaunchKernelGGL((k_scalars_sumcheck_step<Fr, NT>), dim3(tiles), dim3(SDOT_THREADS), 0, stream, partial, out, tab, T, \
                       r, quarter, low ? 1 : 0, d_err);                                                                \
    break
        switch (s.n_tables) {
          MSMZ_SC_LAUNCH(1);
          MSMZ_SC_LAUNCH(2);
          MSMZ_SC_LAUNCH(3);
          MSMZ_SC_LAUNCH(4);
          MSMZ_SC_LAUNCH(5);
        }
#undef MSMZ_SC_LAUNCH
        static_assert(MSC_STEP_FUSED_TABLES == 5, "one instance per table count");
      }
      hipLaunchKernelGGL((k_scalars_dot_fold<Fr>), dim3(values), dim3(SDOT_THREADS), 0, stream, d_res, (const uint32_t*)partial,
                         tiles, 0);
    }, rec);
    if (st) return st;
    *degree = T.degree;
    memcpy(evals, core_.h_res_.p, (size_t)values * 32);
    return MSMZ_OK;
  }

 private:
  // the masks of a round's terms into T, with its degree (MSMZ_ERR_ARG), and then the coefficients, c 2^(256 f) for a
  // term of f factors (fr_sc_coeff; MSMZ_ERR_RANGE): two steps, so that a caller finishes its argument checks in between
  static int read_masks(const msmz_sumcheck_term* terms, uint32_t n_terms, uint32_t n_tables, FrScTerms* T) {
    T->n_terms = n_terms;
    for (uint32_t k = 0; k < n_terms; k++) {
      const uint32_t m = terms[k].mask, f = (uint32_t)__builtin_popcount(m);
      if (m == 0 || (m >> n_tables) || f > (uint32_t)MSC_MAX_DEGREE) return MSMZ_ERR_ARG;
      T->mask[k] = m;
      if (f > T->degree) T->degree = f;
    }
    return MSMZ_OK;
  }
  static int read_coeffs(const msmz_sumcheck_term* terms, FrScTerms* T) {
    for (uint32_t k = 0; k < T->n_terms; k++) {
      uint32_t c[8] = {1, 0, 0, 0, 0, 0, 0, 0};
      if (terms[k].coeff)
        if (int st = Core::read_fr(terms[k].coeff, c, false)) return st;
      fr_sc_coeff<Fr>(T->coeff[k], c, __builtin_popcount(T->mask[k]));
    }
    return MSMZ_OK;
  }

  // the point of an eq table or an evaluation (n_vars values of 32 bytes, each < q) in the form the kernels take
  static int read_point(const uint8_t* point, uint32_t n_vars, FrEqPoint* pt) {
    memset(pt, 0, sizeof(*pt));
    for (uint32_t j = 0; j < n_vars; j++)
      if (int st = Core::read_fr(point + (size_t)32 * j, pt->r[j], true)) return st;
    return MSMZ_OK;
  }
  static_assert(MSC_MAX_TABLES == MSMZ_SUMCHECK_MAX_TABLES && MSC_MAX_DEGREE == MSMZ_SUMCHECK_MAX_DEGREE &&
                    MSC_MAX_TERMS == MSMZ_SUMCHECK_MAX_TERMS,
                "the limits of include/msmz.h are those of mle_kernels.h");

  static_assert(MSMZ_DOT_MANY_MAX_ROWS == DOT_MANY_MAX_ROWS && MSMZ_DOT_MANY_MAX_COLS == DOT_MANY_MAX_COLS,
                "the limits of include/msmz.h are those of dot_kernels.h");

  Core& core_;
  uint32_t dot_many_groups_ = DOT_MANY_GROUPS;   // (msmz_test_set_dot_many_groups lowers it)
  DevBuf sdot_;    // scalars_dot, scalars_dot_many (at most DOT_MANY_SCRATCH_MAX) and the multilinear calls: the result
                   // record, then the partial sums
  DevBuf sscan_;   // scalars_recurrence / _inverse: the result record, then aggregates and incoming values
};

}  // namespace msmz

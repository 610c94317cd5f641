// C ABI of the MSM engine (include/msmz.h): curve dispatch + argument checking.
#include "instantiate.h"
namespace msmz {
#define X(F, Fr) MSMZ_INST_BATCH(F, Fr, MSMZ_EXTERN) MSMZ_INST_REDUCE(F, Fr, MSMZ_EXTERN) MSMZ_INST_MISC(F, Fr, MSMZ_EXTERN) MSMZ_INST_GEN(F, Fr, MSMZ_EXTERN) MSMZ_INST_MLE(F, Fr, MSMZ_EXTERN) MSMZ_INST_MATRIX(F, Fr, MSMZ_EXTERN) MSMZ_INST_LOOKUP(F, Fr, MSMZ_EXTERN) MSMZ_INST_EXPR(F, Fr, MSMZ_EXTERN) MSMZ_INST_DOT(F, Fr, MSMZ_EXTERN)
MSMZ_WEIERSTRASS_FIELDS(X)
#undef X
#define X(F, Fr) MSMZ_INST_REDUCE_TE(F, Fr, MSMZ_EXTERN) MSMZ_INST_MISC_TE(F, Fr, MSMZ_EXTERN) MSMZ_INST_GEN_TE(F, Fr, MSMZ_EXTERN) MSMZ_INST_MLE(F, Fr, MSMZ_EXTERN) MSMZ_INST_MATRIX(F, Fr, MSMZ_EXTERN) MSMZ_INST_LOOKUP(F, Fr, MSMZ_EXTERN) MSMZ_INST_EXPR(F, Fr, MSMZ_EXTERN) MSMZ_INST_DOT(F, Fr, MSMZ_EXTERN)
MSMZ_TE_FIELDS(X)
#undef X
}  // namespace msmz
#include "test_hooks.h"

namespace msmz {

// Curve configurations: field structs, group policy (kernels.h) and curve form (the engine picks the MSM path, Engine::run_problems).
template <class F_, class Fr_>
struct WeierCfg {
  using F = F_;
  using Fr = Fr_;
  using P = WeierPolicy<F>;
  static constexpr bool TE = false;
  static constexpr bool HAS_ENDO = true;
};

template <class F_, class Fr_>
struct TeCfg {
  using F = F_;
  using Fr = Fr_;
  using P = TePolicy<F>;
  static constexpr bool TE = true;
  static constexpr bool HAS_ENDO = false;
};

using CfgBls377 = WeierCfg<Bls377Fp, Bls377Fr>;
using CfgPallas = WeierCfg<PallasFp, PallasFr>;
using CfgBls381 = WeierCfg<Bls381Fp, Bls381Fr>;
using CfgEd377 = TeCfg<Ed377Fp, Ed377Fr>;

}  // namespace msmz

using namespace msmz;

struct msmz_ctx {
  int curve_id;
  IEngine* engine;
  int n_devices;
};

extern "C" {

const char* msmz_strerror(int status) {
  switch (status) {
    case MSMZ_OK: return "ok";
    case MSMZ_ERR_ARG: return "bad argument";
    case MSMZ_ERR_NO_DEVICE: return "no usable HIP device (there is no CPU fallback)";
    case MSMZ_ERR_HIP: return "HIP runtime error";
    case MSMZ_ERR_UNSUPPORTED: return "option combination not supported for this curve";
    case MSMZ_ERR_DEGENERATE: return "unsafe batched addition hit a zero denominator (equal or opposite points); use safe=1";
    case MSMZ_ERR_RANGE: return "scalar >= group order or coordinate >= field modulus";
    case MSMZ_ERR_POINT: return "a compressed record is not a point of the curve";
    default: return "unknown status";
  }
}

int msmz_curve_fe_bytes(int curve_id) {
  switch (curve_id) {
    case MSMZ_BLS12_377_G1:
    case MSMZ_BLS12_381_G1: return 48;
    case MSMZ_PALLAS:
    case MSMZ_ED_ON_BLS12_377: return 32;
    default: return -1;
  }
}

int msmz_ctx_fe_bytes(const msmz_ctx* c) { return c ? msmz_curve_fe_bytes(c->curve_id) : -1; }
int msmz_ctx_n_devices(const msmz_ctx* c) { return c ? c->n_devices : -1; }

static IEngine* make_engine(int curve_id, int device, int* st) {
  IEngine* eng = nullptr;
  *st = MSMZ_ERR_UNSUPPORTED;
  auto make = [&](auto* e) {
    *st = e->init();
    eng = e;
  };
  switch (curve_id) {
    case MSMZ_BLS12_377_G1: make(new Engine<CfgBls377>(curve_id, device)); break;
    case MSMZ_PALLAS: make(new Engine<CfgPallas>(curve_id, device)); break;
    case MSMZ_BLS12_381_G1: make(new Engine<CfgBls381>(curve_id, device)); break;
    case MSMZ_ED_ON_BLS12_377: make(new Engine<CfgEd377>(curve_id, device)); break;
    default: break;
  }
  if (*st != MSMZ_OK) {
    delete eng;
    eng = nullptr;
  }
  return eng;
}

int msmz_create(msmz_ctx** out, int curve_id, const int* device_ids, int n_devices) {
  if (!out) return MSMZ_ERR_ARG;
  *out = nullptr;
  if (msmz_curve_fe_bytes(curve_id) < 0) return MSMZ_ERR_ARG;
  if (n_devices == 0) return MSMZ_ERR_NO_DEVICE;   // there is no CPU backend
  if (n_devices < 0 || n_devices > MSMZ_MAX_DEVICES || !device_ids) return MSMZ_ERR_ARG;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return MSMZ_ERR_NO_DEVICE;
  for (int i = 0; i < n_devices; i++)
    if (device_ids[i] < 0 || device_ids[i] >= count) return MSMZ_ERR_ARG;
  int st = MSMZ_OK;
  if (n_devices == 1) {
    IEngine* eng = make_engine(curve_id, device_ids[0], &st);
    if (!eng) return st;
    *out = new msmz_ctx{curve_id, eng, 1};
    return MSMZ_OK;
  }
  // one engine (own HIP stream, own buffers) per listed device; the same id may be listed more than once
  std::vector<IEngine*> engines;
  for (int i = 0; i < n_devices; i++) {
    IEngine* eng = make_engine(curve_id, device_ids[i], &st);
    if (!eng) {
      for (IEngine* e : engines) delete e;
      return st;
    }
    engines.push_back(eng);
  }
  *out = new msmz_ctx{curve_id, new MultiEngine(curve_id, msmz_curve_fe_bytes(curve_id), engines), n_devices};
  return MSMZ_OK;
}

void msmz_destroy(msmz_ctx* ctx) {
  if (!ctx) return;
  delete ctx->engine;
  delete ctx;
}

int msmz_upload_points(msmz_ctx* c, const uint8_t* xy, const uint8_t* inf, uint64_t n, uint64_t* h) {
  return c ? c->engine->upload_points(xy, inf, n, h) : MSMZ_ERR_ARG;
}
int msmz_upload_scalars(msmz_ctx* c, const uint8_t* s, uint64_t n, uint64_t* h) {
  return c ? c->engine->upload_scalars(s, n, h) : MSMZ_ERR_ARG;
}
int msmz_import_scalars(msmz_ctx* c, const msmz_src* s, uint64_t n, uint64_t* h) {
  return c && s ? c->engine->import_scalars(*s, n, h) : MSMZ_ERR_ARG;
}
int msmz_import_scalars_into(msmz_ctx* c, uint64_t h, uint64_t first, const msmz_src* s, uint64_t n) {
  return c && s ? c->engine->import_scalars_into(h, first, *s, n) : MSMZ_ERR_ARG;
}
int msmz_alloc_scalars(msmz_ctx* c, uint64_t n, uint64_t* h) { return c ? c->engine->alloc_scalars(n, h) : MSMZ_ERR_ARG; }
int msmz_import_points(msmz_ctx* c, const msmz_src* s, uint64_t n, uint64_t* h) {
  return c && s ? c->engine->import_points(*s, n, h) : MSMZ_ERR_ARG;
}
int msmz_random_points(msmz_ctx* c, uint64_t n, uint64_t seed, uint64_t* h) {
  return c ? c->engine->random_points(n, seed, GenMap{}, h) : MSMZ_ERR_ARG;
}
int msmz_random_scalars(msmz_ctx* c, uint64_t n, uint64_t seed, uint64_t* h) {
  return c ? c->engine->random_scalars(n, seed, GenMap{}, h) : MSMZ_ERR_ARG;
}
int msmz_download_points(msmz_ctx* c, uint64_t h, uint64_t first, uint64_t count, uint8_t* xy, uint8_t* inf) {
  return c ? c->engine->download_points(h, first, count, xy, inf) : MSMZ_ERR_ARG;
}
int msmz_download_points_compressed(msmz_ctx* c, uint64_t h, uint64_t first, uint64_t count, uint8_t* out, uint8_t* inf,
                                    uint32_t flags) {
  return c ? c->engine->download_points_compressed(h, first, count, out, inf, flags) : MSMZ_ERR_ARG;
}
int msmz_download_scalars(msmz_ctx* c, uint64_t h, uint64_t first, uint64_t count, uint8_t* s) {
  return c ? c->engine->download_scalars(h, first, count, s) : MSMZ_ERR_ARG;
}
int msmz_export_scalars(msmz_ctx* c, uint64_t h, uint64_t first, uint64_t n, const msmz_dst* d) {
  return c && d ? c->engine->export_scalars(h, first, n, *d) : MSMZ_ERR_ARG;
}
int msmz_export_points(msmz_ctx* c, uint64_t h, uint64_t first, uint64_t n, const msmz_dst* d) {
  return c && d ? c->engine->export_points(h, first, n, *d) : MSMZ_ERR_ARG;
}
int msmz_free(msmz_ctx* c, uint64_t h) { return c ? c->engine->free_handle(h) : MSMZ_ERR_ARG; }

int msmz_msm(msmz_ctx* c, uint64_t ph, const uint8_t* scalars, uint64_t n, const msmz_opts* o, uint8_t* out,
             int* out_inf, msmz_log* log) {
  if (!c || !scalars) return MSMZ_ERR_ARG;
  return c->engine->msm_batch(ph, scalars, 0, n, 1, o, out, out_inf, log);
}
int msmz_msm_resident(msmz_ctx* c, uint64_t ph, uint64_t sh, uint64_t n, const msmz_opts* o, uint8_t* out,
                      int* out_inf, msmz_log* log) {
  if (!c) return MSMZ_ERR_ARG;
  return c->engine->msm_batch(ph, nullptr, sh, n, 1, o, out, out_inf, log);
}

int msmz_msm_batch(msmz_ctx* c, uint64_t ph, const uint8_t* scalars, uint64_t n, uint32_t batch, const msmz_opts* o,
                   uint8_t* out, int* out_inf, msmz_log* log) {
  if (!c || !scalars) return MSMZ_ERR_ARG;
  return c->engine->msm_batch(ph, scalars, 0, n, batch, o, out, out_inf, log);
}
int msmz_msm_batch_resident(msmz_ctx* c, uint64_t ph, uint64_t sh, uint64_t n, uint32_t batch, const msmz_opts* o,
                            uint8_t* out, int* out_inf, msmz_log* log) {
  if (!c) return MSMZ_ERR_ARG;
  return c->engine->msm_batch(ph, nullptr, sh, n, batch, o, out, out_inf, log);
}

int msmz_msm_segments(msmz_ctx* c, uint64_t ph, uint64_t sh, const msmz_segment* segs, uint32_t n_segs, const msmz_opts* o,
                      uint8_t* out, int* out_inf, msmz_log* log) {
  if (!c || !segs || !out || !out_inf || n_segs == 0) return MSMZ_ERR_ARG;
  return c->engine->msm_segments(ph, sh, segs, n_segs, o, out, out_inf, log);
}

int msmz_precompute_points(msmz_ctx* c, uint64_t ph, uint64_t n, const msmz_opts* o, uint32_t factor, uint64_t* h) {
  if (!c || !h) return MSMZ_ERR_ARG;
  int cc = 0, glv = 0, sbits = 0;
  uint32_t copies = 0;
  const int st = c->engine->precompute_params(n, o, factor, &cc, &glv, &copies, nullptr, &sbits);
  if (st) return st;
  return c->engine->precompute_points(ph, n, cc, glv, copies, sbits, h);
}
int msmz_precomputed_info(msmz_ctx* c, uint64_t h, int32_t* cc, int32_t* glv, uint32_t* factor, uint32_t* K,
                          uint64_t* records) {
  return c ? c->engine->precomputed_info(h, cc, glv, factor, K, records, nullptr) : MSMZ_ERR_ARG;
}
int msmz_precomputed_scalar_bits(msmz_ctx* c, uint64_t h, int32_t* bits) {
  if (!c || !bits) return MSMZ_ERR_ARG;
  return c->engine->precomputed_info(h, nullptr, nullptr, nullptr, nullptr, nullptr, bits);
}

int msmz_check_points(msmz_ctx* c, uint64_t ph, uint64_t first, uint64_t count, uint32_t what, msmz_check_result* out,
                      uint8_t* verdicts) {
  return c ? c->engine->check_points(ph, first, count, what, out, verdicts) : MSMZ_ERR_ARG;
}

int msmz_points_mul(msmz_ctx* c, const msmz_mul* m, uint64_t n, uint64_t* h) {
  return msmz_points_mul_opts(c, m, n, nullptr, h);
}
int msmz_points_mul_opts(msmz_ctx* c, const msmz_mul* m, uint64_t n, const msmz_mul_opts* opts, uint64_t* h) {
  const msmz_mul_opts o = opts ? *opts : msmz_mul_opts{};
  if (!c || !m) return MSMZ_ERR_ARG;
  if ((o.flags & ~(uint32_t)MSMZ_MUL_SUBGROUP) || o.reserved[0] || o.reserved[1] || o.scalar_bits < 0 || o.scalar_bits > 256)
    return MSMZ_ERR_ARG;
  return c->engine->points_mul(*m, o, n, h);
}

int msmz_points_fixed_base(msmz_ctx* c, const msmz_fixed_base* f, uint64_t n, uint64_t* h) {
  if (!c || !f || !h) return MSMZ_ERR_ARG;
  if (f->flags || f->scalar_bits < 0 || f->scalar_bits > 256) return MSMZ_ERR_ARG;
  return c->engine->points_fixed_base(*f, n, h);
}

int msmz_scalars_combine(msmz_ctx* c, const msmz_scalar_term* x, const msmz_scalar_term* y, uint64_t n, uint64_t first_out,
                         uint64_t* out_handle) {
  return c && x && out_handle ? c->engine->scalars_combine(*x, y, n, first_out, out_handle) : MSMZ_ERR_ARG;
}
int msmz_scalars_dot(msmz_ctx* c, uint64_t xh, uint64_t first_x, uint64_t yh, uint64_t first_y, uint64_t n, uint8_t* out) {
  return c && out ? c->engine->scalars_dot(xh, first_x, yh, first_y, n, out) : MSMZ_ERR_ARG;
}
int msmz_scalars_powers(msmz_ctx* c, const uint8_t* base, const uint8_t* ratio, uint64_t n, uint64_t* h) {
  return c && ratio && h ? c->engine->scalars_powers(base, ratio, n, GenMap{}, h) : MSMZ_ERR_ARG;
}
int msmz_scalars_recurrence(msmz_ctx* c, const msmz_scalar_rec* r, uint64_t n, uint64_t first_out, uint64_t* out_handle,
                            uint8_t* last) {
  return c && r && out_handle ? c->engine->scalars_recurrence(*r, n, first_out, out_handle, last) : MSMZ_ERR_ARG;
}
int msmz_scalars_inverse(msmz_ctx* c, uint64_t h, uint64_t first, uint64_t n, uint64_t first_out, uint64_t* out_handle,
                         uint64_t* n_zero) {
  return c && out_handle ? c->engine->scalars_inverse(h, first, n, first_out, out_handle, n_zero) : MSMZ_ERR_ARG;
}
int msmz_scalars_ntt(msmz_ctx* c, const msmz_ntt* t, uint64_t first_out, uint64_t* out_handle) {
  return c && t && out_handle ? c->engine->scalars_ntt(*t, first_out, out_handle) : MSMZ_ERR_ARG;
}
int msmz_scalars_eq_table(msmz_ctx* c, const uint8_t* point, uint32_t n_vars, const uint8_t* scale, uint64_t* h) {
  return c && h ? c->engine->scalars_eq_table(point, n_vars, scale, h) : MSMZ_ERR_ARG;
}
int msmz_scalars_mle_eval(msmz_ctx* c, uint64_t h, uint64_t first, uint32_t n_vars, const uint8_t* point, uint8_t* out) {
  return c && out ? c->engine->scalars_mle_eval(h, first, n_vars, point, out) : MSMZ_ERR_ARG;
}
int msmz_scalars_mle_bind(msmz_ctx* c, const msmz_mle_bind* b, uint64_t first_out, uint64_t* out_handle) {
  return c && b && out_handle ? c->engine->scalars_mle_bind(*b, first_out, out_handle) : MSMZ_ERR_ARG;
}
int msmz_scalars_sumcheck_round(msmz_ctx* c, const msmz_sumcheck* s, uint32_t* degree, uint8_t* evals) {
  return c && s && degree && evals ? c->engine->scalars_sumcheck_round(*s, degree, evals) : MSMZ_ERR_ARG;
}
int msmz_scalars_sumcheck_step(msmz_ctx* c, const msmz_sumcheck_step* s, uint32_t* degree, uint8_t* evals) {
  return c && s && degree && evals ? c->engine->scalars_sumcheck_step(*s, degree, evals) : MSMZ_ERR_ARG;
}
int msmz_matrix_create(msmz_ctx* c, const msmz_sparse* s, uint64_t* h) {
  return c && s && h ? c->engine->matrix_create(*s, h) : MSMZ_ERR_ARG;
}
int msmz_matrix_info(msmz_ctx* c, uint64_t h, uint32_t* n_rows, uint32_t* n_cols, uint64_t* nnz, uint32_t* flags) {
  return c ? c->engine->matrix_info(h, n_rows, n_cols, nnz, flags) : MSMZ_ERR_ARG;
}
int msmz_matrix_mul(msmz_ctx* c, const msmz_matvec* v, uint64_t first_out, uint64_t* out_handle) {
  return c && v && out_handle ? c->engine->matrix_mul(*v, first_out, out_handle) : MSMZ_ERR_ARG;
}
int msmz_scalars_lookup(msmz_ctx* c, const msmz_lookup* l, uint64_t first_out, uint64_t* out_handle, msmz_lookup_result* res) {
  return c && l && out_handle ? c->engine->scalars_lookup(*l, first_out, out_handle, res) : MSMZ_ERR_ARG;
}
int msmz_scalars_expr(msmz_ctx* c, const msmz_expr* e, uint64_t first_out, uint64_t* out_handle) {
  return c && e && out_handle ? c->engine->scalars_expr(*e, first_out, out_handle) : MSMZ_ERR_ARG;
}
int msmz_scalars_dot_many(msmz_ctx* c, const msmz_dot_many* d, uint8_t* out_le32, uint64_t first_out, uint64_t* out_handle) {
  return c && d ? c->engine->scalars_dot_many(*d, out_le32, first_out, out_handle) : MSMZ_ERR_ARG;
}
void msmz_test_dot_many_geometry(uint32_t* tile_elements, uint32_t* max_groups, uint32_t* rows_per_block) {
  if (tile_elements) *tile_elements = SDOT_TILE;
  if (max_groups) *max_groups = DOT_MANY_GROUPS;
  if (rows_per_block)
    for (int nc = 1; nc <= DOT_MANY_MAX_COLS; nc++) rows_per_block[nc - 1] = (uint32_t)dot_many_rg(nc);
}
int msmz_test_set_dot_many_groups(msmz_ctx* c, uint32_t max_groups) {
  return c ? c->engine->test_set_dot_many_groups(max_groups) : MSMZ_ERR_ARG;
}
void msmz_test_expr_geometry(uint32_t* threads_per_workgroup, uint32_t* register_slots) {
  if (threads_per_workgroup) *threads_per_workgroup = EXPR_THREADS;
  if (register_slots) *register_slots = EXPR_REGISTER_SLOTS;
}
void msmz_test_lookup_geometry(uint32_t* min_slots, uint32_t* threads_per_workgroup) {
  if (min_slots) *min_slots = lk_slots(1);
  if (threads_per_workgroup) *threads_per_workgroup = LK_THREADS;
}
uint32_t msmz_test_lookup_small_table(uint32_t* passes, uint32_t* max_groups) {
  if (passes) *passes = LK_SMALL_PASSES;
  if (max_groups) *max_groups = LK_SMALL_GROUPS;
  return LK_SMALL_TABLE;
}
uint32_t msmz_test_lookup_slot(int curve_id, const uint8_t* le32, uint64_t table_n) {
  if (!le32 || table_n == 0 || table_n > LK_MAX_TABLE) return LK_EMPTY;
  uint32_t w[8];
  memcpy(w, le32, 32);
  auto of = [&](auto fr) {
    using Fr = decltype(fr);
    return words_geq<8>(w, Fr::Q) ? LK_EMPTY : lk_first_slot(w, lk_slots(table_n) - 1);
  };
  switch (curve_id) {
    case MSMZ_BLS12_377_G1: return of(Bls377Fr{});
    case MSMZ_PALLAS: return of(PallasFr{});
    case MSMZ_BLS12_381_G1: return of(Bls381Fr{});
    case MSMZ_ED_ON_BLS12_377: return of(Ed377Fr{});
    default: return LK_EMPTY;
  }
}
void msmz_test_matrix_geometry(uint32_t* tile, uint32_t* run, uint32_t* carries_per_pass) {
  if (tile) *tile = MAT_TILE;
  if (run) *run = MAT_RUN;
  if (carries_per_pass) *carries_per_pass = MAT_FOLD_PASS;
}
void msmz_test_mle_geometry(uint32_t* run, uint32_t* eval_tile, uint32_t* round_tile) {
  if (run) *run = MLE_RUN;
  if (eval_tile) *eval_tile = MLE_TILE;
  if (round_tile) *round_tile = MSC_TILE;
}
void msmz_test_sumcheck_step_geometry(uint32_t* step_tile) {
  if (step_tile) *step_tile = MSC_TILE;
}

// the 2-adicity of a curve's scalar field, or -1; w (nullable): the default 2^log_n-th root of unity, log_n <= that
static int ntt_two_adicity(int curve_id, uint32_t log_n, uint32_t* w) {
  auto of = [&](auto fr) {
    using Fr = decltype(fr);
    if (w && log_n <= (uint32_t)Fr::TWO_ADICITY) fr_root_of_unity<Fr>(w, log_n);
    return (int)Fr::TWO_ADICITY;
  };
  switch (curve_id) {
    case MSMZ_BLS12_377_G1: return of(Bls377Fr{});
    case MSMZ_PALLAS: return of(PallasFr{});
    case MSMZ_BLS12_381_G1: return of(Bls381Fr{});
    case MSMZ_ED_ON_BLS12_377: return of(Ed377Fr{});
    default: return -1;
  }
}
int msmz_scalars_root_of_unity(int curve_id, uint32_t log_n, uint8_t* out_le32) {
  uint32_t w[8];
  const int S = ntt_two_adicity(curve_id, log_n, w);
  if (S < 0 || !out_le32) return MSMZ_ERR_ARG;
  if (log_n > (uint32_t)S) return MSMZ_ERR_UNSUPPORTED;
  memcpy(out_le32, w, 32);
  return MSMZ_OK;
}
int msmz_test_ntt_plan(int curve_id, uint32_t log_n, uint32_t* n_passes, uint32_t* stages) {
  const int S = ntt_two_adicity(curve_id, 0, nullptr);
  if (S < 0 || !n_passes || !stages || log_n > (uint32_t)NTT_MAX_LOG) return MSMZ_ERR_ARG;
  if (log_n > (uint32_t)S) return MSMZ_ERR_UNSUPPORTED;
  const NttPlan p = ntt_plan(log_n);
  *n_passes = p.n_passes;
  for (uint32_t j = 0; j < 8; j++) stages[j] = j < p.n_passes ? p.pass[j].s : 0;
  return MSMZ_OK;
}
void msmz_test_ntt_geometry(uint32_t* pass_log) {
  if (pass_log) *pass_log = NTT_PASS_LOG;
}
void msmz_test_scalar_dot_geometry(uint32_t* tile_elements, uint32_t* partials_per_pass) {
  if (tile_elements) *tile_elements = SDOT_TILE;
  if (partials_per_pass) *partials_per_pass = SDOT_PASS;
}
void msmz_test_scalar_scan_geometry(uint32_t* rec_tile, uint32_t* rec_pass, uint32_t* inv_chunk) {
  if (rec_tile) *rec_tile = SREC_TILE;
  if (rec_pass) *rec_pass = SREC_PASS;
  if (inv_chunk) *inv_chunk = SINV_CHUNK;
}

int msmz_test_fixed_base_plan(int curve_id, uint64_t n, int bits, int32_t* cc, int32_t* K, uint64_t* entries) {
  if (!cc || !K || !entries || n == 0 || bits < 0 || bits > 256) return MSMZ_ERR_ARG;
  auto of = [&](auto cfg) {
    using Cfg = decltype(cfg);
    const FixedPlan p = fixed_base_plan(n, fixed_base_bits(bits, Cfg::Fr::BITS), Cfg::TE, 2 * Cfg::F::NW * 4);
    *cc = p.c;
    *K = p.K;
    *entries = p.entries;
    return (int)MSMZ_OK;
  };
  switch (curve_id) {
    case MSMZ_BLS12_377_G1: return of(CfgBls377{});
    case MSMZ_PALLAS: return of(CfgPallas{});
    case MSMZ_BLS12_381_G1: return of(CfgBls381{});
    case MSMZ_ED_ON_BLS12_377: return of(CfgEd377{});
    default: return MSMZ_ERR_ARG;
  }
}
int msmz_test_set_fixed_base_window(msmz_ctx* c, int cc) { return c ? c->engine->test_set_fixed_base_window(cc) : MSMZ_ERR_ARG; }
int msmz_test_fixed_base_tables(msmz_ctx* c, uint64_t* built) {
  if (!c || !built) return MSMZ_ERR_ARG;
  *built = c->engine->test_fixed_base_tables();
  return MSMZ_OK;
}

int msmz_test_ntt_tables(msmz_ctx* c, uint64_t* built) {
  if (!c || !built) return MSMZ_ERR_ARG;
  *built = c->engine->test_ntt_tables();
  return MSMZ_OK;
}
void msmz_test_cache_geometry(uint32_t* ntt_sets, uint32_t* fixed_tables, uint32_t* ntt_grid_vectors) {
  if (ntt_sets) *ntt_sets = NTT_CACHE;
  if (fixed_tables) *fixed_tables = FIXED_CACHE;
  if (ntt_grid_vectors) *ntt_grid_vectors = NTT_GRID_VECTORS;
}

int msmz_test_set_glv_bits(msmz_ctx* c, int bits) { return c ? c->engine->test_set_glv_bits(bits) : MSMZ_ERR_ARG; }
int msmz_test_retries(msmz_ctx* c) { return c ? c->engine->test_retries() : -1; }
int msmz_test_set_limits(msmz_ctx* c, uint64_t pass_entries, uint64_t batch_entries) {
  return c ? c->engine->test_set_limits(pass_entries, batch_entries) : MSMZ_ERR_ARG;
}
int msmz_test_passes(msmz_ctx* c, uint64_t* range_passes, uint64_t* sub_batches) {
  if (!c) return MSMZ_ERR_ARG;
  c->engine->test_passes(range_passes, sub_batches);
  return MSMZ_OK;
}
int msmz_test_poison(msmz_ctx* c, int pattern, uint64_t* buffers, uint64_t* bytes) {
  if (!c || pattern < -1 || pattern > 255) return MSMZ_ERR_ARG;   // (the outputs stay as they were)
  return c->engine->test_poison(pattern, buffers, bytes);
}
int msmz_test_scratch(msmz_ctx* c, int engine, uint64_t* buffers, uint64_t* bytes) {
  return c ? c->engine->test_scratch(engine, buffers, bytes) : MSMZ_ERR_ARG;
}
int msmz_test_field(msmz_ctx* c, int op, const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out) {
  return c ? c->engine->test_hooks()->test_field(op, a, b, n, out) : MSMZ_ERR_ARG;
}
int msmz_test_field_limbs(msmz_ctx* c, int op, const int32_t* a, const int32_t* b, uint64_t n, int32_t* raw,
                          uint8_t* canon) {
  return c ? c->engine->test_hooks()->test_field_limbs(op, a, b, n, raw, canon) : MSMZ_ERR_ARG;
}
int msmz_test_field_rows(msmz_ctx* c, int op, const int32_t* a, const int32_t* b, uint64_t n, uint32_t live_rows,
                         int32_t* raw, uint8_t* canon) {
  return c ? c->engine->test_hooks()->test_field_rows(op, a, b, n, live_rows, raw, canon) : MSMZ_ERR_ARG;
}
int msmz_test_glv(msmz_ctx* c, const uint8_t* s, uint64_t n, uint8_t* s0, uint8_t* s1, uint8_t* neg) {
  return c ? c->engine->test_hooks()->test_glv(s, n, s0, s1, neg) : MSMZ_ERR_ARG;
}
int msmz_test_digits(msmz_ctx* c, const uint8_t* s, uint64_t n, int cc, int K, int glv, uint32_t* digits) {
  return c ? c->engine->test_hooks()->test_digits(s, n, cc, K, glv, digits) : MSMZ_ERR_ARG;
}
int msmz_test_sort(msmz_ctx* c, const uint8_t* s, uint64_t n, int cc, int glv, int force_fallback, uint32_t* geom,
                   uint32_t* off, uint64_t off_cap, uint32_t* refs, uint64_t refs_cap) {
  if (!c) return MSMZ_ERR_ARG;
  return c->engine->test_hooks()->test_sort(s, n, cc, glv, force_fallback, geom, off, off_cap, refs, refs_cap);
}
int msmz_test_sort_ex(msmz_ctx* c, const msmz_test_sort_args* a) {
  return c && a ? c->engine->test_hooks()->test_sort_ex(*a) : MSMZ_ERR_ARG;
}
int msmz_test_point_raw(msmz_ctx* c, int op, const uint8_t* a, const uint8_t* b, const uint8_t* neg, uint64_t n, int L,
                        uint8_t* out) {
  return c ? c->engine->test_hooks()->test_point_raw(op, a, b, neg, n, L, out) : MSMZ_ERR_ARG;
}
int msmz_test_point(msmz_ctx* c, int op, const uint8_t* a, const uint8_t* ai, const uint8_t* b, const uint8_t* bi,
                    uint64_t n, uint8_t* out) {
  return c ? c->engine->test_hooks()->test_point(op, a, ai, b, bi, n, out) : MSMZ_ERR_ARG;
}

int msmz_test_batch_add(msmz_ctx* c, int safe, int B, const uint8_t* pxy, const uint8_t* pinf, uint64_t np,
                        const uint8_t* sxy, const uint8_t* sinf, uint64_t ns, const uint32_t* desc, uint64_t n_pairs,
                        uint64_t out_base, uint8_t* out, uint32_t* error) {
  if (!c) return MSMZ_ERR_ARG;
  return c->engine->test_hooks()->test_batch_add(safe, B, pxy, pinf, np, sxy, sinf, ns, desc, n_pairs, out_base, out, error);
}

int msmz_test_reduce(msmz_ctx* c, const msmz_test_reduce_args* a) {
  return c && a ? c->engine->test_hooks()->test_reduce(*a) : MSMZ_ERR_ARG;
}

int msmz_test_plan(msmz_ctx* c, const msmz_test_plan_args* a) {
  return c && a ? c->engine->test_hooks()->test_plan(*a) : MSMZ_ERR_ARG;
}

int msmz_point_add(int curve_id, const uint8_t* a, int ai, const uint8_t* b, int bi, uint8_t* out, int* oi) {
  if (!out || !oi || (!a && !ai) || (!b && !bi)) return MSMZ_ERR_ARG;
  switch (curve_id) {
    case MSMZ_BLS12_377_G1: return host_point_add<CfgBls377::P>(a, ai, b, bi, out, oi);
    case MSMZ_PALLAS: return host_point_add<CfgPallas::P>(a, ai, b, bi, out, oi);
    case MSMZ_BLS12_381_G1: return host_point_add<CfgBls381::P>(a, ai, b, bi, out, oi);
    case MSMZ_ED_ON_BLS12_377: return host_point_add<CfgEd377::P>(a, 0, b, 0, out, oi);
    default: return MSMZ_ERR_UNSUPPORTED;
  }
}

}  // extern "C"

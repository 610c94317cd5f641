/* Thin N-API addon over the C ABI of include/msmz.h -- the binding a TypeScript/JavaScript host uses
 * in place of the reference's wasm instance (src/field-msm.ts:42-133 exports + src/parallel.ts).
 * No arithmetic here: every function forwards to libmsmz.so.  N-API version 6 (BigInt) or later.
 *
 * Build: gcc -O2 -shared -fPIC -I/usr/include/node napi/msmz_napi.c -Lmsm_zprize_amd -lmsmz \
 *            -Wl,-rpath,'$ORIGIN/../msm_zprize_amd' -o js/msmz_napi.node
 */
#define NAPI_VERSION 6
#include <node_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/msmz.h"

#define NAPI_CALL(env, call)                                          \
  do {                                                                \
    napi_status s_ = (call);                                          \
    if (s_ != napi_ok) {                                              \
      napi_throw_error((env), NULL, "N-API call failed: " #call);     \
      return NULL;                                                    \
    }                                                                 \
  } while (0)

static napi_value throw_status(napi_env env, int st, const char* where) {
  char msg[256];
  strcpy(msg, where);
  strcat(msg, ": ");
  strncat(msg, msmz_strerror(st), sizeof(msg) - strlen(msg) - 1);
  char code[16];
  int n = 0, v = st;
  char tmp[16];
  do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  for (int i = 0; i < n; i++) code[i] = tmp[n - 1 - i];
  code[n] = 0;
  napi_throw_error(env, code, msg);
  return NULL;
}

static int get_u64(napi_env env, napi_value v, uint64_t* out) {
  napi_valuetype t;
  if (napi_typeof(env, v, &t) != napi_ok) return 0;
  if (t == napi_bigint) {
    bool lossless;
    return napi_get_value_bigint_uint64(env, v, out, &lossless) == napi_ok;
  }
  double d;
  if (napi_get_value_double(env, v, &d) != napi_ok || d < 0) return 0;
  *out = (uint64_t)d;
  return 1;
}

static int get_ctx(napi_env env, napi_value v, msmz_ctx** ctx) {
  void* p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) return 0;
  *ctx = *(msmz_ctx**)p;
  return *ctx != NULL;
}

static void ctx_finalize(napi_env env, void* data, void* hint) {
  (void)env; (void)hint;
  msmz_ctx** slot = (msmz_ctx**)data;
  if (*slot) msmz_destroy(*slot);
  free(slot);
}

/* create(curveId, deviceId | [deviceIds]) -> ctx   (an array = one engine per listed GPU, startThreads(n)) */
static napi_value Create(napi_env env, napi_callback_info info) {
  size_t argc = 2; napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t curve = 0, devs[MSMZ_MAX_DEVICES] = {0};
  uint32_t ndev = 1;
  NAPI_CALL(env, napi_get_value_int32(env, argv[0], &curve));
  if (argc > 1) {
    bool is_arr = false;
    NAPI_CALL(env, napi_is_array(env, argv[1], &is_arr));
    if (is_arr) {
      NAPI_CALL(env, napi_get_array_length(env, argv[1], &ndev));
      if (ndev < 1 || ndev > MSMZ_MAX_DEVICES) return throw_status(env, MSMZ_ERR_ARG, "msmz_create");
      for (uint32_t i = 0; i < ndev; i++) {
        napi_value v;
        NAPI_CALL(env, napi_get_element(env, argv[1], i, &v));
        NAPI_CALL(env, napi_get_value_int32(env, v, &devs[i]));
      }
    } else {
      NAPI_CALL(env, napi_get_value_int32(env, argv[1], &devs[0]));
    }
  }
  msmz_ctx* ctx = NULL;
  int st = msmz_create(&ctx, curve, devs, (int)ndev);
  if (st) return throw_status(env, st, "msmz_create");
  msmz_ctx** slot = (msmz_ctx**)malloc(sizeof(*slot));
  *slot = ctx;
  napi_value ext;
  NAPI_CALL(env, napi_create_external(env, slot, ctx_finalize, NULL, &ext));
  return ext;
}

/* destroy(ctx) */
static napi_value Destroy(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void* p = NULL;
  if (napi_get_value_external(env, argv[0], &p) == napi_ok && p) {
    msmz_ctx** slot = (msmz_ctx**)p;
    if (*slot) msmz_destroy(*slot);
    *slot = NULL;
  }
  return NULL;
}

static napi_value make_handle(napi_env env, uint64_t h) {
  napi_value v;
  napi_create_double(env, (double)h, &v);
  return v;
}

/* uploadPoints(ctx, xyBuffer, infBufferOrNull, n) -> handle */
static napi_value UploadPoints(napi_env env, napi_callback_info info) {
  size_t argc = 4; napi_value argv[4];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (!get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "uploadPoints");
  void* xy; size_t xylen; NAPI_CALL(env, napi_get_buffer_info(env, argv[1], &xy, &xylen));
  void* inf = NULL; size_t inflen = 0; bool isbuf = false;
  napi_is_buffer(env, argv[2], &isbuf);
  if (isbuf) NAPI_CALL(env, napi_get_buffer_info(env, argv[2], &inf, &inflen));
  uint64_t n; if (!get_u64(env, argv[3], &n)) return throw_status(env, MSMZ_ERR_ARG, "uploadPoints");
  {
    int fbc = msmz_ctx_fe_bytes(ctx);   /* buffers must cover n records: 2 * fe_bytes each (+ one flag byte) */
    if (fbc <= 0 || n == 0 || xylen / (2 * (size_t)fbc) < n || (inf != NULL && inflen < n))
      return throw_status(env, MSMZ_ERR_ARG, "uploadPoints");
  }
  uint64_t h = 0;
  int st = msmz_upload_points(ctx, (const uint8_t*)xy, (const uint8_t*)inf, n, &h);
  if (st) return throw_status(env, st, "msmz_upload_points");
  return make_handle(env, h);
}

/* uploadScalars(ctx, buffer, n) -> handle */
static napi_value UploadScalars(napi_env env, napi_callback_info info) {
  size_t argc = 3; napi_value argv[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (!get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "uploadScalars");
  void* s; size_t slen; NAPI_CALL(env, napi_get_buffer_info(env, argv[1], &s, &slen));
  uint64_t n; if (!get_u64(env, argv[2], &n) || slen < 32 * n) return throw_status(env, MSMZ_ERR_ARG, "uploadScalars");
  uint64_t h = 0;
  int st = msmz_upload_scalars(ctx, (const uint8_t*)s, n, &h);
  if (st) return throw_status(env, st, "msmz_upload_scalars");
  return make_handle(env, h);
}

/* importScalars(ctx, buffer, n, width, montgomery) -> handle: host records of `width` bytes, optionally 64-bit-limb
 * Montgomery residues (msmz_import_scalars; N-API has no device pointers, so the host forms only) */
static napi_value ImportScalars(napi_env env, napi_callback_info info) {
  size_t argc = 5; napi_value argv[5];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (argc < 5 || !get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "importScalars");
  void* s; size_t slen; NAPI_CALL(env, napi_get_buffer_info(env, argv[1], &s, &slen));
  uint64_t n, width; bool mont = false;
  if (!get_u64(env, argv[2], &n) || !get_u64(env, argv[3], &width) || napi_get_value_bool(env, argv[4], &mont) != napi_ok ||
      width < 4 || width > 32 || n == 0 || slen / (size_t)width < n)
    return throw_status(env, MSMZ_ERR_ARG, "importScalars");
  msmz_src src = {s, 0, (uint32_t)width, mont ? MSMZ_SRC_MONTGOMERY : 0u, NULL, NULL};
  uint64_t h = 0;
  int st = msmz_import_scalars(ctx, &src, n, &h);
  if (st) return throw_status(env, st, "msmz_import_scalars");
  return make_handle(env, h);
}

/* importPoints(ctx, xyBuffer, infBufferOrNull, n, montgomery) -> handle */
static napi_value ImportPoints(napi_env env, napi_callback_info info) {
  size_t argc = 5; napi_value argv[5];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (argc < 5 || !get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "importPoints");
  void* xy; size_t xylen; NAPI_CALL(env, napi_get_buffer_info(env, argv[1], &xy, &xylen));
  void* inf = NULL; size_t inflen = 0; bool isbuf = false, mont = false;
  napi_is_buffer(env, argv[2], &isbuf);
  if (isbuf) NAPI_CALL(env, napi_get_buffer_info(env, argv[2], &inf, &inflen));
  uint64_t n;
  int fbc = msmz_ctx_fe_bytes(ctx);
  if (!get_u64(env, argv[3], &n) || napi_get_value_bool(env, argv[4], &mont) != napi_ok || fbc <= 0 || n == 0 ||
      xylen / (2 * (size_t)fbc) < n || (inf != NULL && inflen < n))
    return throw_status(env, MSMZ_ERR_ARG, "importPoints");
  msmz_src src = {xy, 0, 0, mont ? MSMZ_SRC_MONTGOMERY : 0u, NULL, (const uint8_t*)inf};
  uint64_t h = 0;
  int st = msmz_import_points(ctx, &src, n, &h);
  if (st) return throw_status(env, st, "msmz_import_points");
  return make_handle(env, h);
}

/* randomPoints(ctx, n, seed) / randomScalars(ctx, n, seed) -> handle */
static napi_value random_common(napi_env env, napi_callback_info info, int scalars) {
  size_t argc = 3; napi_value argv[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (!get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "random");
  uint64_t n, seed;
  if (!get_u64(env, argv[1], &n) || !get_u64(env, argv[2], &seed)) return throw_status(env, MSMZ_ERR_ARG, "random");
  uint64_t h = 0;
  int st = scalars ? msmz_random_scalars(ctx, n, seed, &h) : msmz_random_points(ctx, n, seed, &h);
  if (st) return throw_status(env, st, scalars ? "msmz_random_scalars" : "msmz_random_points");
  return make_handle(env, h);
}
static napi_value RandomPoints(napi_env env, napi_callback_info info) { return random_common(env, info, 0); }
static napi_value RandomScalars(napi_env env, napi_callback_info info) { return random_common(env, info, 1); }

/* downloadPoints(ctx, handle, first, count, feBytes) -> Buffer(xy) ; downloadScalars(ctx, handle, first, count) */
static napi_value DownloadPoints(napi_env env, napi_callback_info info) {
  size_t argc = 5; napi_value argv[5];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (!get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "downloadPoints");
  uint64_t h, first, count, fb;
  if (!get_u64(env, argv[1], &h) || !get_u64(env, argv[2], &first) || !get_u64(env, argv[3], &count) ||
      !get_u64(env, argv[4], &fb))
    return throw_status(env, MSMZ_ERR_ARG, "downloadPoints");
  void* data; napi_value buf;
  NAPI_CALL(env, napi_create_buffer(env, (size_t)(2 * fb * count), &data, &buf));
  int st = msmz_download_points(ctx, h, first, count, (uint8_t*)data, NULL);
  if (st) return throw_status(env, st, "msmz_download_points");
  return buf;
}
static napi_value DownloadScalars(napi_env env, napi_callback_info info) {
  size_t argc = 4; napi_value argv[4];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (!get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "downloadScalars");
  uint64_t h, first, count;
  if (!get_u64(env, argv[1], &h) || !get_u64(env, argv[2], &first) || !get_u64(env, argv[3], &count))
    return throw_status(env, MSMZ_ERR_ARG, "downloadScalars");
  void* data; napi_value buf;
  NAPI_CALL(env, napi_create_buffer(env, (size_t)(32 * count), &data, &buf));
  int st = msmz_download_scalars(ctx, h, first, count, (uint8_t*)data);
  if (st) return throw_status(env, st, "msmz_download_scalars");
  return buf;
}

static napi_value Free(napi_env env, napi_callback_info info) {
  size_t argc = 2; napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (!get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "free");
  uint64_t h; if (!get_u64(env, argv[1], &h)) return throw_status(env, MSMZ_ERR_ARG, "free");
  int st = msmz_free(ctx, h);
  if (st) return throw_status(env, st, "msmz_free");
  return NULL;
}

static int32_t opt_i32(napi_env env, napi_value obj, const char* key) {
  napi_valuetype t;
  if (napi_typeof(env, obj, &t) != napi_ok || t != napi_object) return 0;
  napi_value v; bool has = false;
  if (napi_has_named_property(env, obj, key, &has) != napi_ok || !has) return 0;
  if (napi_get_named_property(env, obj, key, &v) != napi_ok) return 0;
  if (napi_typeof(env, v, &t) != napi_ok) return 0;
  if (t == napi_boolean) { bool b; napi_get_value_bool(env, v, &b); return b ? 1 : 0; }
  int32_t r = 0;
  if (t == napi_number) napi_get_value_int32(env, v, &r);
  return r;
}

static void set_num(napi_env env, napi_value obj, const char* key, double v) {
  napi_value n; napi_create_double(env, v, &n); napi_set_named_property(env, obj, key, n);
}

/* msm(ctx, pointsHandle, scalars (handle number or Buffer), n, feBytes, opts) -> {xy, isInf, log} */
static napi_value Msm(napi_env env, napi_callback_info info) {
  size_t argc = 6; napi_value argv[6];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (!get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "msm");
  uint64_t ph, n, fb;
  if (!get_u64(env, argv[1], &ph) || !get_u64(env, argv[3], &n) || !get_u64(env, argv[4], &fb))
    return throw_status(env, MSMZ_ERR_ARG, "msm");
  msmz_opts o; memset(&o, 0, sizeof(o));
  if (argc > 5) {
    o.c = opt_i32(env, argv[5], "c");
    o.glv = opt_i32(env, argv[5], "glv");
    o.safe = opt_i32(env, argv[5], "safe");
    o.buckets = opt_i32(env, argv[5], "buckets");
    o.timing = opt_i32(env, argv[5], "timing");
    o.reserved[0] = opt_i32(env, argv[5], "reduceAffine");
    o.reserved[1] = opt_i32(env, argv[5], "scalarBits");   /* every scalar < 2^scalarBits; 0 = no bound */
  }
  void* data; napi_value xy;
  NAPI_CALL(env, napi_create_buffer(env, (size_t)(2 * fb), &data, &xy));
  int is_inf = 0; msmz_log log;
  bool isbuf = false; napi_is_buffer(env, argv[2], &isbuf);
  int st;
  if (isbuf) {
    void* s; size_t slen; NAPI_CALL(env, napi_get_buffer_info(env, argv[2], &s, &slen));
    if (slen < 32 * n) return throw_status(env, MSMZ_ERR_ARG, "msm");
    st = msmz_msm(ctx, ph, (const uint8_t*)s, n, &o, (uint8_t*)data, &is_inf, &log);
  } else {
    uint64_t sh; if (!get_u64(env, argv[2], &sh)) return throw_status(env, MSMZ_ERR_ARG, "msm");
    st = msmz_msm_resident(ctx, ph, sh, n, &o, (uint8_t*)data, &is_inf, &log);
  }
  if (st) return throw_status(env, st, "msmz_msm");
  napi_value res, jlog, inf, stages, rounds;
  NAPI_CALL(env, napi_create_object(env, &res));
  NAPI_CALL(env, napi_create_object(env, &jlog));
  napi_get_boolean(env, is_inf != 0, &inf);
  napi_set_named_property(env, res, "xy", xy);
  napi_set_named_property(env, res, "isInf", inf);
  static const char* names[MSMZ_N_STAGES] = {"digits", "scan", "scatter", "plan", "accumulate", "reduce", "final", "total"};
  NAPI_CALL(env, napi_create_object(env, &stages));
  for (int i = 0; i < MSMZ_N_STAGES; i++) set_num(env, stages, names[i], log.stage_ms[i]);
  napi_set_named_property(env, jlog, "stageMs", stages);
  set_num(env, jlog, "c", log.c); set_num(env, jlog, "K", log.K); set_num(env, jlog, "rounds", log.rounds);
  set_num(env, jlog, "glv", log.glv); set_num(env, jlog, "nEntries", (double)log.n_entries);
  set_num(env, jlog, "nPairs", (double)log.n_pairs); set_num(env, jlog, "maxBucket", log.max_bucket);
  set_num(env, jlog, "scatterKernelMs", log.scatter_kernel_ms);
  NAPI_CALL(env, napi_create_array_with_length(env, 32, &rounds));
  for (uint32_t i = 0; i < 32; i++) { napi_value v; napi_create_double(env, log.batch_add_ms[i], &v); napi_set_element(env, rounds, i, v); }
  napi_set_named_property(env, jlog, "batchAddMs", rounds);
  napi_set_named_property(env, res, "log", jlog);
  return res;
}

/* msmBatch(ctx, pointsHandle, scalars (handle number of >= batch * n scalars, or one Buffer of batch vectors), n, batch,
 * feBytes, opts) -> {xy (batch records), isInf (batch flags in a Buffer)} */
static napi_value MsmBatch(napi_env env, napi_callback_info info) {
  size_t argc = 7; napi_value argv[7];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (!get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "msmBatch");
  uint64_t ph, n, batch, fb;
  if (argc < 6 || !get_u64(env, argv[1], &ph) || !get_u64(env, argv[3], &n) || !get_u64(env, argv[4], &batch) ||
      !get_u64(env, argv[5], &fb) || batch == 0 || batch > 0xffffffffu || fb > 64)
    return throw_status(env, MSMZ_ERR_ARG, "msmBatch");
  msmz_opts o; memset(&o, 0, sizeof(o));
  if (argc > 6) {
    o.c = opt_i32(env, argv[6], "c");
    o.glv = opt_i32(env, argv[6], "glv");
    o.safe = opt_i32(env, argv[6], "safe");
    o.buckets = opt_i32(env, argv[6], "buckets");
    o.reserved[0] = opt_i32(env, argv[6], "reduceAffine");
    o.reserved[1] = opt_i32(env, argv[6], "scalarBits");
  }
  void* data; napi_value xy;
  NAPI_CALL(env, napi_create_buffer(env, (size_t)(2 * fb * batch), &data, &xy));
  int* flags = (int*)calloc((size_t)batch, sizeof(int));
  if (!flags) return throw_status(env, MSMZ_ERR_ARG, "msmBatch");
  bool isbuf = false; napi_is_buffer(env, argv[2], &isbuf);
  int st;
  if (isbuf) {
    void* s; size_t slen;
    if (napi_get_buffer_info(env, argv[2], &s, &slen) != napi_ok || n == 0 || slen / 32 / n < batch) {
      free(flags);
      return throw_status(env, MSMZ_ERR_ARG, "msmBatch");
    }
    st = msmz_msm_batch(ctx, ph, (const uint8_t*)s, n, (uint32_t)batch, &o, (uint8_t*)data, flags, NULL);
  } else {
    uint64_t sh;
    if (!get_u64(env, argv[2], &sh)) { free(flags); return throw_status(env, MSMZ_ERR_ARG, "msmBatch"); }
    st = msmz_msm_batch_resident(ctx, ph, sh, n, (uint32_t)batch, &o, (uint8_t*)data, flags, NULL);
  }
  void* fdata = NULL; napi_value inf;
  if (st == 0 && napi_create_buffer(env, (size_t)batch, &fdata, &inf) == napi_ok)
    for (uint64_t k = 0; k < batch; k++) ((uint8_t*)fdata)[k] = flags[k] ? 1 : 0;
  free(flags);
  if (st) return throw_status(env, st, "msmz_msm_batch");
  if (!fdata) return throw_status(env, MSMZ_ERR_ARG, "msmBatch");
  napi_value res;
  NAPI_CALL(env, napi_create_object(env, &res));
  napi_set_named_property(env, res, "xy", xy);
  napi_set_named_property(env, res, "isInf", inf);
  return res;
}

/* msmSegments(ctx, pointsHandle, scalarsHandle, segs (Buffer: per segment firstPoint, firstScalar, n as three
 * little-endian uint64 = msmz_segment), count, feBytes, opts) -> {xy (count records), isInf (count flags in a Buffer)} */
static napi_value MsmSegments(napi_env env, napi_callback_info info) {
  size_t argc = 7; napi_value argv[7];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (!get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "msmSegments");
  uint64_t ph, sh, count, fb;
  if (argc < 6 || !get_u64(env, argv[1], &ph) || !get_u64(env, argv[2], &sh) || !get_u64(env, argv[4], &count) ||
      !get_u64(env, argv[5], &fb) || count == 0 || count > 0xffffffffu || fb > 64)
    return throw_status(env, MSMZ_ERR_ARG, "msmSegments");
  void* sp; size_t slen;
  if (napi_get_buffer_info(env, argv[3], &sp, &slen) != napi_ok || slen / sizeof(msmz_segment) < count)
    return throw_status(env, MSMZ_ERR_ARG, "msmSegments");
  msmz_opts o; memset(&o, 0, sizeof(o));
  if (argc > 6) {
    o.c = opt_i32(env, argv[6], "c");
    o.glv = opt_i32(env, argv[6], "glv");
    o.safe = opt_i32(env, argv[6], "safe");
    o.buckets = opt_i32(env, argv[6], "buckets");
    o.reserved[0] = opt_i32(env, argv[6], "reduceAffine");
    o.reserved[1] = opt_i32(env, argv[6], "scalarBits");
  }
  void* data; napi_value xy;
  NAPI_CALL(env, napi_create_buffer(env, (size_t)(2 * fb * count), &data, &xy));
  int* flags = (int*)calloc((size_t)count, sizeof(int));
  msmz_segment* segs = (msmz_segment*)malloc((size_t)count * sizeof(msmz_segment));   /* (a Buffer need not be aligned) */
  if (!flags || !segs) { free(flags); free(segs); return throw_status(env, MSMZ_ERR_ARG, "msmSegments"); }
  memcpy(segs, sp, (size_t)count * sizeof(msmz_segment));
  const int st = msmz_msm_segments(ctx, ph, sh, segs, (uint32_t)count, &o, (uint8_t*)data, flags, NULL);
  free(segs);
  void* fdata = NULL; napi_value inf;
  if (st == 0 && napi_create_buffer(env, (size_t)count, &fdata, &inf) == napi_ok)
    for (uint64_t k = 0; k < count; k++) ((uint8_t*)fdata)[k] = flags[k] ? 1 : 0;
  free(flags);
  if (st) return throw_status(env, st, "msmz_msm_segments");
  if (!fdata) return throw_status(env, MSMZ_ERR_ARG, "msmSegments");
  napi_value res;
  NAPI_CALL(env, napi_create_object(env, &res));
  napi_set_named_property(env, res, "xy", xy);
  napi_set_named_property(env, res, "isInf", inf);
  return res;
}

/* pointAdd(curveId, aXy|null, bXy|null, feBytes) -> {xy, isInf}  (null = infinity) */
/* precomputePoints(ctx, pointsHandle, n, {c, glv, scalarBits}, factor) -> handle of a precomputed point set (msmz_precompute_points;
   glv -1 = the engine's choice, factor 0 = all windows in one bucket set) */
static napi_value PrecomputePoints(napi_env env, napi_callback_info info) {
  size_t argc = 5; napi_value argv[5];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (argc < 5 || !get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "precomputePoints");
  uint64_t ph, n, factor;
  if (!get_u64(env, argv[1], &ph) || !get_u64(env, argv[2], &n) || !get_u64(env, argv[4], &factor) || factor > 0xffffffffu)
    return throw_status(env, MSMZ_ERR_ARG, "precomputePoints");
  msmz_opts o; memset(&o, 0, sizeof(o));
  o.c = opt_i32(env, argv[3], "c");
  o.glv = opt_i32(env, argv[3], "glv");
  o.reserved[1] = opt_i32(env, argv[3], "scalarBits");
  uint64_t h = 0;
  int st = msmz_precompute_points(ctx, ph, n, &o, (uint32_t)factor, &h);
  if (st) return throw_status(env, st, "msmz_precompute_points");
  return make_handle(env, h);
}

/* precomputedInfo(ctx, handle) -> {c, glv, factor, K, records, scalarBits} (msmz_precomputed_info,
   msmz_precomputed_scalar_bits) */
static napi_value PrecomputedInfo(napi_env env, napi_callback_info info) {
  size_t argc = 2; napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (argc < 2 || !get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "precomputedInfo");
  uint64_t h; if (!get_u64(env, argv[1], &h)) return throw_status(env, MSMZ_ERR_ARG, "precomputedInfo");
  int32_t c = 0, glv = 0; uint32_t factor = 0, K = 0; uint64_t records = 0;
  int st = msmz_precomputed_info(ctx, h, &c, &glv, &factor, &K, &records);
  if (st) return throw_status(env, st, "msmz_precomputed_info");
  int32_t sbits = 0;
  st = msmz_precomputed_scalar_bits(ctx, h, &sbits);
  if (st) return throw_status(env, st, "msmz_precomputed_scalar_bits");
  napi_value res;
  NAPI_CALL(env, napi_create_object(env, &res));
  set_num(env, res, "c", c); set_num(env, res, "glv", glv); set_num(env, res, "factor", factor);
  set_num(env, res, "K", K); set_num(env, res, "records", (double)records); set_num(env, res, "scalarBits", sbits);
  return res;
}

/* checkPoints(ctx, pointsHandle, first, count, what, wantVerdicts) -> {offCurve, offSubgroup, firstBad, verdicts}
   (msmz_check_points; what: 1 = curve, 3 = curve + subgroup; firstBad -1 = none; verdicts: Buffer or null) */
static napi_value CheckPoints(napi_env env, napi_callback_info info) {
  size_t argc = 6; napi_value argv[6];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (argc < 6 || !get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "checkPoints");
  uint64_t h, first, count, what;
  if (!get_u64(env, argv[1], &h) || !get_u64(env, argv[2], &first) || !get_u64(env, argv[3], &count) ||
      !get_u64(env, argv[4], &what) || what > 0xffffffffu || count > 0xffffffffu)
    return throw_status(env, MSMZ_ERR_ARG, "checkPoints");
  bool want = false;
  NAPI_CALL(env, napi_get_value_bool(env, argv[5], &want));
  void* data = NULL; napi_value buf;
  if (want) NAPI_CALL(env, napi_create_buffer(env, (size_t)count, &data, &buf));
  else NAPI_CALL(env, napi_get_null(env, &buf));
  msmz_check_result r;
  int st = msmz_check_points(ctx, h, first, count, (uint32_t)what, &r, (uint8_t*)data);
  if (st) return throw_status(env, st, "msmz_check_points");
  napi_value res;
  NAPI_CALL(env, napi_create_object(env, &res));
  set_num(env, res, "offCurve", (double)r.off_curve); set_num(env, res, "offSubgroup", (double)r.off_subgroup);
  set_num(env, res, "firstBad", r.first_bad == UINT64_MAX ? -1.0 : (double)r.first_bad);
  NAPI_CALL(env, napi_set_named_property(env, res, "verdicts", buf));
  return res;
}

/* mulPoints(ctx, pointsHandle, firstPoint, scalarsHandle | 32-byte Buffer, firstScalar, addendHandle (0 = none),
   firstAddend, n) -> handle of a new point set, record i = [s_i] P_i (+ Q_i)  (msmz_points_mul; a Buffer is the one
   scalar, little-endian, for every point) */
static napi_value MulPoints(napi_env env, napi_callback_info info) {
  size_t argc = 8; napi_value argv[8];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (argc < 8 || !get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "mulPoints");
  msmz_mul m; memset(&m, 0, sizeof(m));
  uint64_t n;
  if (!get_u64(env, argv[1], &m.points_handle) || !get_u64(env, argv[2], &m.first_p) || !get_u64(env, argv[4], &m.first_s) ||
      !get_u64(env, argv[5], &m.addend_handle) || !get_u64(env, argv[6], &m.first_q) || !get_u64(env, argv[7], &n))
    return throw_status(env, MSMZ_ERR_ARG, "mulPoints");
  bool isbuf = false; napi_is_buffer(env, argv[3], &isbuf);
  if (isbuf) {
    void* s; size_t slen;
    if (napi_get_buffer_info(env, argv[3], &s, &slen) != napi_ok || slen != 32) return throw_status(env, MSMZ_ERR_ARG, "mulPoints");
    m.scalar = (const uint8_t*)s;
  } else if (!get_u64(env, argv[3], &m.scalars_handle) || m.scalars_handle == 0) {
    return throw_status(env, MSMZ_ERR_ARG, "mulPoints");
  }
  uint64_t h = 0;
  int st = msmz_points_mul(ctx, &m, n, &h);
  if (st) return throw_status(env, st, "msmz_points_mul");
  return make_handle(env, h);
}

/* a coefficient argument of scalarsCombine: a 32-byte Buffer (one scalar for every entry, little-endian), null (1), or
   the handle of a resident scalar array */
static int get_coeff(napi_env env, napi_value v, msmz_scalar_term* t) {
  bool isbuf = false; napi_is_buffer(env, v, &isbuf);
  if (isbuf) {
    void* s; size_t slen;
    if (napi_get_buffer_info(env, v, &s, &slen) != napi_ok || slen != 32) return 0;
    t->coeff = (const uint8_t*)s;
    return 1;
  }
  napi_valuetype ty;
  if (napi_typeof(env, v, &ty) != napi_ok) return 0;
  if (ty == napi_null || ty == napi_undefined) return 1;
  return get_u64(env, v, &t->coeff_handle) && t->coeff_handle != 0;
}

/* scalarsCombine(ctx, xHandle, xFirst, xCoeff, xCoeffFirst, yHandle (0 = no second term), yFirst, yCoeff, yCoeffFirst, n,
   firstOut, outHandle (0 = a new array)) -> handle of the array written: entry i = xCoeff_i x_i (+ yCoeff_i y_i)
   (msmz_scalars_combine) */
static napi_value ScalarsCombine(napi_env env, napi_callback_info info) {
  size_t argc = 12; napi_value argv[12];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (argc < 12 || !get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "scalarsCombine");
  msmz_scalar_term x, y; memset(&x, 0, sizeof(x)); memset(&y, 0, sizeof(y));
  uint64_t n, first_out, h = 0;
  if (!get_u64(env, argv[1], &x.handle) || !get_u64(env, argv[2], &x.first) || !get_coeff(env, argv[3], &x) ||
      !get_u64(env, argv[4], &x.coeff_first) || !get_u64(env, argv[5], &y.handle) || !get_u64(env, argv[6], &y.first) ||
      !get_coeff(env, argv[7], &y) || !get_u64(env, argv[8], &y.coeff_first) || !get_u64(env, argv[9], &n) ||
      !get_u64(env, argv[10], &first_out) || !get_u64(env, argv[11], &h))
    return throw_status(env, MSMZ_ERR_ARG, "scalarsCombine");
  int st = msmz_scalars_combine(ctx, &x, y.handle ? &y : NULL, n, first_out, &h);
  if (st) return throw_status(env, st, "msmz_scalars_combine");
  return make_handle(env, h);
}

/* scalarsDot(ctx, xHandle, xFirst, yHandle (0 = the plain sum of x), yFirst, n) -> 32-byte Buffer, little-endian
   (msmz_scalars_dot) */
static napi_value ScalarsDot(napi_env env, napi_callback_info info) {
  size_t argc = 6; napi_value argv[6];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (argc < 6 || !get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "scalarsDot");
  uint64_t xh, fx, yh, fy, n;
  if (!get_u64(env, argv[1], &xh) || !get_u64(env, argv[2], &fx) || !get_u64(env, argv[3], &yh) || !get_u64(env, argv[4], &fy) ||
      !get_u64(env, argv[5], &n))
    return throw_status(env, MSMZ_ERR_ARG, "scalarsDot");
  void* data; napi_value buf;
  NAPI_CALL(env, napi_create_buffer(env, 32, &data, &buf));
  int st = msmz_scalars_dot(ctx, xh, fx, yh, fy, n, (uint8_t*)data);
  if (st) return throw_status(env, st, "msmz_scalars_dot");
  return buf;
}

/* scalarsPowers(ctx, base (32-byte Buffer or null = 1), ratio (32-byte Buffer), n) -> handle of a new scalar array, entry
   i = base ratio^i (msmz_scalars_powers) */
static napi_value ScalarsPowers(napi_env env, napi_callback_info info) {
  size_t argc = 4; napi_value argv[4];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (argc < 4 || !get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "scalarsPowers");
  msmz_scalar_term base, ratio; memset(&base, 0, sizeof(base)); memset(&ratio, 0, sizeof(ratio));
  uint64_t n, h = 0;
  if (!get_coeff(env, argv[1], &base) || base.coeff_handle || !get_coeff(env, argv[2], &ratio) || !ratio.coeff ||
      !get_u64(env, argv[3], &n))
    return throw_status(env, MSMZ_ERR_ARG, "scalarsPowers");
  int st = msmz_scalars_powers(ctx, base.coeff, ratio.coeff, n, &h);
  if (st) return throw_status(env, st, "msmz_scalars_powers");
  return make_handle(env, h);
}

/* a 32-byte Buffer (a scalar, little-endian) -> *out, null / undefined -> NULL */
static int get_scalar_or_null(napi_env env, napi_value v, const uint8_t** out) {
  msmz_scalar_term t; memset(&t, 0, sizeof(t));
  if (!get_coeff(env, v, &t) || t.coeff_handle) return 0;
  *out = t.coeff;
  return 1;
}

/* scalarsRecurrence(ctx, a (handle, 32-byte Buffer = one multiplier for every entry, or null = 1), aFirst, bHandle (0 = no
   addend), bFirst, init (32-byte Buffer or null), flags (1 = reverse, 2 = exclusive), n, firstOut, outHandle (0 = a new
   array)) -> {handle, last}: the array written and the final value as a 32-byte Buffer  (msmz_scalars_recurrence) */
static napi_value ScalarsRecurrence(napi_env env, napi_callback_info info) {
  size_t argc = 10; napi_value argv[10];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (argc < 10 || !get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "scalarsRecurrence");
  msmz_scalar_rec r; memset(&r, 0, sizeof(r));
  msmz_scalar_term a; memset(&a, 0, sizeof(a));
  uint64_t flags, n, first_out, h = 0;
  if (!get_coeff(env, argv[1], &a) || !get_u64(env, argv[2], &r.a_first) || !get_u64(env, argv[3], &r.b_handle) ||
      !get_u64(env, argv[4], &r.b_first) || !get_scalar_or_null(env, argv[5], &r.init) || !get_u64(env, argv[6], &flags) ||
      flags >> 32 || !get_u64(env, argv[7], &n) || !get_u64(env, argv[8], &first_out) || !get_u64(env, argv[9], &h))
    return throw_status(env, MSMZ_ERR_ARG, "scalarsRecurrence");
  r.a_handle = a.coeff_handle;
  r.a = a.coeff;
  r.flags = (uint32_t)flags;
  void* data; napi_value last, res;
  NAPI_CALL(env, napi_create_buffer(env, 32, &data, &last));
  int st = msmz_scalars_recurrence(ctx, &r, n, first_out, &h, (uint8_t*)data);
  if (st) return throw_status(env, st, "msmz_scalars_recurrence");
  NAPI_CALL(env, napi_create_object(env, &res));
  NAPI_CALL(env, napi_set_named_property(env, res, "handle", make_handle(env, h)));
  NAPI_CALL(env, napi_set_named_property(env, res, "last", last));
  return res;
}

/* scalarsInverse(ctx, handle, first, n, firstOut, outHandle (0 = a new array)) -> {handle, zeros}: the array written,
   entry i = x_i^-1 (0 -> 0), and the number of zero entries  (msmz_scalars_inverse) */
static napi_value ScalarsInverse(napi_env env, napi_callback_info info) {
  size_t argc = 6; napi_value argv[6];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  msmz_ctx* ctx; if (argc < 6 || !get_ctx(env, argv[0], &ctx)) return throw_status(env, MSMZ_ERR_ARG, "scalarsInverse");
  uint64_t xh, first, n, first_out, h = 0, zeros = 0;
  if (!get_u64(env, argv[1], &xh) || !get_u64(env, argv[2], &first) || !get_u64(env, argv[3], &n) ||
      !get_u64(env, argv[4], &first_out) || !get_u64(env, argv[5], &h))
    return throw_status(env, MSMZ_ERR_ARG, "scalarsInverse");
  int st = msmz_scalars_inverse(ctx, xh, first, n, first_out, &h, &zeros);
  if (st) return throw_status(env, st, "msmz_scalars_inverse");
  napi_value res, z;
  NAPI_CALL(env, napi_create_object(env, &res));
  NAPI_CALL(env, napi_create_double(env, (double)zeros, &z));
  NAPI_CALL(env, napi_set_named_property(env, res, "handle", make_handle(env, h)));
  NAPI_CALL(env, napi_set_named_property(env, res, "zeros", z));
  return res;
}

static napi_value PointAdd(napi_env env, napi_callback_info info) {
  size_t argc = 4; napi_value argv[4];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t curve; NAPI_CALL(env, napi_get_value_int32(env, argv[0], &curve));
  uint64_t fb; if (!get_u64(env, argv[3], &fb)) return throw_status(env, MSMZ_ERR_ARG, "pointAdd");
  void *a = NULL, *b = NULL; size_t la, lb; bool ia = false, ib = false;
  napi_is_buffer(env, argv[1], &ia); napi_is_buffer(env, argv[2], &ib);
  if (ia) NAPI_CALL(env, napi_get_buffer_info(env, argv[1], &a, &la));
  if (ib) NAPI_CALL(env, napi_get_buffer_info(env, argv[2], &b, &lb));
  void* data; napi_value xy;
  NAPI_CALL(env, napi_create_buffer(env, (size_t)(2 * fb), &data, &xy));
  int is_inf = 0;
  int st = msmz_point_add(curve, (const uint8_t*)a, a == NULL, (const uint8_t*)b, b == NULL, (uint8_t*)data, &is_inf);
  if (st) return throw_status(env, st, "msmz_point_add");
  napi_value res, inf;
  NAPI_CALL(env, napi_create_object(env, &res));
  napi_get_boolean(env, is_inf != 0, &inf);
  napi_set_named_property(env, res, "xy", xy);
  napi_set_named_property(env, res, "isInf", inf);
  return res;
}

static napi_value FeBytes(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t curve; NAPI_CALL(env, napi_get_value_int32(env, argv[0], &curve));
  napi_value v; napi_create_int32(env, msmz_curve_fe_bytes(curve), &v);
  return v;
}

static napi_value Init(napi_env env, napi_value exports) {
  static const struct { const char* name; napi_callback fn; } fns[] = {
      {"create", Create}, {"destroy", Destroy}, {"uploadPoints", UploadPoints}, {"uploadScalars", UploadScalars},
      {"importScalars", ImportScalars}, {"importPoints", ImportPoints},
      {"randomPoints", RandomPoints}, {"randomScalars", RandomScalars}, {"downloadPoints", DownloadPoints},
      {"downloadScalars", DownloadScalars}, {"free", Free}, {"msm", Msm}, {"msmBatch", MsmBatch}, {"msmSegments", MsmSegments},
      {"precomputePoints", PrecomputePoints}, {"precomputedInfo", PrecomputedInfo}, {"checkPoints", CheckPoints},
      {"mulPoints", MulPoints}, {"scalarsCombine", ScalarsCombine}, {"scalarsDot", ScalarsDot},
      {"scalarsPowers", ScalarsPowers}, {"scalarsRecurrence", ScalarsRecurrence}, {"scalarsInverse", ScalarsInverse},
      {"pointAdd", PointAdd}, {"feBytes", FeBytes}};
  for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); i++) {
    napi_value f;
    if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
    napi_set_named_property(env, exports, fns[i].name, f);
  }
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)

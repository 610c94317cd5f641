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
#include <stdio.h>
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
  char msg[256], code[16];
  snprintf(msg, sizeof(msg), "%s: %s", where, msmz_strerror(st));
  snprintf(code, sizeof(code), "%d", st);
  napi_throw_error(env, code, msg);
  return NULL;
}
#define BAD_ARG(env, where) throw_status((env), MSMZ_ERR_ARG, (where))

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

/* The arguments of a call into argv[MAX_ARGS] (those not passed read as undefined): at least `need` of them, and, with
   `ctx`, the context in the first.  0: a short list or no context -- the caller refuses. */
#define MAX_ARGS 12
static int get_args(napi_env env, napi_callback_info info, size_t need, napi_value* argv, msmz_ctx** ctx) {
  size_t argc = MAX_ARGS;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < need) return 0;
  return ctx == NULL || get_ctx(env, argv[0], ctx);
}

/* A Buffer -> 1 and its (*data, *len); anything else -> 0 and (NULL, 0): an optional Buffer argument. */
static int opt_buffer(napi_env env, napi_value v, void** data, size_t* len) {
  bool isbuf = false;
  *data = NULL; *len = 0;
  return napi_is_buffer(env, v, &isbuf) == napi_ok && isbuf && napi_get_buffer_info(env, v, data, len) == napi_ok;
}

/* A 32-byte Buffer (a scalar, little-endian) -> *out; null / undefined -> NULL.  0 for anything else. */
static int scalar_or_null(napi_env env, napi_value v, const uint8_t** out) {
  void* p; size_t len; napi_valuetype t;
  *out = NULL;
  if (opt_buffer(env, v, &p, &len)) { *out = (const uint8_t*)p; return len == 32; }
  return napi_typeof(env, v, &t) == napi_ok && (t == napi_null || t == napi_undefined);
}

/* ... or the handle of a resident scalar array: the coefficient of scalarsCombine, the multiplier of scalarsRecurrence,
   the scalars of mulPoints */
static int scalar_or_handle(napi_env env, napi_value v, const uint8_t** scalar, uint64_t* handle) {
  return scalar_or_null(env, v, scalar) || (get_u64(env, v, handle) && *handle != 0);
}

/* The feBytes a caller passes is the library's for this context / curve, or the call is refused: the Buffers a point goes
   into are sized from the library's number, the one the C ABI writes by. */
static int is_fe_bytes(napi_env env, napi_value v, int fe) {
  uint64_t fb;
  return fe > 0 && get_u64(env, v, &fb) && fb == (uint64_t)fe;
}

static void ctx_finalize(napi_env env, void* data, void* hint) {
  (void)env; (void)hint;
  msmz_ctx** slot = (msmz_ctx**)data;
  if (*slot) msmz_destroy(*slot);
  free(slot);
}

/* create(curveId, deviceId | [deviceIds]) -> ctx   (an array = one engine per listed GPU, startThreads(n)) */
static napi_value Create(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS];
  if (!get_args(env, info, 1, argv, NULL)) return BAD_ARG(env, "msmz_create");
  int32_t curve = 0, devs[MSMZ_MAX_DEVICES] = {0};
  uint32_t ndev = 1;
  NAPI_CALL(env, napi_get_value_int32(env, argv[0], &curve));
  bool is_arr = false;
  NAPI_CALL(env, napi_is_array(env, argv[1], &is_arr));
  if (is_arr) {
    NAPI_CALL(env, napi_get_array_length(env, argv[1], &ndev));
    if (ndev < 1 || ndev > MSMZ_MAX_DEVICES) return BAD_ARG(env, "msmz_create");
    for (uint32_t i = 0; i < ndev; i++) {
      napi_value v;
      NAPI_CALL(env, napi_get_element(env, argv[1], i, &v));
      NAPI_CALL(env, napi_get_value_int32(env, v, &devs[i]));
    }
  } else {
    napi_valuetype t;
    NAPI_CALL(env, napi_typeof(env, argv[1], &t));
    if (t != napi_undefined) NAPI_CALL(env, napi_get_value_int32(env, argv[1], &devs[0]));
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
  napi_value argv[MAX_ARGS];
  void* p = NULL;
  if (get_args(env, info, 1, argv, NULL) && napi_get_value_external(env, argv[0], &p) == napi_ok && p) {
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

/* n point records (2 * fe_bytes each) and, if given, n infinity flags are in the Buffers? */
static int covers_points(msmz_ctx* ctx, uint64_t n, size_t xylen, const void* inf, size_t inflen) {
  const int fe = msmz_ctx_fe_bytes(ctx);
  return fe > 0 && n != 0 && xylen / (2 * (size_t)fe) >= n && (inf == NULL || inflen >= n);
}

/* uploadPoints(ctx, xyBuffer, infBufferOrNull, n) -> handle */
static napi_value UploadPoints(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  if (!get_args(env, info, 4, argv, &ctx)) return BAD_ARG(env, "uploadPoints");
  void *xy, *inf; size_t xylen, inflen; uint64_t n, h = 0;
  NAPI_CALL(env, napi_get_buffer_info(env, argv[1], &xy, &xylen));
  opt_buffer(env, argv[2], &inf, &inflen);
  if (!get_u64(env, argv[3], &n) || !covers_points(ctx, n, xylen, inf, inflen)) return BAD_ARG(env, "uploadPoints");
  int st = msmz_upload_points(ctx, (const uint8_t*)xy, (const uint8_t*)inf, n, &h);
  if (st) return throw_status(env, st, "msmz_upload_points");
  return make_handle(env, h);
}

/* uploadScalars(ctx, buffer, n) -> handle */
static napi_value UploadScalars(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  if (!get_args(env, info, 3, argv, &ctx)) return BAD_ARG(env, "uploadScalars");
  void* s; size_t slen; uint64_t n, h = 0;
  NAPI_CALL(env, napi_get_buffer_info(env, argv[1], &s, &slen));
  if (!get_u64(env, argv[2], &n) || slen < 32 * n) return BAD_ARG(env, "uploadScalars");
  int st = msmz_upload_scalars(ctx, (const uint8_t*)s, n, &h);
  if (st) return throw_status(env, st, "msmz_upload_scalars");
  return make_handle(env, h);
}

/* importScalars(ctx, buffer, n, width, montgomery) -> handle: host records of `width` bytes, optionally 64-bit-limb
 * Montgomery residues (msmz_import_scalars; N-API has no device pointers, so the host forms only) */
static napi_value ImportScalars(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  if (!get_args(env, info, 5, argv, &ctx)) return BAD_ARG(env, "importScalars");
  void* s; size_t slen; NAPI_CALL(env, napi_get_buffer_info(env, argv[1], &s, &slen));
  uint64_t n, width, h = 0; bool mont = false;
  if (!get_u64(env, argv[2], &n) || !get_u64(env, argv[3], &width) || napi_get_value_bool(env, argv[4], &mont) != napi_ok ||
      width < 4 || width > 32 || n == 0 || slen / (size_t)width < n)
    return BAD_ARG(env, "importScalars");
  msmz_src src = {s, 0, (uint32_t)width, mont ? MSMZ_SRC_MONTGOMERY : 0u, NULL, NULL};
  int st = msmz_import_scalars(ctx, &src, n, &h);
  if (st) return throw_status(env, st, "msmz_import_scalars");
  return make_handle(env, h);
}

/* importPoints(ctx, xyBuffer, infBufferOrNull, n, montgomery) -> handle */
static napi_value ImportPoints(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  if (!get_args(env, info, 5, argv, &ctx)) return BAD_ARG(env, "importPoints");
  void *xy, *inf; size_t xylen, inflen; uint64_t n, h = 0; bool mont = false;
  NAPI_CALL(env, napi_get_buffer_info(env, argv[1], &xy, &xylen));
  opt_buffer(env, argv[2], &inf, &inflen);
  if (!get_u64(env, argv[3], &n) || napi_get_value_bool(env, argv[4], &mont) != napi_ok ||
      !covers_points(ctx, n, xylen, inf, inflen))
    return BAD_ARG(env, "importPoints");
  msmz_src src = {xy, 0, 0, mont ? MSMZ_SRC_MONTGOMERY : 0u, NULL, (const uint8_t*)inf};
  int st = msmz_import_points(ctx, &src, n, &h);
  if (st) return throw_status(env, st, "msmz_import_points");
  return make_handle(env, h);
}

/* importPointsCompressed(ctx, buffer, infBufferOrNull, n, parity) -> handle: n records of fe_bytes, one coordinate with
 * the sign of the other in bit 7 of the last byte (msmz_import_points with MSMZ_SRC_COMPRESSED); parity: the sign bit
 * means "odd", not "the larger root" */
static napi_value ImportPointsCompressed(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  if (!get_args(env, info, 5, argv, &ctx)) return BAD_ARG(env, "importPointsCompressed");
  void *rec, *inf; size_t reclen, inflen; uint64_t n, h = 0; bool parity = false;
  const int fe = msmz_ctx_fe_bytes(ctx);
  if (!opt_buffer(env, argv[1], &rec, &reclen)) return BAD_ARG(env, "importPointsCompressed");
  opt_buffer(env, argv[2], &inf, &inflen);
  if (!get_u64(env, argv[3], &n) || napi_get_value_bool(env, argv[4], &parity) != napi_ok || fe <= 0 || n == 0 ||
      reclen / (size_t)fe < n || (inf != NULL && inflen < n))
    return BAD_ARG(env, "importPointsCompressed");
  msmz_src src = {rec, 0, (uint32_t)fe, MSMZ_SRC_COMPRESSED | (parity ? MSMZ_SRC_SIGN_PARITY : 0u), NULL, (const uint8_t*)inf};
  int st = msmz_import_points(ctx, &src, n, &h);
  if (st) return throw_status(env, st, "msmz_import_points");
  return make_handle(env, h);
}

/* randomPoints(ctx, n, seed) / randomScalars(ctx, n, seed) -> handle */
static napi_value random_common(napi_env env, napi_callback_info info, int scalars) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t n, seed, h = 0;
  if (!get_args(env, info, 3, argv, &ctx) || !get_u64(env, argv[1], &n) || !get_u64(env, argv[2], &seed))
    return BAD_ARG(env, "random");
  int st = scalars ? msmz_random_scalars(ctx, n, seed, &h) : msmz_random_points(ctx, n, seed, &h);
  if (st) return throw_status(env, st, scalars ? "msmz_random_scalars" : "msmz_random_points");
  return make_handle(env, h);
}
static napi_value RandomPoints(napi_env env, napi_callback_info info) { return random_common(env, info, 0); }
static napi_value RandomScalars(napi_env env, napi_callback_info info) { return random_common(env, info, 1); }

/* downloadPoints(ctx, handle, first, count, feBytes) -> Buffer(xy) ; downloadScalars(ctx, handle, first, count) */
static napi_value DownloadPoints(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t h, first, count;
  if (!get_args(env, info, 5, argv, &ctx) || !get_u64(env, argv[1], &h) || !get_u64(env, argv[2], &first) ||
      !get_u64(env, argv[3], &count) || !is_fe_bytes(env, argv[4], msmz_ctx_fe_bytes(ctx)))
    return BAD_ARG(env, "downloadPoints");
  void* data; napi_value buf;
  NAPI_CALL(env, napi_create_buffer(env, 2 * (size_t)msmz_ctx_fe_bytes(ctx) * (size_t)count, &data, &buf));
  int st = msmz_download_points(ctx, h, first, count, (uint8_t*)data, NULL);
  if (st) return throw_status(env, st, "msmz_download_points");
  return buf;
}
/* downloadPointsCompressed(ctx, handle, first, count, feBytes, parity) -> {records: Buffer(count * feBytes), isInf: Buffer(count)} */
static napi_value DownloadPointsCompressed(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t h, first, count; bool parity = false;
  if (!get_args(env, info, 6, argv, &ctx) || !get_u64(env, argv[1], &h) || !get_u64(env, argv[2], &first) ||
      !get_u64(env, argv[3], &count) || !is_fe_bytes(env, argv[4], msmz_ctx_fe_bytes(ctx)) ||
      napi_get_value_bool(env, argv[5], &parity) != napi_ok)
    return BAD_ARG(env, "downloadPointsCompressed");
  void *data, *flags; napi_value rec, inf, out;
  NAPI_CALL(env, napi_create_buffer(env, (size_t)msmz_ctx_fe_bytes(ctx) * (size_t)count, &data, &rec));
  NAPI_CALL(env, napi_create_buffer(env, (size_t)count, &flags, &inf));
  int st = msmz_download_points_compressed(ctx, h, first, count, (uint8_t*)data, (uint8_t*)flags, parity ? MSMZ_SRC_SIGN_PARITY : 0u);
  if (st) return throw_status(env, st, "msmz_download_points_compressed");
  NAPI_CALL(env, napi_create_object(env, &out));
  NAPI_CALL(env, napi_set_named_property(env, out, "records", rec));
  NAPI_CALL(env, napi_set_named_property(env, out, "isInf", inf));
  return out;
}
static napi_value DownloadScalars(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t h, first, count;
  if (!get_args(env, info, 4, argv, &ctx) || !get_u64(env, argv[1], &h) || !get_u64(env, argv[2], &first) ||
      !get_u64(env, argv[3], &count))
    return BAD_ARG(env, "downloadScalars");
  void* data; napi_value buf;
  NAPI_CALL(env, napi_create_buffer(env, (size_t)(32 * count), &data, &buf));
  int st = msmz_download_scalars(ctx, h, first, count, (uint8_t*)data);
  if (st) return throw_status(env, st, "msmz_download_scalars");
  return buf;
}

/* exportScalars(ctx, handle, first, count, width, montgomery) -> Buffer(count * width): msmz_export_scalars on the host
 * route (N-API has no device pointers); a scalar that does not fit `width` bytes is MSMZ_ERR_RANGE */
static napi_value ExportScalars(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t h, first, count, width; bool mont = false;
  if (!get_args(env, info, 6, argv, &ctx) || !get_u64(env, argv[1], &h) || !get_u64(env, argv[2], &first) ||
      !get_u64(env, argv[3], &count) || !get_u64(env, argv[4], &width) || napi_get_value_bool(env, argv[5], &mont) != napi_ok ||
      width < 4 || width > 32 || count == 0 || count >> 32)
    return BAD_ARG(env, "exportScalars");
  void* data; napi_value buf;
  NAPI_CALL(env, napi_create_buffer(env, (size_t)width * (size_t)count, &data, &buf));
  msmz_dst dst = {data, 0, (uint32_t)width, mont ? MSMZ_SRC_MONTGOMERY : 0u, NULL, NULL};
  int st = msmz_export_scalars(ctx, h, first, count, &dst);
  if (st) return throw_status(env, st, "msmz_export_scalars");
  return buf;
}

/* exportPoints(ctx, handle, first, count, feBytes, montgomery) -> {records: Buffer(count * 2 * feBytes), isInf: Buffer(count)}:
 * msmz_export_points on the host route, x || y canonical or as 64-bit-limb Montgomery residues */
static napi_value ExportPoints(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t h, first, count; bool mont = false;
  if (!get_args(env, info, 6, argv, &ctx) || !get_u64(env, argv[1], &h) || !get_u64(env, argv[2], &first) ||
      !get_u64(env, argv[3], &count) || !is_fe_bytes(env, argv[4], msmz_ctx_fe_bytes(ctx)) ||
      napi_get_value_bool(env, argv[5], &mont) != napi_ok || count == 0 || count >> 31)
    return BAD_ARG(env, "exportPoints");
  void *data, *flags; napi_value rec, inf, out;
  NAPI_CALL(env, napi_create_buffer(env, 2 * (size_t)msmz_ctx_fe_bytes(ctx) * (size_t)count, &data, &rec));
  NAPI_CALL(env, napi_create_buffer(env, (size_t)count, &flags, &inf));
  msmz_dst dst = {data, 0, 0, mont ? MSMZ_SRC_MONTGOMERY : 0u, NULL, (uint8_t*)flags};
  int st = msmz_export_points(ctx, h, first, count, &dst);
  if (st) return throw_status(env, st, "msmz_export_points");
  NAPI_CALL(env, napi_create_object(env, &out));
  NAPI_CALL(env, napi_set_named_property(env, out, "records", rec));
  NAPI_CALL(env, napi_set_named_property(env, out, "isInf", inf));
  return out;
}

static napi_value Free(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t h;
  if (!get_args(env, info, 2, argv, &ctx) || !get_u64(env, argv[1], &h)) return BAD_ARG(env, "free");
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

/* {c, glv, safe, buckets, timing, reduceAffine, scalarBits} -> msmz_opts; a key that is absent, and anything that is no
   object, leaves 0.  scalarBits: every scalar < 2^scalarBits; 0 = no bound */
static void get_opts(napi_env env, napi_value obj, msmz_opts* o) {
  memset(o, 0, sizeof(*o));
  o->c = opt_i32(env, obj, "c");
  o->glv = opt_i32(env, obj, "glv");
  o->safe = opt_i32(env, obj, "safe");
  o->buckets = opt_i32(env, obj, "buckets");
  o->timing = opt_i32(env, obj, "timing");
  o->reserved[0] = opt_i32(env, obj, "reduceAffine");
  o->reserved[1] = opt_i32(env, obj, "scalarBits");
}

static void set_num(napi_env env, napi_value obj, const char* key, double v) {
  napi_value n; napi_create_double(env, v, &n); napi_set_named_property(env, obj, key, n);
}

/* {xy, isInf} of one point */
static napi_value point_result(napi_env env, napi_value xy, int is_inf) {
  napi_value res, inf;
  NAPI_CALL(env, napi_create_object(env, &res));
  NAPI_CALL(env, napi_get_boolean(env, is_inf != 0, &inf));
  NAPI_CALL(env, napi_set_named_property(env, res, "xy", xy));
  NAPI_CALL(env, napi_set_named_property(env, res, "isInf", inf));
  return res;
}

/* The results of a call that gives `count` points: many_begin makes the Buffer for the records (count * 2 fe_bytes of
   the context's curve) and the flag array the C ABI writes; many_results turns the call's status into the error, or
   {xy (count records), isInf (count flags in a Buffer)}, and frees the flag array on every path.  Nothing returns
   between the two. */
typedef struct { napi_value xy; uint8_t* data; int* flags; uint64_t count; } many;
static int many_begin(napi_env env, msmz_ctx* ctx, uint64_t count, many* m) {
  void* data;
  m->count = count;
  m->flags = (int*)calloc((size_t)count, sizeof(int));
  if (m->flags && napi_create_buffer(env, 2 * (size_t)msmz_ctx_fe_bytes(ctx) * (size_t)count, &data, &m->xy) == napi_ok) {
    m->data = (uint8_t*)data;
    return 1;
  }
  free(m->flags);
  return 0;
}
static napi_value many_results(napi_env env, many* m, int st, const char* where) {
  void* fdata = NULL; napi_value inf, res;
  if (st == 0 && napi_create_buffer(env, (size_t)m->count, &fdata, &inf) == napi_ok)
    for (uint64_t k = 0; k < m->count; k++) ((uint8_t*)fdata)[k] = m->flags[k] ? 1 : 0;
  free(m->flags);
  if (st) return throw_status(env, st, where);
  if (!fdata) return BAD_ARG(env, where);
  NAPI_CALL(env, napi_create_object(env, &res));
  NAPI_CALL(env, napi_set_named_property(env, res, "xy", m->xy));
  NAPI_CALL(env, napi_set_named_property(env, res, "isInf", inf));
  return res;
}

/* msm(ctx, pointsHandle, scalars (handle number or Buffer), n, feBytes, opts) -> {xy, isInf, log} */
static napi_value Msm(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t ph, n, sh = 0;
  if (!get_args(env, info, 5, argv, &ctx) || !get_u64(env, argv[1], &ph) || !get_u64(env, argv[3], &n) ||
      !is_fe_bytes(env, argv[4], msmz_ctx_fe_bytes(ctx)))
    return BAD_ARG(env, "msm");
  void* s; size_t slen;
  const int host = opt_buffer(env, argv[2], &s, &slen);   /* a Buffer = host scalars */
  if (host ? slen < 32 * n : !get_u64(env, argv[2], &sh)) return BAD_ARG(env, "msm");
  msmz_opts o; get_opts(env, argv[5], &o);
  void* data; napi_value xy;
  NAPI_CALL(env, napi_create_buffer(env, 2 * (size_t)msmz_ctx_fe_bytes(ctx), &data, &xy));
  int is_inf = 0; msmz_log log;
  int st = host ? msmz_msm(ctx, ph, (const uint8_t*)s, n, &o, (uint8_t*)data, &is_inf, &log)
                : msmz_msm_resident(ctx, ph, sh, n, &o, (uint8_t*)data, &is_inf, &log);
  if (st) return throw_status(env, st, "msmz_msm");
  napi_value res = point_result(env, xy, is_inf), jlog, stages, rounds;
  if (!res) return NULL;
  NAPI_CALL(env, napi_create_object(env, &jlog));
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
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t ph, n, batch, sh = 0;
  if (!get_args(env, info, 6, argv, &ctx) || !get_u64(env, argv[1], &ph) || !get_u64(env, argv[3], &n) ||
      !get_u64(env, argv[4], &batch) || !is_fe_bytes(env, argv[5], msmz_ctx_fe_bytes(ctx)) || batch == 0 || batch > 0xffffffffu)
    return BAD_ARG(env, "msmBatch");
  void* s; size_t slen;
  const int host = opt_buffer(env, argv[2], &s, &slen);
  if (host ? (n == 0 || slen / 32 / n < batch) : !get_u64(env, argv[2], &sh)) return BAD_ARG(env, "msmBatch");
  msmz_opts o; get_opts(env, argv[6], &o);
  many m;
  if (!many_begin(env, ctx, batch, &m)) return BAD_ARG(env, "msmBatch");
  int st = host ? msmz_msm_batch(ctx, ph, (const uint8_t*)s, n, (uint32_t)batch, &o, m.data, m.flags, NULL)
                : msmz_msm_batch_resident(ctx, ph, sh, n, (uint32_t)batch, &o, m.data, m.flags, NULL);
  return many_results(env, &m, st, "msmz_msm_batch");
}

/* msmSegments(ctx, pointsHandle, scalarsHandle, segs (Buffer: per segment firstPoint, firstScalar, n as three
 * little-endian uint64 = msmz_segment), count, feBytes, opts) -> {xy (count records), isInf (count flags in a Buffer)} */
static napi_value MsmSegments(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t ph, sh, count;
  if (!get_args(env, info, 6, argv, &ctx) || !get_u64(env, argv[1], &ph) || !get_u64(env, argv[2], &sh) ||
      !get_u64(env, argv[4], &count) || !is_fe_bytes(env, argv[5], msmz_ctx_fe_bytes(ctx)) || count == 0 || count > 0xffffffffu)
    return BAD_ARG(env, "msmSegments");
  void* sp; size_t slen;
  if (!opt_buffer(env, argv[3], &sp, &slen) || slen / sizeof(msmz_segment) < count) return BAD_ARG(env, "msmSegments");
  msmz_opts o; get_opts(env, argv[6], &o);
  msmz_segment* segs = (msmz_segment*)malloc((size_t)count * sizeof(msmz_segment));   /* (a Buffer need not be aligned) */
  many m;
  if (!segs || !many_begin(env, ctx, count, &m)) { free(segs); return BAD_ARG(env, "msmSegments"); }
  memcpy(segs, sp, (size_t)count * sizeof(msmz_segment));
  const int st = msmz_msm_segments(ctx, ph, sh, segs, (uint32_t)count, &o, m.data, m.flags, NULL);
  free(segs);
  return many_results(env, &m, st, "msmz_msm_segments");
}

/* precomputePoints(ctx, pointsHandle, n, {c, glv, scalarBits}, factor) -> handle of a precomputed point set (msmz_precompute_points;
   glv -1 = the engine's choice, factor 0 = all windows in one bucket set) */
static napi_value PrecomputePoints(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t ph, n, factor, h = 0;
  if (!get_args(env, info, 5, argv, &ctx) || !get_u64(env, argv[1], &ph) || !get_u64(env, argv[2], &n) ||
      !get_u64(env, argv[4], &factor) || factor > 0xffffffffu)
    return BAD_ARG(env, "precomputePoints");
  msmz_opts o; get_opts(env, argv[3], &o);
  int st = msmz_precompute_points(ctx, ph, n, &o, (uint32_t)factor, &h);
  if (st) return throw_status(env, st, "msmz_precompute_points");
  return make_handle(env, h);
}

/* precomputedInfo(ctx, handle) -> {c, glv, factor, K, records, scalarBits} (msmz_precomputed_info,
   msmz_precomputed_scalar_bits) */
static napi_value PrecomputedInfo(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t h;
  if (!get_args(env, info, 2, argv, &ctx) || !get_u64(env, argv[1], &h)) return BAD_ARG(env, "precomputedInfo");
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
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t h, first, count, what;
  if (!get_args(env, info, 6, argv, &ctx) || !get_u64(env, argv[1], &h) || !get_u64(env, argv[2], &first) ||
      !get_u64(env, argv[3], &count) || !get_u64(env, argv[4], &what) || what > 0xffffffffu || count > 0xffffffffu)
    return BAD_ARG(env, "checkPoints");
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
   firstAddend, n, scalarBits (0 = no bound), flags (MSMZ_MUL_*)) -> handle of a new point set, record i = [s_i] P_i
   (+ Q_i)  (msmz_points_mul_opts; a Buffer is the one scalar, little-endian, for every point) */
static napi_value MulPoints(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  msmz_mul m; memset(&m, 0, sizeof(m));
  msmz_mul_opts o; memset(&o, 0, sizeof(o));
  uint64_t n, bits, flags, h = 0;
  if (!get_args(env, info, 10, argv, &ctx) || !get_u64(env, argv[1], &m.points_handle) || !get_u64(env, argv[2], &m.first_p) ||
      !get_u64(env, argv[4], &m.first_s) || !get_u64(env, argv[5], &m.addend_handle) || !get_u64(env, argv[6], &m.first_q) ||
      !get_u64(env, argv[7], &n) || !scalar_or_handle(env, argv[3], &m.scalar, &m.scalars_handle) ||
      (!m.scalar && !m.scalars_handle) || !get_u64(env, argv[8], &bits) || bits > 256 || !get_u64(env, argv[9], &flags) ||
      flags > 0xffffffffu)
    return BAD_ARG(env, "mulPoints");
  o.scalar_bits = (int32_t)bits;
  o.flags = (uint32_t)flags;
  int st = msmz_points_mul_opts(ctx, &m, n, &o, &h);
  if (st) return throw_status(env, st, "msmz_points_mul_opts");
  return make_handle(env, h);
}

/* fixedBaseMul(ctx, scalarsHandle, firstScalar, n, base (null = the generator, a Buffer of 2 * fe_bytes = x || y
   little-endian, or the handle of a resident point array), baseIndex, scalarBits (0 = no bound)) -> handle of a new
   point set, record i = [s_(firstScalar + i)] B  (msmz_points_fixed_base) */
static napi_value FixedBaseMul(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  msmz_fixed_base f; memset(&f, 0, sizeof(f));
  uint64_t n, bits, h = 0;
  if (!get_args(env, info, 7, argv, &ctx) || !get_u64(env, argv[1], &f.scalars_handle) || !get_u64(env, argv[2], &f.first_s) ||
      !get_u64(env, argv[3], &n) || !get_u64(env, argv[5], &f.base_index) || !get_u64(env, argv[6], &bits) || bits > 256)
    return BAD_ARG(env, "fixedBaseMul");
  napi_valuetype t;
  NAPI_CALL(env, napi_typeof(env, argv[4], &t));
  void* xy = NULL; size_t len = 0;
  if (t == napi_null || t == napi_undefined) {
    /* the generator */
  } else if (opt_buffer(env, argv[4], &xy, &len)) {
    if (len != 2 * (size_t)msmz_ctx_fe_bytes(ctx)) return BAD_ARG(env, "fixedBaseMul");
    f.base_xy_le = (const uint8_t*)xy;
  } else if (!get_u64(env, argv[4], &f.base_handle) || !f.base_handle) {
    return BAD_ARG(env, "fixedBaseMul");
  }
  f.scalar_bits = (int32_t)bits;
  int st = msmz_points_fixed_base(ctx, &f, n, &h);
  if (st) return throw_status(env, st, "msmz_points_fixed_base");
  return make_handle(env, h);
}

/* scalarsCombine(ctx, xHandle, xFirst, xCoeff, xCoeffFirst, yHandle (0 = no second term), yFirst, yCoeff, yCoeffFirst, n,
   firstOut, outHandle (0 = a new array)) -> handle of the array written: entry i = xCoeff_i x_i (+ yCoeff_i y_i)
   (msmz_scalars_combine).  A coefficient: a 32-byte Buffer (one scalar for every entry, little-endian), null (1), or
   the handle of a resident scalar array */
static napi_value ScalarsCombine(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  msmz_scalar_term x, y; memset(&x, 0, sizeof(x)); memset(&y, 0, sizeof(y));
  uint64_t n, first_out, h = 0;
  if (!get_args(env, info, 12, argv, &ctx) || !get_u64(env, argv[1], &x.handle) || !get_u64(env, argv[2], &x.first) ||
      !scalar_or_handle(env, argv[3], &x.coeff, &x.coeff_handle) || !get_u64(env, argv[4], &x.coeff_first) ||
      !get_u64(env, argv[5], &y.handle) || !get_u64(env, argv[6], &y.first) ||
      !scalar_or_handle(env, argv[7], &y.coeff, &y.coeff_handle) || !get_u64(env, argv[8], &y.coeff_first) ||
      !get_u64(env, argv[9], &n) || !get_u64(env, argv[10], &first_out) || !get_u64(env, argv[11], &h))
    return BAD_ARG(env, "scalarsCombine");
  int st = msmz_scalars_combine(ctx, &x, y.handle ? &y : NULL, n, first_out, &h);
  if (st) return throw_status(env, st, "msmz_scalars_combine");
  return make_handle(env, h);
}

/* scalarsDot(ctx, xHandle, xFirst, yHandle (0 = the plain sum of x), yFirst, n) -> 32-byte Buffer, little-endian
   (msmz_scalars_dot) */
static napi_value ScalarsDot(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t xh, fx, yh, fy, n;
  if (!get_args(env, info, 6, argv, &ctx) || !get_u64(env, argv[1], &xh) || !get_u64(env, argv[2], &fx) ||
      !get_u64(env, argv[3], &yh) || !get_u64(env, argv[4], &fy) || !get_u64(env, argv[5], &n))
    return BAD_ARG(env, "scalarsDot");
  void* data; napi_value buf;
  NAPI_CALL(env, napi_create_buffer(env, 32, &data, &buf));
  int st = msmz_scalars_dot(ctx, xh, fx, yh, fy, n, (uint8_t*)data);
  if (st) return throw_status(env, st, "msmz_scalars_dot");
  return buf;
}

/* scalarsPowers(ctx, base (32-byte Buffer or null = 1), ratio (32-byte Buffer), n) -> handle of a new scalar array, entry
   i = base ratio^i (msmz_scalars_powers) */
static napi_value ScalarsPowers(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  const uint8_t *base, *ratio;
  uint64_t n, h = 0;
  if (!get_args(env, info, 4, argv, &ctx) || !scalar_or_null(env, argv[1], &base) || !scalar_or_null(env, argv[2], &ratio) ||
      !ratio || !get_u64(env, argv[3], &n))
    return BAD_ARG(env, "scalarsPowers");
  int st = msmz_scalars_powers(ctx, base, ratio, n, &h);
  if (st) return throw_status(env, st, "msmz_scalars_powers");
  return make_handle(env, h);
}

/* scalarsRecurrence(ctx, a (handle, 32-byte Buffer = one multiplier for every entry, or null = 1), aFirst, bHandle (0 = no
   addend), bFirst, init (32-byte Buffer or null), flags (1 = reverse, 2 = exclusive), n, firstOut, outHandle (0 = a new
   array)) -> {handle, last}: the array written and the final value as a 32-byte Buffer  (msmz_scalars_recurrence) */
static napi_value ScalarsRecurrence(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  msmz_scalar_rec r; memset(&r, 0, sizeof(r));
  uint64_t flags, n, first_out, h = 0;
  if (!get_args(env, info, 10, argv, &ctx) || !scalar_or_handle(env, argv[1], &r.a, &r.a_handle) ||
      !get_u64(env, argv[2], &r.a_first) || !get_u64(env, argv[3], &r.b_handle) || !get_u64(env, argv[4], &r.b_first) ||
      !scalar_or_null(env, argv[5], &r.init) || !get_u64(env, argv[6], &flags) || flags >> 32 ||
      !get_u64(env, argv[7], &n) || !get_u64(env, argv[8], &first_out) || !get_u64(env, argv[9], &h))
    return BAD_ARG(env, "scalarsRecurrence");
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
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t xh, first, n, first_out, h = 0, zeros = 0;
  if (!get_args(env, info, 6, argv, &ctx) || !get_u64(env, argv[1], &xh) || !get_u64(env, argv[2], &first) ||
      !get_u64(env, argv[3], &n) || !get_u64(env, argv[4], &first_out) || !get_u64(env, argv[5], &h))
    return BAD_ARG(env, "scalarsInverse");
  int st = msmz_scalars_inverse(ctx, xh, first, n, first_out, &h, &zeros);
  if (st) return throw_status(env, st, "msmz_scalars_inverse");
  napi_value res;
  NAPI_CALL(env, napi_create_object(env, &res));
  NAPI_CALL(env, napi_set_named_property(env, res, "handle", make_handle(env, h)));
  set_num(env, res, "zeros", (double)zeros);
  return res;
}

/* scalarsNtt(ctx, handle, first, logN, flags (1 = inverse, 2 = coset), nIn (0 = n), count, root (32-byte Buffer or null =
   the default root), shift (32-byte Buffer with the coset flag, else null), firstOut, outHandle (0 = a new array)) ->
   handle of the array written: count transforms of length 2^logN  (msmz_scalars_ntt) */
static napi_value ScalarsNtt(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  msmz_ntt t; memset(&t, 0, sizeof(t));
  uint64_t log_n, flags, count, first_out, h = 0;
  if (!get_args(env, info, 11, argv, &ctx) || !get_u64(env, argv[1], &t.handle) || !get_u64(env, argv[2], &t.first) ||
      !get_u64(env, argv[3], &log_n) || log_n >> 32 || !get_u64(env, argv[4], &flags) || flags >> 32 ||
      !get_u64(env, argv[5], &t.n_in) || !get_u64(env, argv[6], &count) || count >> 32 ||
      !scalar_or_null(env, argv[7], &t.root) || !scalar_or_null(env, argv[8], &t.shift) ||
      !get_u64(env, argv[9], &first_out) || !get_u64(env, argv[10], &h))
    return BAD_ARG(env, "scalarsNtt");
  t.log_n = (uint32_t)log_n; t.flags = (uint32_t)flags; t.count = (uint32_t)count;
  int st = msmz_scalars_ntt(ctx, &t, first_out, &h);
  if (st) return throw_status(env, st, "msmz_scalars_ntt");
  return make_handle(env, h);
}

/* scalarsRootOfUnity(curveId, logN) -> 32-byte Buffer, little-endian: the default primitive 2^logN-th root of unity of the
   curve's scalar field  (msmz_scalars_root_of_unity; no context) */
static napi_value ScalarsRootOfUnity(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS];
  int32_t curve;
  uint64_t log_n;
  if (!get_args(env, info, 2, argv, NULL) || napi_get_value_int32(env, argv[0], &curve) != napi_ok ||
      !get_u64(env, argv[1], &log_n) || log_n >> 32)
    return BAD_ARG(env, "scalarsRootOfUnity");
  void* data; napi_value buf;
  NAPI_CALL(env, napi_create_buffer(env, 32, &data, &buf));
  int st = msmz_scalars_root_of_unity(curve, (uint32_t)log_n, (uint8_t*)data);
  if (st) return throw_status(env, st, "msmz_scalars_root_of_unity");
  return buf;
}

/* a point of nVars variables: a Buffer of at least nVars * 32 bytes (none needed for 0 variables) */
static int get_point(napi_env env, napi_value v, uint64_t n_vars, const uint8_t** out) {
  void* p; size_t len;
  *out = NULL;
  if (n_vars > 31) return 0;
  if (!opt_buffer(env, v, &p, &len)) return n_vars == 0;
  *out = (const uint8_t*)p;
  return len >= 32 * (size_t)n_vars;
}

/* scalarsEqTable(ctx, point (Buffer of nVars * 32 bytes), nVars, scale (32-byte Buffer or null = 1)) -> handle of a new
   scalar array of 2^nVars entries, entry i = scale eq(point, i)  (msmz_scalars_eq_table) */
static napi_value ScalarsEqTable(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  const uint8_t *point, *scale;
  uint64_t n_vars, h = 0;
  if (!get_args(env, info, 4, argv, &ctx) || !get_u64(env, argv[2], &n_vars) || !get_point(env, argv[1], n_vars, &point) ||
      !scalar_or_null(env, argv[3], &scale))
    return BAD_ARG(env, "scalarsEqTable");
  int st = msmz_scalars_eq_table(ctx, point, (uint32_t)n_vars, scale, &h);
  if (st) return throw_status(env, st, "msmz_scalars_eq_table");
  return make_handle(env, h);
}

/* scalarsMleEval(ctx, handle, first, point (Buffer of nVars * 32 bytes), nVars) -> 32-byte Buffer, little-endian: the
   polynomial of entries [first, first + 2^nVars) at the point  (msmz_scalars_mle_eval) */
static napi_value ScalarsMleEval(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  const uint8_t* point;
  uint64_t h, first, n_vars;
  if (!get_args(env, info, 5, argv, &ctx) || !get_u64(env, argv[1], &h) || !get_u64(env, argv[2], &first) ||
      !get_u64(env, argv[4], &n_vars) || !get_point(env, argv[3], n_vars, &point))
    return BAD_ARG(env, "scalarsMleEval");
  void* data; napi_value buf;
  NAPI_CALL(env, napi_create_buffer(env, 32, &data, &buf));
  int st = msmz_scalars_mle_eval(ctx, h, first, (uint32_t)n_vars, point, (uint8_t*)data);
  if (st) return throw_status(env, st, "msmz_scalars_mle_eval");
  return buf;
}

/* scalarsMleBind(ctx, handle, first, nVars, count, flags (1 = the low variable), r (32-byte Buffer), firstOut, outHandle
   (0 = a new array)) -> handle of the array written: count tables of 2^(nVars-1) entries  (msmz_scalars_mle_bind) */
static napi_value ScalarsMleBind(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  msmz_mle_bind b; memset(&b, 0, sizeof(b));
  uint64_t n_vars, count, flags, first_out, h = 0;
  if (!get_args(env, info, 9, argv, &ctx) || !get_u64(env, argv[1], &b.handle) || !get_u64(env, argv[2], &b.first) ||
      !get_u64(env, argv[3], &n_vars) || n_vars >> 32 || !get_u64(env, argv[4], &count) || count >> 32 ||
      !get_u64(env, argv[5], &flags) || flags >> 32 || !scalar_or_null(env, argv[6], &b.r) || !b.r ||
      !get_u64(env, argv[7], &first_out) || !get_u64(env, argv[8], &h))
    return BAD_ARG(env, "scalarsMleBind");
  b.n_vars = (uint32_t)n_vars; b.count = (uint32_t)count; b.flags = (uint32_t)flags;
  int st = msmz_scalars_mle_bind(ctx, &b, first_out, &h);
  if (st) return throw_status(env, st, "msmz_scalars_mle_bind");
  return make_handle(env, h);
}

/* scalarsSumcheckRound(ctx, tables (Buffer: nTables records of sizeof(msmz_sumcheck_table) = 16 bytes, handle and first
   as little-endian u64), nTables, nVars, masks (Buffer: nTerms little-endian u32), coeffs (Buffer: nTerms * 32 bytes),
   unit (Buffer: nTerms bytes, 1 = the coefficient is 1 and its 32 bytes are not read), nTerms, flags (1 = the low
   variable)) -> Buffer of (degree + 1) * 32 bytes: g(0) .. g(degree)  (msmz_scalars_sumcheck_round) */
static napi_value ScalarsSumcheckRound(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t n_tables, n_vars, n_terms, flags;
  void *tp, *mp, *cp, *up; size_t tl, ml, cl, ul;
  if (!get_args(env, info, 9, argv, &ctx) || !opt_buffer(env, argv[1], &tp, &tl) || !get_u64(env, argv[2], &n_tables) ||
      !get_u64(env, argv[3], &n_vars) || n_vars >> 32 || !opt_buffer(env, argv[4], &mp, &ml) ||
      !opt_buffer(env, argv[5], &cp, &cl) || !opt_buffer(env, argv[6], &up, &ul) || !get_u64(env, argv[7], &n_terms) ||
      !get_u64(env, argv[8], &flags) || flags >> 32 || n_tables < 1 || n_tables > MSMZ_SUMCHECK_MAX_TABLES ||
      n_terms < 1 || n_terms > MSMZ_SUMCHECK_MAX_TERMS || tl < n_tables * sizeof(msmz_sumcheck_table) || ml < n_terms * 4 ||
      cl < n_terms * 32 || ul < n_terms)
    return BAD_ARG(env, "scalarsSumcheckRound");
  msmz_sumcheck_table tables[MSMZ_SUMCHECK_MAX_TABLES];   /* (a Buffer need not be aligned) */
  msmz_sumcheck_term terms[MSMZ_SUMCHECK_MAX_TERMS];
  memcpy(tables, tp, (size_t)n_tables * sizeof(msmz_sumcheck_table));
  for (uint64_t k = 0; k < n_terms; k++) {
    memcpy(&terms[k].mask, (const uint8_t*)mp + 4 * k, 4);
    terms[k].coeff = ((const uint8_t*)up)[k] ? NULL : (const uint8_t*)cp + 32 * k;
  }
  msmz_sumcheck s = {tables, (uint32_t)n_tables, (uint32_t)n_vars, terms, (uint32_t)n_terms, (uint32_t)flags};
  uint8_t evals[(MSMZ_SUMCHECK_MAX_DEGREE + 1) * 32];
  uint32_t degree = 0;
  int st = msmz_scalars_sumcheck_round(ctx, &s, &degree, evals);
  if (st) return throw_status(env, st, "msmz_scalars_sumcheck_round");
  napi_value buf;
  NAPI_CALL(env, napi_create_buffer_copy(env, ((size_t)degree + 1) * 32, evals, NULL, &buf));
  return buf;
}

/* allocScalars(ctx, n) -> handle of a new scalar array of n entries whose contents are unspecified, for a call that
   writes into an existing array  (msmz_alloc_scalars) */
static napi_value AllocScalars(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t n, h = 0;
  if (!get_args(env, info, 2, argv, &ctx) || !get_u64(env, argv[1], &n)) return BAD_ARG(env, "allocScalars");
  int st = msmz_alloc_scalars(ctx, n, &h);
  if (st) return throw_status(env, st, "msmz_alloc_scalars");
  return make_handle(env, h);
}

/* scalarsSumcheckStep(ctx, tables, outs (a Buffer like tables: one destination per table, or null: every table in place),
   nTables, nVars, masks, coeffs, unit, nTerms, flags, r (32-byte Buffer)) -- tables, masks, coeffs, unit and flags as
   scalarsSumcheckRound takes them -> Buffer of (degree + 1) * 32 bytes: the polynomial of the next round over the bound
   tables, or with nVars == 1 the one value that is left  (msmz_scalars_sumcheck_step) */
static napi_value ScalarsSumcheckStep(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t n_tables, n_vars, n_terms, flags;
  const uint8_t* r;
  void *tp, *op, *mp, *cp, *up; size_t tl, ol = 0, ml, cl, ul;
  napi_valuetype out_type;
  if (!get_args(env, info, 11, argv, &ctx) || !opt_buffer(env, argv[1], &tp, &tl) || napi_typeof(env, argv[2], &out_type) != napi_ok ||
      !get_u64(env, argv[3], &n_tables) || !get_u64(env, argv[4], &n_vars) || n_vars >> 32 ||
      !opt_buffer(env, argv[5], &mp, &ml) || !opt_buffer(env, argv[6], &cp, &cl) || !opt_buffer(env, argv[7], &up, &ul) ||
      !get_u64(env, argv[8], &n_terms) || !get_u64(env, argv[9], &flags) || flags >> 32 ||
      !scalar_or_null(env, argv[10], &r) || !r || n_tables < 1 || n_tables > MSMZ_SUMCHECK_MAX_TABLES || n_terms < 1 ||
      n_terms > MSMZ_SUMCHECK_MAX_TERMS || tl < n_tables * sizeof(msmz_sumcheck_table) || ml < n_terms * 4 || cl < n_terms * 32 ||
      ul < n_terms)
    return BAD_ARG(env, "scalarsSumcheckStep");
  const int in_place = out_type == napi_null || out_type == napi_undefined;
  if (!in_place && (!opt_buffer(env, argv[2], &op, &ol) || ol < n_tables * sizeof(msmz_sumcheck_table)))
    return BAD_ARG(env, "scalarsSumcheckStep");
  msmz_sumcheck_table tables[MSMZ_SUMCHECK_MAX_TABLES], outs[MSMZ_SUMCHECK_MAX_TABLES];   /* (a Buffer need not be aligned) */
  msmz_sumcheck_term terms[MSMZ_SUMCHECK_MAX_TERMS];
  memcpy(tables, tp, (size_t)n_tables * sizeof(msmz_sumcheck_table));
  if (!in_place) memcpy(outs, op, (size_t)n_tables * sizeof(msmz_sumcheck_table));
  for (uint64_t k = 0; k < n_terms; k++) {
    memcpy(&terms[k].mask, (const uint8_t*)mp + 4 * k, 4);
    terms[k].coeff = ((const uint8_t*)up)[k] ? NULL : (const uint8_t*)cp + 32 * k;
  }
  msmz_sumcheck_step s = {tables, in_place ? NULL : outs, (uint32_t)n_tables, (uint32_t)n_vars, terms, (uint32_t)n_terms,
                          (uint32_t)flags, r};
  uint8_t evals[(MSMZ_SUMCHECK_MAX_DEGREE + 1) * 32];
  uint32_t degree = 0;
  int st = msmz_scalars_sumcheck_step(ctx, &s, &degree, evals);
  if (st) return throw_status(env, st, "msmz_scalars_sumcheck_step");
  napi_value buf;
  NAPI_CALL(env, napi_create_buffer_copy(env, ((size_t)degree + 1) * 32, evals, NULL, &buf));
  return buf;
}

/* scalarsDotMany(ctx, rows, nRows, cols, nCols (Buffers of msmz_scalar_vec: handle, first as little-endian u64 pairs), n,
   resident (0: the values come back as a Buffer of nRows * nCols * 32 bytes, row-major; 1: they go to a scalar array),
   outHandle (resident: the array written, 0 = a new one of nRows * nCols entries), firstOut)
   -> the Buffer, or the handle written  (msmz_scalars_dot_many) */
static napi_value ScalarsDotMany(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t n_rows, n_cols, n, resident, h, first_out;
  void *rp, *cp; size_t rl, cl;
  if (!get_args(env, info, 9, argv, &ctx) || !opt_buffer(env, argv[1], &rp, &rl) || !get_u64(env, argv[2], &n_rows) ||
      !opt_buffer(env, argv[3], &cp, &cl) || !get_u64(env, argv[4], &n_cols) || !get_u64(env, argv[5], &n) ||
      !get_u64(env, argv[6], &resident) || resident > 1 || !get_u64(env, argv[7], &h) || !get_u64(env, argv[8], &first_out) ||
      n_rows < 1 || n_rows > MSMZ_DOT_MANY_MAX_ROWS || n_cols < 1 || n_cols > MSMZ_DOT_MANY_MAX_COLS ||
      rl < n_rows * sizeof(msmz_scalar_vec) || cl < n_cols * sizeof(msmz_scalar_vec))
    return BAD_ARG(env, "scalarsDotMany");
  msmz_scalar_vec rows[MSMZ_DOT_MANY_MAX_ROWS], cols[MSMZ_DOT_MANY_MAX_COLS];   /* (a Buffer need not be aligned) */
  memcpy(rows, rp, (size_t)n_rows * sizeof(msmz_scalar_vec));
  memcpy(cols, cp, (size_t)n_cols * sizeof(msmz_scalar_vec));
  msmz_dot_many d = {rows, (uint32_t)n_rows, cols, (uint32_t)n_cols, n, 0};
  if (resident) {
    int st = msmz_scalars_dot_many(ctx, &d, NULL, first_out, &h);
    if (st) return throw_status(env, st, "msmz_scalars_dot_many");
    return make_handle(env, h);
  }
  uint8_t out[MSMZ_DOT_MANY_MAX_ROWS * MSMZ_DOT_MANY_MAX_COLS * 32];   /* 32 KiB */
  int st = msmz_scalars_dot_many(ctx, &d, out, first_out, NULL);
  if (st) return throw_status(env, st, "msmz_scalars_dot_many");
  napi_value buf;
  NAPI_CALL(env, napi_create_buffer_copy(env, (size_t)(n_rows * n_cols) * 32, out, NULL, &buf));
  return buf;
}

/* matrixCreate(ctx, rows, cols (Buffers of nnz little-endian u32 each), nnz, valHandle (0 = every value is 1), valFirst,
   nRows, nCols, flags (1 = rows, 2 = cols, 3 = both)) -> handle of a new sparse matrix  (msmz_matrix_create) */
static napi_value MatrixCreate(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  msmz_sparse s; memset(&s, 0, sizeof(s));
  uint64_t n_rows, n_cols, flags, h = 0;
  void *rp, *cp; size_t rl, cl;
  if (!get_args(env, info, 9, argv, &ctx) || !opt_buffer(env, argv[1], &rp, &rl) || !opt_buffer(env, argv[2], &cp, &cl) ||
      !get_u64(env, argv[3], &s.nnz) || s.nnz == 0 || s.nnz >> 32 || rl < 4 * s.nnz || cl < 4 * s.nnz ||
      !get_u64(env, argv[4], &s.val_handle) || !get_u64(env, argv[5], &s.val_first) || !get_u64(env, argv[6], &n_rows) ||
      n_rows >> 32 || !get_u64(env, argv[7], &n_cols) || n_cols >> 32 || !get_u64(env, argv[8], &flags) || flags >> 32)
    return BAD_ARG(env, "matrixCreate");
  uint32_t* idx = (uint32_t*)malloc(8 * (size_t)s.nnz);   /* (a Buffer need not be aligned) */
  if (!idx) return throw_status(env, MSMZ_ERR_HIP, "matrixCreate");
  memcpy(idx, rp, 4 * (size_t)s.nnz);
  memcpy(idx + s.nnz, cp, 4 * (size_t)s.nnz);
  s.row = idx; s.col = idx + s.nnz;
  s.n_rows = (uint32_t)n_rows; s.n_cols = (uint32_t)n_cols; s.flags = (uint32_t)flags;
  int st = msmz_matrix_create(ctx, &s, &h);
  free(idx);
  if (st) return throw_status(env, st, "msmz_matrix_create");
  return make_handle(env, h);
}

/* matrixInfo(ctx, handle) -> {nRows, nCols, nnz, flags}  (msmz_matrix_info) */
static napi_value MatrixInfo(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t h, nnz = 0;
  uint32_t n_rows = 0, n_cols = 0, flags = 0;
  if (!get_args(env, info, 2, argv, &ctx) || !get_u64(env, argv[1], &h)) return BAD_ARG(env, "matrixInfo");
  int st = msmz_matrix_info(ctx, h, &n_rows, &n_cols, &nnz, &flags);
  if (st) return throw_status(env, st, "msmz_matrix_info");
  napi_value res;
  NAPI_CALL(env, napi_create_object(env, &res));
  set_num(env, res, "nRows", (double)n_rows);
  set_num(env, res, "nCols", (double)n_cols);
  set_num(env, res, "nnz", (double)nnz);
  set_num(env, res, "flags", (double)flags);
  return res;
}

/* matrixMul(ctx, matrix, xHandle, xFirst, flags (1 = transposed), firstOut, outHandle (0 = a new array)) -> handle of
   the array written  (msmz_matrix_mul) */
static napi_value MatrixMul(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  msmz_matvec v; memset(&v, 0, sizeof(v));
  uint64_t flags, first_out, h = 0;
  if (!get_args(env, info, 7, argv, &ctx) || !get_u64(env, argv[1], &v.matrix) || !get_u64(env, argv[2], &v.x_handle) ||
      !get_u64(env, argv[3], &v.x_first) || !get_u64(env, argv[4], &flags) || flags >> 32 ||
      !get_u64(env, argv[5], &first_out) || !get_u64(env, argv[6], &h))
    return BAD_ARG(env, "matrixMul");
  v.flags = (uint32_t)flags;
  int st = msmz_matrix_mul(ctx, &v, first_out, &h);
  if (st) return throw_status(env, st, "msmz_matrix_mul");
  return make_handle(env, h);
}

/* scalarsLookup(ctx, tableHandle, tableFirst, tableN, colHandle, colFirst, colN, firstOut, outHandle (0 = a new array),
   wantPositions) -> {handle, missing, firstMissing (-1 = none), distinct, positions: Buffer of colN little-endian u32 or
   null}  (msmz_scalars_lookup) */
static napi_value ScalarsLookup(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  msmz_lookup l; memset(&l, 0, sizeof(l));
  uint64_t first_out, h = 0;
  if (!get_args(env, info, 10, argv, &ctx) || !get_u64(env, argv[1], &l.table_handle) || !get_u64(env, argv[2], &l.table_first) ||
      !get_u64(env, argv[3], &l.table_n) || !get_u64(env, argv[4], &l.col_handle) || !get_u64(env, argv[5], &l.col_first) ||
      !get_u64(env, argv[6], &l.col_n) || l.col_n == 0 || l.col_n >> 32 || !get_u64(env, argv[7], &first_out) ||
      !get_u64(env, argv[8], &h))
    return BAD_ARG(env, "scalarsLookup");
  bool want = false;
  NAPI_CALL(env, napi_get_value_bool(env, argv[9], &want));
  void* data = NULL; napi_value buf;
  if (want) NAPI_CALL(env, napi_create_buffer(env, 4 * (size_t)l.col_n, &data, &buf));
  else NAPI_CALL(env, napi_get_null(env, &buf));
  l.positions = (uint32_t*)data;
  msmz_lookup_result r; memset(&r, 0, sizeof(r));
  int st = msmz_scalars_lookup(ctx, &l, first_out, &h, &r);
  if (st) return throw_status(env, st, "msmz_scalars_lookup");
  napi_value res;
  NAPI_CALL(env, napi_create_object(env, &res));
  NAPI_CALL(env, napi_set_named_property(env, res, "handle", make_handle(env, h)));
  set_num(env, res, "missing", (double)r.n_missing);
  set_num(env, res, "firstMissing", r.first_missing == UINT64_MAX ? -1.0 : (double)r.first_missing);
  set_num(env, res, "distinct", (double)r.n_distinct);
  NAPI_CALL(env, napi_set_named_property(env, res, "positions", buf));
  return res;
}

/* scalarsExpr(ctx, columns (Buffer: nColumns records of sizeof(msmz_expr_column) = 16 bytes, handle and first as
   little-endian u64), nColumns, factors (Buffer: the factors of all terms in a row, sizeof(msmz_expr_factor) = 8 bytes
   each, column as little-endian u32 and rot as i32), counts (Buffer: nTerms bytes, the factors of each term), coeffs
   (Buffer: nTerms * 32 bytes), unit (Buffer: nTerms bytes, 1 = the coefficient is 1 and its 32 bytes are not read),
   nTerms, n, firstOut, outHandle (0 = a new array)) -> handle of the array written  (msmz_scalars_expr) */
static napi_value ScalarsExpr(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS]; msmz_ctx* ctx;
  uint64_t n_columns, n_terms, n, first_out, h = 0;
  void *colp, *fp, *kp, *cp, *up; size_t coll, fl, kl, cl, ul;
  if (!get_args(env, info, 11, argv, &ctx) || !opt_buffer(env, argv[1], &colp, &coll) || !get_u64(env, argv[2], &n_columns) ||
      !opt_buffer(env, argv[3], &fp, &fl) || !opt_buffer(env, argv[4], &kp, &kl) || !opt_buffer(env, argv[5], &cp, &cl) ||
      !opt_buffer(env, argv[6], &up, &ul) || !get_u64(env, argv[7], &n_terms) || !get_u64(env, argv[8], &n) ||
      !get_u64(env, argv[9], &first_out) || !get_u64(env, argv[10], &h) || n_columns < 1 || n_columns > MSMZ_EXPR_MAX_COLUMNS ||
      n_terms < 1 || n_terms > MSMZ_EXPR_MAX_TERMS || coll < n_columns * sizeof(msmz_expr_column) || kl < n_terms ||
      cl < n_terms * 32 || ul < n_terms)
    return BAD_ARG(env, "scalarsExpr");
  msmz_expr_column columns[MSMZ_EXPR_MAX_COLUMNS];   /* (a Buffer need not be aligned) */
  msmz_expr_factor factors[MSMZ_EXPR_MAX_TERMS * MSMZ_EXPR_MAX_DEGREE];
  msmz_expr_term terms[MSMZ_EXPR_MAX_TERMS];
  memcpy(columns, colp, (size_t)n_columns * sizeof(msmz_expr_column));
  size_t at = 0;
  for (uint64_t k = 0; k < n_terms; k++) {
    const size_t nf = ((const uint8_t*)kp)[k];
    if (nf > MSMZ_EXPR_MAX_DEGREE || fl < (at + nf) * sizeof(msmz_expr_factor)) return BAD_ARG(env, "scalarsExpr");
    memcpy(factors + at, (const uint8_t*)fp + at * sizeof(msmz_expr_factor), nf * sizeof(msmz_expr_factor));
    terms[k].coeff = ((const uint8_t*)up)[k] ? NULL : (const uint8_t*)cp + 32 * k;
    terms[k].factors = nf ? factors + at : NULL;
    terms[k].n_factors = (uint32_t)nf;
    terms[k].reserved = 0;
    at += nf;
  }
  msmz_expr e = {columns, (uint32_t)n_columns, (uint32_t)n_terms, terms, n, 0};
  int st = msmz_scalars_expr(ctx, &e, first_out, &h);
  if (st) return throw_status(env, st, "msmz_scalars_expr");
  return make_handle(env, h);
}

/* descriptorSizes() -> {mleBind, sumcheck, sumcheckTable, sumcheckTerm, maxTables, maxDegree, maxTerms}: what the addon
   was compiled with, for the host to check its packing against (no context).  descriptorSizes("matrix") -> {sparse,
   matvec, matRows, matCols, matvecTranspose}: the same for the descriptors and flags of the sparse-matrix calls;
   descriptorSizes("lookup") -> {lookup, lookupResult, none}: the two descriptors of scalarsLookup and the position of a
   column entry that is in no table; descriptorSizes("expr") -> {exprColumn, exprFactor, exprTerm, expr, maxColumns,
   maxTerms, maxDegree, maxOperands}; descriptorSizes("sumcheckStep") -> {sumcheckStep, sumcheckTable, sumcheckTerm};
   descriptorSizes("dotMany") -> {dotMany, scalarVec, maxRows, maxCols}
   (the call without an argument answers what it always did). */
static napi_value DescriptorSizes(napi_env env, napi_callback_info info) {
  napi_value res, argv[MAX_ARGS];
  size_t argc = MAX_ARGS;
  char family[16] = "";
  size_t got = 0;
  NAPI_CALL(env, napi_create_object(env, &res));
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < 1 ||
      napi_get_value_string_utf8(env, argv[0], family, sizeof(family), &got) != napi_ok)
    family[0] = 0;
  if (strcmp(family, "lookup") == 0) {
    set_num(env, res, "lookup", (double)sizeof(msmz_lookup));
    set_num(env, res, "lookupResult", (double)sizeof(msmz_lookup_result));
    set_num(env, res, "none", (double)0xffffffffu);
    return res;
  }
  if (strcmp(family, "expr") == 0) {   /* the descriptors and limits of scalarsExpr */
    set_num(env, res, "exprColumn", (double)sizeof(msmz_expr_column));
    set_num(env, res, "exprFactor", (double)sizeof(msmz_expr_factor));
    set_num(env, res, "exprTerm", (double)sizeof(msmz_expr_term));
    set_num(env, res, "expr", (double)sizeof(msmz_expr));
    set_num(env, res, "maxColumns", (double)MSMZ_EXPR_MAX_COLUMNS);
    set_num(env, res, "maxTerms", (double)MSMZ_EXPR_MAX_TERMS);
    set_num(env, res, "maxDegree", (double)MSMZ_EXPR_MAX_DEGREE);
    set_num(env, res, "maxOperands", (double)MSMZ_EXPR_MAX_OPERANDS);
    return res;
  }
  if (strcmp(family, "dotMany") == 0) {   /* the descriptors and limits of scalarsDotMany */
    set_num(env, res, "dotMany", (double)sizeof(msmz_dot_many));
    set_num(env, res, "scalarVec", (double)sizeof(msmz_scalar_vec));
    set_num(env, res, "maxRows", (double)MSMZ_DOT_MANY_MAX_ROWS);
    set_num(env, res, "maxCols", (double)MSMZ_DOT_MANY_MAX_COLS);
    return res;
  }
  if (strcmp(family, "sumcheckStep") == 0) {   /* the descriptors of scalarsSumcheckStep */
    set_num(env, res, "sumcheckStep", (double)sizeof(msmz_sumcheck_step));
    set_num(env, res, "sumcheckTable", (double)sizeof(msmz_sumcheck_table));
    set_num(env, res, "sumcheckTerm", (double)sizeof(msmz_sumcheck_term));
    return res;
  }
  if (strcmp(family, "matrix") == 0) {
    set_num(env, res, "sparse", (double)sizeof(msmz_sparse));
    set_num(env, res, "matvec", (double)sizeof(msmz_matvec));
    set_num(env, res, "matRows", (double)MSMZ_MAT_ROWS);
    set_num(env, res, "matCols", (double)MSMZ_MAT_COLS);
    set_num(env, res, "matvecTranspose", (double)MSMZ_MATVEC_TRANSPOSE);
    return res;
  }
  set_num(env, res, "mleBind", (double)sizeof(msmz_mle_bind));
  set_num(env, res, "sumcheck", (double)sizeof(msmz_sumcheck));
  set_num(env, res, "sumcheckTable", (double)sizeof(msmz_sumcheck_table));
  set_num(env, res, "sumcheckTerm", (double)sizeof(msmz_sumcheck_term));
  set_num(env, res, "maxTables", (double)MSMZ_SUMCHECK_MAX_TABLES);
  set_num(env, res, "maxDegree", (double)MSMZ_SUMCHECK_MAX_DEGREE);
  set_num(env, res, "maxTerms", (double)MSMZ_SUMCHECK_MAX_TERMS);
  return res;
}

/* pointAdd(curveId, aXy|null, bXy|null, feBytes) -> {xy, isInf}  (null = infinity).  Refused: a curve id the library does
   not know, a feBytes that is not that curve's, an input Buffer shorter than the 2 * fe_bytes the library reads */
static napi_value PointAdd(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS];
  int32_t curve;
  if (!get_args(env, info, 4, argv, NULL) || napi_get_value_int32(env, argv[0], &curve) != napi_ok ||
      !is_fe_bytes(env, argv[3], msmz_curve_fe_bytes(curve)))
    return BAD_ARG(env, "pointAdd");
  const size_t rec = 2 * (size_t)msmz_curve_fe_bytes(curve);
  void *a, *b; size_t la, lb;
  if ((opt_buffer(env, argv[1], &a, &la) && la < rec) || (opt_buffer(env, argv[2], &b, &lb) && lb < rec))
    return BAD_ARG(env, "pointAdd");
  void* data; napi_value xy;
  NAPI_CALL(env, napi_create_buffer(env, rec, &data, &xy));
  int is_inf = 0;
  int st = msmz_point_add(curve, (const uint8_t*)a, a == NULL, (const uint8_t*)b, b == NULL, (uint8_t*)data, &is_inf);
  if (st) return throw_status(env, st, "msmz_point_add");
  return point_result(env, xy, is_inf);
}

static napi_value FeBytes(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS];
  int32_t curve;
  if (!get_args(env, info, 1, argv, NULL) || napi_get_value_int32(env, argv[0], &curve) != napi_ok) return BAD_ARG(env, "feBytes");
  napi_value v; napi_create_int32(env, msmz_curve_fe_bytes(curve), &v);
  return v;
}

static napi_value Init(napi_env env, napi_value exports) {
  static const struct { const char* name; napi_callback fn; } fns[] = {
      {"create", Create}, {"destroy", Destroy}, {"uploadPoints", UploadPoints}, {"uploadScalars", UploadScalars},
      {"importScalars", ImportScalars}, {"importPoints", ImportPoints},
      {"importPointsCompressed", ImportPointsCompressed}, {"downloadPointsCompressed", DownloadPointsCompressed},
      {"randomPoints", RandomPoints}, {"randomScalars", RandomScalars}, {"downloadPoints", DownloadPoints},
      {"downloadScalars", DownloadScalars}, {"exportScalars", ExportScalars}, {"exportPoints", ExportPoints}, {"free", Free}, {"msm", Msm}, {"msmBatch", MsmBatch}, {"msmSegments", MsmSegments},
      {"precomputePoints", PrecomputePoints}, {"precomputedInfo", PrecomputedInfo}, {"checkPoints", CheckPoints},
      {"mulPoints", MulPoints}, {"fixedBaseMul", FixedBaseMul}, {"scalarsCombine", ScalarsCombine}, {"scalarsDot", ScalarsDot},
      {"scalarsPowers", ScalarsPowers}, {"scalarsRecurrence", ScalarsRecurrence}, {"scalarsInverse", ScalarsInverse},
      {"scalarsNtt", ScalarsNtt}, {"scalarsRootOfUnity", ScalarsRootOfUnity},
      {"scalarsEqTable", ScalarsEqTable}, {"scalarsMleEval", ScalarsMleEval}, {"scalarsMleBind", ScalarsMleBind},
      {"scalarsSumcheckRound", ScalarsSumcheckRound}, {"scalarsSumcheckStep", ScalarsSumcheckStep}, {"allocScalars", AllocScalars},
      {"descriptorSizes", DescriptorSizes},
      {"matrixCreate", MatrixCreate}, {"matrixInfo", MatrixInfo}, {"matrixMul", MatrixMul},
      {"scalarsLookup", ScalarsLookup}, {"scalarsExpr", ScalarsExpr}, {"scalarsDotMany", ScalarsDotMany},
      {"pointAdd", PointAdd}, {"feBytes", FeBytes}};
  for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); i++) {
    napi_value f;
    if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
    napi_set_named_property(env, exports, fns[i].name, f);
  }
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)

/* msmz -- C ABI of the MI355X-native Pippenger MSM engine.
 *
 * This is the drop-in boundary for the reference's MSM hot path: the functions below are what an
 * N-API / ctypes binding calls in place of the reference's wasm-backed
 *   Curve.Parallel.{msm, msmUnsafe, msmProjective, pointsFromBytes, scalarsFromBytes,
 *                   randomPointsFast, randomScalars}      (src/parallel.ts:89-158, 209-271)
 * and the result read-back   Projective.toAffine + Affine.toBigint   (scripts/msm-weierstrass.ts:90-92).
 * See INTEGRATION.md for the binding a maintainer would add.
 *
 * Conventions: every function returns an int status (0 = MSMZ_OK; msmz_strerror() explains the
 * rest); no C++ types cross the boundary; the caller owns all host buffers; a context drives the
 * GPU(s) it was created for and is not thread-safe (one caller at a time per context); there is no CPU fallback --
 * creating a context without a usable HIP device fails.
 *
 * Wire formats (same as the reference's byte route, parallel.ts:97-133, 209-249):
 *   point  = x || y, each coordinate little-endian canonical (non-Montgomery), fe_bytes = 48
 *            (BLS12-377 / BLS12-381) or 32 (Pallas, ed-on-bls12-377); optional per-point infinity flag
 *   scalar = 32 bytes little-endian, value < group order
 *   result = canonical affine x || y (both < p) + infinity flag -- "bit-exact" is defined on this.
 * Imported forms (msmz_import_scalars / msmz_import_points, below): the same records read where the caller has them, in
 * host or device memory, at a byte stride; scalars of 4..32 bytes (zero-extended); scalars and coordinates optionally
 * as 64-bit-limb Montgomery residues (v * 2^256 mod q, v * 2^(8 fe_bytes) mod p).  The resident format and the results
 * are the same whichever way the data came in.
 */
#ifndef MSMZ_H
#define MSMZ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* curve ids: src/concrete/{bls12-377,pasta,bls12-381,ed-on-bls12-377}.params.ts */
enum {
  MSMZ_BLS12_377_G1 = 0,
  MSMZ_PALLAS = 1,
  MSMZ_BLS12_381_G1 = 2,
  MSMZ_ED_ON_BLS12_377 = 3
};

enum {
  MSMZ_OK = 0,
  MSMZ_ERR_ARG = 1,          /* bad argument (null pointer, unknown curve / handle, N mismatch) */
  MSMZ_ERR_NO_DEVICE = 2,    /* no usable HIP device: there is no CPU fallback */
  MSMZ_ERR_HIP = 3,          /* a HIP call failed (out of memory, launch failure) */
  MSMZ_ERR_UNSUPPORTED = 4,  /* option combination not available for this curve */
  MSMZ_ERR_DEGENERATE = 5,   /* msmUnsafe hit P + (+-P): a batch inversion saw a zero denominator
                                (the reference traps with wasm `unreachable`, inverse.ts:198-199) */
  MSMZ_ERR_RANGE = 6,        /* a scalar is >= the group order (or >= 2^bits of msmz_opts.reserved[1]) / a coordinate is >= p;
                                imported Montgomery residues: the residue itself is >= q / >= p */
  MSMZ_ERR_POINT = 7         /* a compressed record is not a point of the curve: no square root, or a sign bit on a zero root */
};

enum { MSMZ_BUCKETS_AFFINE = 0, MSMZ_BUCKETS_PROJECTIVE = 1 };

/* Per-call options: the reference's `{c, useSafeAdditions}` (msm-batched-affine.ts:79-82) plus the
 * choices BASELINE.json's configs name (GLV on/off, affine vs projective buckets). 0 = default. */
typedef struct msmz_opts {
  int32_t c;        /* window size in bits; 0 = pick from N like windowSizeAffine (msm-common.ts:15-21) */
  int32_t glv;      /* 1 = GLV endomorphism split (the reference always splits on Weierstrass curves), 0 = off,
                     * -1 = the engine picks (GLV below 2^21 points, the measured crossover; the result is the same) */
  int32_t safe;     /* 1 = msm (handles equal / opposite / infinity points), 0 = msmUnsafe */
  int32_t buckets;  /* MSMZ_BUCKETS_AFFINE (batched-affine) or MSMZ_BUCKETS_PROJECTIVE (msmProjective) */
  int32_t timing;   /* 1 = fill msmz_log stage timings with HIP events (the reference's tic/toc log) */
  int32_t reserved[3]; /* reserved[0] = 1: first level of the bucket reduction by batched-affine additions
                        * (reduceBucketsAffine, msm-batched-affine-single-thread.ts:522-667) instead of XYZZ running
                        * sums; same result, measured slower on MI355X (profiles/r02_reduce_ab.txt): default 0
                        * reserved[1] = scalar bit bound: "every scalar of this call is below 2^reserved[1]".  The windows are
                        * sized for it (64-bit scalars at c = 17: 4 windows, not 15), and so is everything paid per window.
                        * 0 = no bound; a value of at least the scalar field's bit length means the same; a negative value
                        * or one above 256 is MSMZ_ERR_ARG.  A scalar >= 2^reserved[1] fails the call with MSMZ_ERR_RANGE
                        * (checked exactly, on the device, while the scalars are sliced, like a scalar >= the group
                        * order; a batched call fails as a whole; the context stays usable).  With glv = -1 a bound of at
                        * most the GLV half length turns the split off.  The result is the same with and without it. */
} msmz_opts;

/* Stage timings + counts, the analogue of the `log` array msm() returns (msm-common.ts:192-230). */
enum {
  MSMZ_ST_DIGITS = 0,      /* GLV + signed digits + histogram */
  MSMZ_ST_SCAN = 1,        /* bucket offsets */
  MSMZ_ST_SCATTER = 2,     /* counting-sort scatter of references (the HBM-bound kernel) */
  MSMZ_ST_PLAN = 3,        /* per-round pair offsets */
  MSMZ_ST_ACCUMULATE = 4,  /* all batched-affine tree rounds (or projective bucket accumulation) */
  MSMZ_ST_REDUCE = 5,      /* bucket reduction */
  MSMZ_ST_FINAL = 6,       /* window sums -> result (host) */
  MSMZ_ST_TOTAL = 7,       /* whole call, host wall clock */
  MSMZ_N_STAGES = 8
};

typedef struct msmz_log {
  float stage_ms[MSMZ_N_STAGES];
  int32_t c, K, rounds, glv;
  uint64_t n_entries;       /* non-zero digits = bucket insertions ("point-adds" of the metric) */
  uint64_t n_pairs;         /* affine additions performed in the tree rounds */
  uint32_t max_bucket;
  uint32_t scatter_launches;
  float scatter_kernel_ms;  /* duration of the scatter kernel alone (roofline numerator's time) */
  float batch_add_ms[32];   /* per tree round */
} msmz_log;

typedef struct msmz_ctx msmz_ctx;

/* device_ids / n_devices: the GPU(s) this context drives, 1 <= n_devices <= MSMZ_MAX_DEVICES (0 = "CPU backend":
 * refused with MSMZ_ERR_NO_DEVICE).  Replaces startThreads(n) (parallel.ts:291-315, threads.ts:132-359): with
 * n_devices > 1 the context owns one engine + HIP stream + host thread per device, every uploaded / generated set is
 * split over the devices in contiguous blocks of 2^16 entries dealt round-robin (so the first n entries of a set are a
 * prefix on every device), msmz_msm runs the whole pipeline on each device's share concurrently and adds the partial
 * sums on the host (no inter-GPU traffic).  The same device id may be listed more than once
 * (used to rehearse the scheduler on one GPU).  The other route to multi-GPU -- one process and one single-device
 * context per GPU, partial sums combined with msmz_point_add -- is what bench.py --gpus N uses. */
#define MSMZ_MAX_DEVICES 8
int msmz_create(msmz_ctx** ctx, int curve_id, const int* device_ids, int n_devices);
void msmz_destroy(msmz_ctx* ctx);            /* stopThreads() + frees every handle */
const char* msmz_strerror(int status);
int msmz_curve_fe_bytes(int curve_id);       /* 48 or 32; -1 for an unknown curve */
int msmz_ctx_fe_bytes(const msmz_ctx* ctx);  /* fe_bytes of the context's curve; -1 for a null context */
int msmz_ctx_n_devices(const msmz_ctx* ctx); /* number of engines (GPUs) the context drives */

/* Point sets live on the GPU across MSMs, like the reference keeps them in wasm memory
 * (scripts/msm-weierstrass.ts:19-35).  pointsFromBytes (parallel.ts:97-112 / 209-232). */
int msmz_upload_points(msmz_ctx* ctx, const uint8_t* xy_le, const uint8_t* is_inf /* nullable */, uint64_t n,
                       uint64_t* handle);
/* scalarsFromBytes (parallel.ts:114-133) */
int msmz_upload_scalars(msmz_ctx* ctx, const uint8_t* scalars_le32, uint64_t n, uint64_t* handle);
/* randomPointsFast / randomScalars (curve-random.ts:14-92, 151-194), seeded and generated on the GPU:
 * point i = a_i * G with a_i = splitmix64(seed, i) (64-bit), scalar i = rejection-sampled 32 bytes. */
int msmz_random_points(msmz_ctx* ctx, uint64_t n, uint64_t seed, uint64_t* handle);
int msmz_random_scalars(msmz_ctx* ctx, uint64_t n, uint64_t seed, uint64_t* handle);
int msmz_download_points(msmz_ctx* ctx, uint64_t handle, uint64_t first, uint64_t count, uint8_t* xy_le,
                         uint8_t* is_inf /* nullable */);
int msmz_download_scalars(msmz_ctx* ctx, uint64_t handle, uint64_t first, uint64_t count, uint8_t* scalars_le32);
/* msmz_download_points with compressed records (below, MSMZ_SRC_COMPRESSED): out receives count * fe_bytes bytes, the
 * wire coordinate with the sign bit in bit 7 of the last byte; flags = 0 (sign = larger root) or MSMZ_SRC_SIGN_PARITY
 * (sign = odd), anything else is MSMZ_ERR_ARG.  The range rules are those of msmz_download_points.  A point at infinity
 * is written as all-zero bytes with is_inf = 1; is_inf is nullable but the bytes alone do not tell infinity from the
 * point (0, 1) of BLS12-377, which also compresses to zeros.  ed-on-bls12-377 has no infinity: is_inf is all 0. */
int msmz_download_points_compressed(msmz_ctx* ctx, uint64_t handle, uint64_t first, uint64_t count, uint8_t* out,
                                    uint8_t* is_inf /* nullable */, uint32_t flags);
int msmz_free(msmz_ctx* ctx, uint64_t handle);

/* Import: make a resident handle of records where the caller has them, in the form they have.
 * The handles are ordinary scalar / point handles: every function that takes an uploaded one takes them, an MSM over
 * them returns the same bytes, msmz_download_* return the canonical values.
 *   flags 0               ptr (and is_inf) are host memory; only `width` bytes per record are copied to the GPU (a
 *                         strided source is packed on the host first).  Scalars of width 32 at stride 0: the handle
 *                         holds what msmz_upload_scalars leaves.
 *   MSMZ_SRC_DEVICE       ptr (and is_inf) are memory of the context's GPU, or pinned / registered host memory it can
 *                         read.  The engine asks the HIP runtime what the pointer is (hipPointerGetAttributes) and that the
 *                         whole source lies inside that one allocation (hipMemGetAddressRange), and refuses anything
 *                         else with MSMZ_ERR_ARG: no kernel is launched
 *                         on a pointer the runtime does not know.  Ordering: `stream` (a hipStream_t) is the stream
 *                         whose queued work produces the data -- the engine records an event on it and makes its own
 *                         stream wait for that event, no host wait; NULL = the data is ready.  The null stream cannot be
 *                         named by a pointer: MSMZ_SRC_DEFAULT_STREAM says "order after the device's null stream".
 *   MSMZ_SRC_MONTGOMERY   records are 64-bit-limb Montgomery residues (arkworks / sppark style; little-endian limbs =
 *                         little-endian bytes): scalars v * 2^256 mod q (width 32 only), coordinates
 *                         v * 2^(8 fe_bytes) mod p.  Converted on the GPU.
 *   MSMZ_SRC_COMPRESSED   points only: a record is ONE coordinate, fe_bytes little-endian canonical
 *                         bytes -- x on the Weierstrass curves, y on ed-on-bls12-377 -- with the sign of the other
 *                         coordinate in bit 7 of the last byte (free in all four fields).  `width` is 0 or fe_bytes.  The
 *                         GPU recovers the other coordinate (one field square root per point) and the handle is an
 *                         ordinary point handle: msmz_download_points returns x || y.  sign = 1 means the canonical value
 *                         of the recovered coordinate is larger than (p - 1) / 2 (believed to match arkworks' YIsNegative
 *                         flag and zcash's "lexicographically largest"; neither library was run against this); with
 *                         MSMZ_SRC_SIGN_PARITY it means that value is odd (believed to match pasta_curves).  A recovered
 *                         coordinate of 0 takes sign 0 only.  There is no infinity bit in the record: infinity is is_inf,
 *                         and a flagged record is not decompressed, its bytes may be anything (on ed-on-bls12-377, which has
 *                         no point at infinity, it becomes the identity (0, 1)).  An arkworks record with
 *                         its infinity flag in bit 6 is a coordinate >= p on BLS12-377 / BLS12-381: MSMZ_ERR_RANGE.
 *                         Not with MSMZ_SRC_MONTGOMERY; MSMZ_SRC_SIGN_PARITY needs MSMZ_SRC_COMPRESSED; either flag on a
 *                         scalar source is MSMZ_ERR_ARG.  MSMZ_ERR_RANGE: a coordinate >= p once the sign bit is masked
 *                         off.  MSMZ_ERR_POINT: a record with no square root, or a sign bit on a zero root.  Both are found
 *                         by the kernel, RANGE wins when both occur; no handle is created, the context stays usable.
 * Every import returns after the GPU has read the source: it may be overwritten or freed at once.
 * Errors.  MSMZ_ERR_ARG, before anything is launched: a null descriptor / pointer / handle pointer, n == 0 (scalars:
 * n >= 2^32; points: the limits of msmz_upload_points), unknown flag bits, a stream without MSMZ_SRC_DEVICE, a pointer not
 * 4-byte aligned, a stride that is neither 0 nor a multiple of 4 of at least the width (or is 2^24 or more), a scalar width outside 4..32
 * or not a multiple of 4 or (Montgomery) other than 32, a point width other than 0 or 2 * fe_bytes, is_inf on a scalar
 * source, memory the runtime does not vouch for.  MSMZ_ERR_RANGE, found by the conversion kernel: a scalar or residue
 * >= q, a coordinate or residue >= p; no handle is created and the context stays usable.
 * msmz_import_scalars_into writes n scalars over entries [first, first + n) of an existing scalar handle and nothing else
 * (a batch assembled vector by vector); a handle that is not a scalar set or first + n beyond it is MSMZ_ERR_ARG; after
 * MSMZ_ERR_RANGE the contents of [first, first + n) are unspecified.
 * Multi-device contexts: a device source is first copied to the host, then dealt to the devices like an upload, so the
 * result equals an upload and nothing is gained; msmz_import_scalars_into returns MSMZ_ERR_UNSUPPORTED there (a vector
 * start is not a block boundary of the devices' shares).  Like the rest of the multi-device code this has run on several
 * engines of ONE GPU only. */
enum {
  MSMZ_SRC_DEVICE = 1,
  MSMZ_SRC_MONTGOMERY = 2,
  MSMZ_SRC_DEFAULT_STREAM = 4,  /* with MSMZ_SRC_DEVICE and a NULL stream: the data is produced on the null stream */
  MSMZ_SRC_COMPRESSED = 8,      /* points: records are one coordinate + sign bit */
  MSMZ_SRC_SIGN_PARITY = 16     /* with MSMZ_SRC_COMPRESSED: the sign bit is the parity, not "the larger root" */
};
typedef struct msmz_src {
  const void* ptr;        /* first record */
  uint64_t stride;        /* bytes from one record to the next; 0 = packed (= the width) */
  uint32_t width;         /* scalars: bytes per record, 4..32, a multiple of 4; points: 0 or 2 * fe_bytes (compressed: fe_bytes) */
  uint32_t flags;         /* MSMZ_SRC_* */
  void* stream;           /* MSMZ_SRC_DEVICE: the hipStream_t whose work produces the data; NULL = the data is ready */
  const uint8_t* is_inf;  /* points only, nullable: one flag byte per point, packed, same memory space as ptr; checked but
                             without effect on the twisted-Edwards curve, which has no point at infinity (as the
                             is_inf of msmz_upload_points) */
} msmz_src;
int msmz_import_scalars(msmz_ctx* ctx, const msmz_src* src, uint64_t n, uint64_t* handle);
int msmz_import_scalars_into(msmz_ctx* ctx, uint64_t handle, uint64_t first, const msmz_src* src, uint64_t n);
int msmz_import_points(msmz_ctx* ctx, const msmz_src* src, uint64_t n, uint64_t* handle);
/* a new scalar handle of n zeros, the target msmz_import_scalars_into fills (n == 0 or n >= 2^32: MSMZ_ERR_ARG; a
 * multi-device context: MSMZ_ERR_UNSUPPORTED, as _into) */
int msmz_alloc_scalars(msmz_ctx* ctx, uint64_t n, uint64_t* handle);

/* Export: the way out that mirrors the imports.  Entries [first, first + n) of a resident set are
 * written where the caller wants them, in the form it wants: record i is entry first + i, at ptr + i * stride.  The
 * descriptor is msmz_src read in the other direction -- the same fields at the same offsets, the same MSMZ_SRC_* flags:
 *   flags 0               ptr (and is_inf) are host memory; only `width` bytes per record cross PCIe; a strided
 *                         destination is filled from a packed copy on the host and the bytes between records are not
 *                         touched.
 *   MSMZ_SRC_DEVICE       ptr (and is_inf) are memory of the context's GPU, or pinned / registered host memory it can
 *                         address; the engine asks the runtime, as for a source, about the (n - 1) * stride + width bytes
 *                         (is_inf: n bytes) it will write, and refuses anything else with MSMZ_ERR_ARG: nothing is
 *                         launched.  Ordering: `stream` is the stream whose queued work last reads or writes the
 *                         destination (MSMZ_SRC_DEFAULT_STREAM: the null stream) -- the engine records an event there and
 *                         its own stream waits for it before the kernel writes.
 *   MSMZ_SRC_MONTGOMERY   64-bit-limb Montgomery residues: scalars v * 2^256 mod q (width 32 only), coordinates
 *                         v * 2^(8 fe_bytes) mod p -- the exact inverse of the import.
 *   MSMZ_SRC_COMPRESSED   points only: one coordinate + sign bit, byte for byte msmz_download_points_compressed
 *                         (MSMZ_SRC_SIGN_PARITY: its second convention).  Not with MSMZ_SRC_MONTGOMERY.
 * Every export returns after the GPU has written everything (one host wait, the one that brings the error word): any
 * stream may read the destination afterwards.
 * Scalars: little-endian, `width` bytes (4..32, a multiple of 4).  An entry of the range that does not fit `width` bytes,
 * or is >= q, fails the call with MSMZ_ERR_RANGE (found by the kernel): the addressed records are then unspecified,
 * nothing outside them is written, the context stays usable.  Entries outside the range are not read.  A host export
 * with flags 0, width 32 and stride 0 gives byte for byte what msmz_download_scalars gives.
 * Points: the range rules of msmz_download_points (endomorphism images and the copies of a precomputed handle stay
 * readable); x || y canonical, Montgomery, or compressed.  Infinity on the Weierstrass curves is the all-zero record in
 * every form, with is_inf[i] = 1 where is_inf is given; on ed-on-bls12-377 the identity is (0, 1) in the requested form
 * and is_inf is all 0.  A host export with flags 0 and stride 0 is byte for byte msmz_download_points.
 * msmz_import_points of an exported buffer with the same flags and its is_inf gives a set that downloads identically.
 * MSMZ_ERR_ARG, before any launch and with the destination untouched: a null ctx, dst or ptr; n == 0; an unknown handle
 * or one of the wrong kind; a range beyond the set; every descriptor fault listed for a source above (is_inf on scalars
 * and the compressed flags on scalars included); memory the runtime does not vouch for.
 * Multi-device contexts: a host destination works (every engine exports its own blocks of 2^16 records); a device
 * destination is MSMZ_ERR_UNSUPPORTED. */
typedef struct msmz_dst {
  void* ptr;         /* first record */
  uint64_t stride;   /* bytes from one record to the next; 0 = packed (= the width) */
  uint32_t width;    /* scalars: 4..32, a multiple of 4; points: 0 or 2 * fe_bytes (compressed: 0 or fe_bytes) */
  uint32_t flags;    /* MSMZ_SRC_* */
  void* stream;      /* MSMZ_SRC_DEVICE: the hipStream_t whose queued work last reads or writes the destination */
  uint8_t* is_inf;   /* points only, nullable: one flag byte per point, packed, same memory space as ptr */
} msmz_dst;
int msmz_export_scalars(msmz_ctx* ctx, uint64_t handle, uint64_t first, uint64_t n, const msmz_dst* dst);
int msmz_export_points(msmz_ctx* ctx, uint64_t handle, uint64_t first, uint64_t n, const msmz_dst* dst);

/* The MSM: sum_i scalar_i * point_i over the first n entries.  Scalars either come from a host
 * buffer (copied to the GPU inside the call) or are already resident (scalars_handle).
 * out_xy_le: 2*fe_bytes.  Curve.Parallel.msm / msmUnsafe / msmProjective. */
int msmz_msm(msmz_ctx* ctx, uint64_t points_handle, const uint8_t* scalars_le32, uint64_t n, const msmz_opts* opts,
             uint8_t* out_xy_le, int* out_is_inf, msmz_log* log /* nullable */);
int msmz_msm_resident(msmz_ctx* ctx, uint64_t points_handle, uint64_t scalars_handle, uint64_t n,
                      const msmz_opts* opts, uint8_t* out_xy_le, int* out_is_inf, msmz_log* log /* nullable */);

/* Batched MSM: `batch` MSMs over the same first n points, out_k = sum_i scalars[k][i] * point_i, k = 0 .. batch-1 -- a
 * prover committing to many polynomials against one SRS.  scalars_le32: batch * n * 32 bytes, vector k at offset
 * k * n * 32 (host buffer, copied inside the call); msmz_msm_batch_resident: one scalar handle holding >= batch * n
 * scalars, vector k = entries [k n, (k+1) n).  out_xy_le: batch * 2 * fe_bytes; out_is_inf: batch ints.  Options as
 * msmz_msm; log (nullable) describes the whole call (stage times and counts are totals over the batch).
 * batch == 1 returns exactly what msmz_msm / msmz_msm_resident return; batch == 0 or n == 0 is MSMZ_ERR_ARG; a scalar
 * >= the group order in any vector fails the whole call with MSMZ_ERR_RANGE (the context stays usable).
 * Weierstrass curves with batched-affine buckets run all problems through ONE device pipeline (one sort, one plan, one
 * train of tree rounds, one bucket reduction, one host round trip), in consecutive sub-batches of at most 2^26 bucket
 * entries.  Twisted Edwards (ed-on-bls12-377), MSMZ_BUCKETS_PROJECTIVE, reserved[0] = 1 and n beyond one sort pass
 * (2^24 entries) run the problems one by one: same results, no batching gain.  A multi-device context runs the batch on
 * every device's share of the points and adds the partial sums on the host per problem; resident scalars are first
 * gathered to the host there. */
int msmz_msm_batch(msmz_ctx* ctx, uint64_t points_handle, const uint8_t* scalars_le32, uint64_t n, uint32_t batch,
                   const msmz_opts* opts, uint8_t* out_xy_le, int* out_is_inf, msmz_log* log /* nullable */);
int msmz_msm_batch_resident(msmz_ctx* ctx, uint64_t points_handle, uint64_t scalars_handle, uint64_t n,
                            uint32_t batch, const msmz_opts* opts, uint8_t* out_xy_le, int* out_is_inf,
                            msmz_log* log /* nullable */);

/* Segmented MSM: every problem has its own range of ONE resident point set and ONE resident scalar
 * set,
 *     out_k = sum_{i < n_k} scalar[first_s_k + i] * P[first_p_k + i],   k = 0 .. n_segs - 1
 * -- the L = <a_lo, G_hi> and R = <a_hi, G_lo> of an IPA round over the halves of one SRS, or commitments to columns of
 * different lengths against one SRS.  Segments may overlap or repeat.  Only the base points of a set are addressed: the
 * endomorphism images and the copies of a precomputed set are reached by the engine.  out_xy_le: n_segs * 2 * fe_bytes,
 * out_is_inf: n_segs ints, in the caller's order, as msmz_msm_batch lays them out.  Options mean what they mean for
 * msmz_msm_batch_resident (reserved[1], safe and timing included); log (nullable) describes the whole call, totals merged
 * as the batch merges them.  One segment {0, 0, n} returns exactly the bytes and status of msmz_msm_resident; n_segs
 * segments {0, k n, n} exactly those of msmz_msm_batch_resident.
 * How it runs: the segments are dealt into length classes (same floor(log2 n_k)).  On Weierstrass curves with
 * batched-affine buckets the segments of a class go through ONE device pipeline, sized for the class's longest segment,
 * in consecutive sub-batches as a batch; twisted Edwards, MSMZ_BUCKETS_PROJECTIVE, reserved[0] = 1, a length beyond one
 * sort pass and a class of one run segment by segment.  Same results either way.
 * MSMZ_ERR_ARG, before any launch: a null ctx, segs, out_xy_le or out_is_inf; n_segs == 0; a segment with n == 0; an
 * unknown handle or one of the wrong kind; a range beyond its set (tested without wrap-around); a precomputed handle:
 * first_p + n beyond the n it was built for, or options that contradict it (as msmz_msm).  MSMZ_ERR_RANGE: a scalar >= q
 * (or >= 2^reserved[1]) inside any segment fails the whole call, the context stays usable; a bad scalar no segment covers
 * is not read.  MSMZ_ERR_DEGENERATE: as msmUnsafe.  MSMZ_ERR_UNSUPPORTED: a multi-device context (sets are dealt in blocks
 * of 2^16 records, and a range is not a prefix of a device's share: the stance of msmz_import_scalars_into), and on a
 * precomputed handle the combinations unsupported in every MSM over one. */
typedef struct msmz_segment {
  uint64_t first_p;   /* first base point of the problem */
  uint64_t first_s;   /* first scalar of the problem */
  uint64_t n;         /* its length, >= 1 */
} msmz_segment;
int msmz_msm_segments(msmz_ctx* ctx, uint64_t points_handle, uint64_t scalars_handle, const msmz_segment* segs,
                      uint32_t n_segs, const msmz_opts* opts, uint8_t* out_xy_le, int* out_is_inf,
                      msmz_log* log /* nullable */);

/* Fixed-base precomputation of a resident point set.  The new handle holds `factor` copies of the
 * first n points of points_handle, copy j = 2^(c j) * P_i, so that window k of every scalar adds into bucket set
 * floor(k / factor) with copy k mod factor: ceil(K / factor) bucket reductions per MSM instead of K, and a Horner with
 * (factor - 1) fewer doubling runs per set.  factor 0 = all windows (one bucket set per MSM; the copies also cover the
 * window count of the GLV retry); 1 is MSMZ_ERR_ARG; a factor above the window count is lowered to it.  opts->c /
 * opts->glv fix the window size and the GLV choice the copies are built for (0 / -1 = the engine's choice for n; a null
 * opts means both); opts->reserved[1] is the scalar bit bound the copies are built for: the window count of bounded
 * scalars (fewer copies, less memory; factor 0 = all windows of a bounded scalar; a bound that leaves a single window
 * is MSMZ_ERR_ARG: nothing to share); opts->safe / timing play no part.  The new handle owns its memory: the source handle may be freed.
 * Memory: factor * R records of the point stride (R = n, or 2n with GLV: the endomorphism images follow the base points in
 * every copy), e.g. 2 GiB for 2^20 BLS12-377 points at c = 16, factor 0.
 * Limits (MSMZ_ERR_ARG at precompute time): the records fit the 30-bit record index (factor * R < 2^30), one bucket can
 * hold every entry of its set (min(factor, K) * n entries, 2n with GLV, below 2^26: all digits equal), and a bucket set
 * of min(factor, K) windows of n (2n with GLV) entries fits one pass of the two-level sort (n <= 2^24 entries; a window
 * at most 512 coarse bins, all windows at most 8192).  Twisted Edwards, MSMZ_BUCKETS_PROJECTIVE and reserved[0] = 1 are
 * MSMZ_ERR_UNSUPPORTED, here and in every MSM over a precomputed handle.
 * Use: msmz_msm, msmz_msm_resident, msmz_msm_batch and msmz_msm_batch_resident take the precomputed handle wherever they
 * take points_handle, n up to its n, and return bit-identical results to the plain handle; opts.c must be 0 or the
 * handle's c, opts.glv -1 or the handle's choice and opts.reserved[1] 0 (the handle's bound applies) or the handle's
 * bound (else MSMZ_ERR_ARG).  msmz_download_points reads its records: copy j
 * at [j R, (j + 1) R) (a multi-device context: the first n records, copy 0).  msmz_free releases it.  On a multi-device
 * context every engine precomputes its own share of the points. */
int msmz_precompute_points(msmz_ctx* ctx, uint64_t points_handle, uint64_t n, const msmz_opts* opts, uint32_t factor,
                           uint64_t* handle);
/* what a precomputed handle was built with (any pointer may be null): window size, GLV choice, copies, windows K of an
 * MSM over it and records (factor * R, all devices) */
int msmz_precomputed_info(msmz_ctx* ctx, uint64_t handle, int32_t* c, int32_t* glv, uint32_t* factor, uint32_t* K,
                          uint64_t* records);
/* the scalar bit bound a precomputed handle was built for: 0 = none (also for a bound of at least the field's bit length) */
int msmz_precomputed_scalar_bits(msmz_ctx* ctx, uint64_t handle, int32_t* bits);

/* Validation of a resident point set: is every point on the curve, and in the subgroup of prime
 * order q the scalars are reduced for?  The engine checks coordinates < p on the way in (MSMZ_ERR_RANGE) and nothing
 * else: every addition formula assumes a = 0 and never reads b, so an off-curve input is summed, silently, on some
 * other curve, and a point with a cofactor component gives a result outside the group.  This is the reference's
 * isOnCurve / isInSubgroup (src/curve-affine.ts:193, src/curve-projective.ts:291-303) over a resident set, on the GPU.
 * It is a QUERY: bad points are not an error, the call returns MSMZ_OK and `out` says what was found.
 *   what       MSMZ_CHECK_CURVE: y^2 = x^3 + b (Weierstrass), -x^2 + y^2 = 1 + d x^2 y^2 (twisted Edwards).
 *              MSMZ_CHECK_SUBGROUP (implies CURVE): also [q]P = O for every point on the curve, q the order of the curve
 *              parameters: one scalar multiplication per point.  Pallas has cofactor 1: there SUBGROUP equals CURVE and
 *              no scalar multiplication is run (curve-projective.ts:295).
 *   verdicts   nullable, count bytes: verdicts[i] describes point first + i.  Bit 0 (value 1): not on the curve.  Bit 1
 *              (value 2): on the curve and [q]P != O.  An off-curve point never has bit 1 (the group law means nothing
 *              for it; it is not multiplied).  With MSMZ_CHECK_CURVE alone bit 1 is never set.
 *   out        counts of either verdict in [first, first + count) and first_bad, the smallest index -- in the set, not
 *              relative to `first` -- with a non-zero verdict (UINT64_MAX: none).  Deterministic.
 * A Weierstrass point flagged as infinity when it came in is on the curve and in the subgroup whatever its coordinates
 * were (an UNFLAGGED (0, 0) is not that record: zero is stored as a non-zero multiple of p, and the point is reported
 * off the curve, as the reference's isOnCurve reports it); the twisted-Edwards identity (0, 1) is in the subgroup.  The resident records are what is read: a set that came in by
 * upload, import (host or device memory, canonical or Montgomery) or msmz_random_points is checked by the same code.  Of a
 * set with endomorphism images only the n base points are checked and indexed.
 * MSMZ_ERR_ARG, before any launch: a null ctx or out, an unknown or a scalar handle, count == 0, first + count beyond
 * the set, what == 0 or unknown bits in it.  MSMZ_ERR_UNSUPPORTED: a precomputed handle (derived data: check the source
 * set before precomputing).  On a multi-device context every engine checks its own share; indices are the set's. */
enum { MSMZ_CHECK_CURVE = 1, MSMZ_CHECK_SUBGROUP = 2 };   /* SUBGROUP implies CURVE */
typedef struct msmz_check_result {
  uint64_t off_curve;     /* points that do not satisfy the curve equation */
  uint64_t off_subgroup;  /* points on the curve with [q]P != O */
  uint64_t first_bad;     /* smallest index (in the set, not relative to `first`) with a non-zero verdict; UINT64_MAX = none */
} msmz_check_result;
int msmz_check_points(msmz_ctx* ctx, uint64_t points_handle, uint64_t first, uint64_t count, uint32_t what,
                      msmz_check_result* out, uint8_t* verdicts /* nullable, count bytes */);

/* Per-point scalar multiplication of resident point sets:
 *     out_i = [s_i] P_i (+ Q_i),   i = 0 .. n-1,   P_i = record first_p + i of points_handle, s_i and Q_i likewise
 * -- a NEW point set made from resident ones: IPA generator folding (G'_i = G_lo,i + [u] G_hi,i: one handle as P and Q,
 * first_p = n, first_q = 0, the broadcast u), SRS re-randomisation (P_i -> [tau^i] P_i).  (Fixed-base vectors [s_i] B
 * for ONE base are msmz_points_fixed_base's, below: the same result from a window table at a fraction of the cost.)
 * Result: a new plain point handle of n base points, exactly what msmz_upload_points of the same affine points leaves
 * (the endomorphism images behind them on the Weierstrass curves, Niels records on the twisted Edwards curve); every
 * function that takes a point handle takes it.  It owns its memory, and the call returns after the GPU has finished.
 * Values: [0]P, [s]O and P + (-P) are the point at infinity (Weierstrass: the all-zero record, is_inf = 1 on download;
 * ed-on-bls12-377: the identity (0, 1)).  The addition of Q is complete: Q = [s]P (a doubling), Q = -[s]P and either
 * operand at infinity are covered.  The inputs need not lie in the subgroup: a point of small order multiplies to what
 * the group law gives.  Of sets with endomorphism images only the base points are read.  Scalars are read whole: plain
 * double-and-add over all bits of the group order's length, one thread per point, 64 points sharing one field inversion
 * (msmz_points_mul_opts below: shorter chains for bounded scalars and for points known to lie in the subgroup).
 * MSMZ_ERR_ARG, before any launch: a null ctx, descriptor or out_handle; n == 0; an unknown handle or one of the wrong
 * kind; a range [first, first + n) beyond its set; scalars_handle == 0 with a null `scalar`; n beyond the limit of
 * msmz_upload_points.  MSMZ_ERR_UNSUPPORTED: a precomputed handle as P or Q.  MSMZ_ERR_RANGE: the broadcast scalar >= q
 * (checked on the host), or a resident scalar >= q (found by the kernel; no handle is created, the context stays usable).
 * Multi-device contexts: every engine multiplies its own share and the result is dealt like an upload.  Sets are dealt in
 * blocks of 2^16 records, so index i of P, s and Q lives on one device only when first_p == first_s == first_q == 0: any
 * other combination is MSMZ_ERR_UNSUPPORTED there.  Like the rest of the multi-device code this has run as several
 * engines on ONE GPU only. */
typedef struct msmz_mul {
  uint64_t points_handle;   /* plain point handle: P */
  uint64_t first_p;         /* P_i = record first_p + i */
  uint64_t scalars_handle;  /* scalar handle, or 0 = one scalar for all i (`scalar`) */
  uint64_t first_s;
  const uint8_t* scalar;    /* 32 bytes little-endian, < q; read only when scalars_handle == 0 */
  uint64_t addend_handle;   /* plain point handle Q, or 0 = no addend; may equal points_handle */
  uint64_t first_q;
} msmz_mul;
int msmz_points_mul(msmz_ctx* ctx, const msmz_mul* m, uint64_t n, uint64_t* out_handle);

/* msmz_points_mul with what the caller knows about its inputs; opts == NULL is msmz_points_mul.
 * Everything documented there holds, plus:
 * scalar_bits = b (all four curves): "every scalar of this call is below 2^b".  The chain then walks min(b, bit length
 * of q) bits instead of all of them -- a 128-bit challenge costs half.  0 = no bound, and b >= the bit length of q means
 * the same.  The result is byte-identical to the call without the bound.  MSMZ_ERR_RANGE: the broadcast scalar >= 2^b
 * (found on the host, nothing launched), or a resident scalar >= 2^b inside the addressed range (found by the kernel,
 * exactly like one >= q: no handle is created, the context stays usable).
 * MSMZ_MUL_SUBGROUP: the caller vouches that every finite P_i of the range lies in the prime-order subgroup
 * (msmz_check_points with MSMZ_CHECK_SUBGROUP earns that vouch); Q is not constrained.  On the three Weierstrass curves
 * the engine may then split s = (+-)k0 + (+-)k1 lambda and walk both halves jointly over the table
 * {(+-)P, (+-)phi P, their sum}: 126 (BLS12-377) or 128 steps instead of 253 / 255.  For such inputs the result is
 * byte-identical to the plain call.  For a P_i outside the subgroup record i is UNSPECIFIED -- some point of the curve, or
 * infinity -- while the call still returns MSMZ_OK, nothing faults and every other record is right.  ed-on-bls12-377 has
 * no endomorphism: the flag is accepted and changes nothing.
 * Which chain runs: a bound b <= the proven length of the GLV halves (126 / 128) -> the plain chain of b steps; else the
 * flag on a Weierstrass curve -> the GLV chain; else the plain chain of min(b, bit length of q) steps.
 * MSMZ_ERR_ARG: unknown bits in flags, a non-zero reserved word, scalar_bits < 0 or > 256.
 * Multi-device contexts pass the options to every engine. */
enum { MSMZ_MUL_SUBGROUP = 1 };
typedef struct msmz_mul_opts {
  uint32_t flags;        /* MSMZ_MUL_* */
  int32_t scalar_bits;   /* every scalar of this call is below 2^scalar_bits; 0 = no bound */
  int32_t reserved[2];   /* must be 0 */
} msmz_mul_opts;
int msmz_points_mul_opts(msmz_ctx* ctx, const msmz_mul* m, uint64_t n, const msmz_mul_opts* opts /* nullable */,
                         uint64_t* out_handle);

/* Fixed-base multiplication: a point set from a resident scalar set and ONE base,
 *     out_i = [s_(first_s + i)] B,   i = 0 .. n-1
 * -- a KZG SRS [tau^i]G from the powers msmz_scalars_powers leaves resident, Pedersen and ElGamal vectors, the fixed-base
 * half of a Groth16 setup, a test SRS with known discrete logs.  msmz_points_mul over n copies of B gives the same set
 * by a chain of 253 / 255 doublings per point; this call builds a window table of multiples of B once (kept for the
 * next call) and pays K = 16 to 32 mixed additions per point.
 * The base: record base_index of the plain point handle base_handle; or, with base_handle == 0, the canonical
 * little-endian x || y at base_xy_le (2 * fe_bytes; on the Weierstrass curves the all-zero record is the point at
 * infinity, as in a download), or the curve's generator when that is NULL too.  B is taken as given: it need not lie
 * in the subgroup, and a base of small order or at infinity multiplies to what the group law gives.
 * Result: a new plain point handle of n base points, byte for byte what msmz_points_mul leaves for n copies of B and the
 * same scalars -- the endomorphism images behind the base points, Niels records on ed-on-bls12-377, [0]B and every
 * multiple of an infinite B the infinity record / (0, 1).  Every function that takes a point handle takes it.
 * scalar_bits = b: "every scalar of the range is below 2^b", as in msmz_mul_opts: fewer windows, the same bytes.
 * MSMZ_ERR_ARG, before any launch: a null ctx, f or out_handle; n == 0 or beyond the limit of msmz_upload_points; an
 * unknown handle or one of the wrong kind; a scalar range beyond its set; base_index beyond the base points of
 * base_handle (or non-zero without one); both base_handle and base_xy_le; non-zero flags; scalar_bits < 0 or > 256.
 * MSMZ_ERR_UNSUPPORTED: a precomputed handle as base.  MSMZ_ERR_RANGE: a coordinate of base_xy_le >= p (found on the
 * host); a resident scalar >= q or >= 2^b inside the range (found by the kernel: no handle is created, *out_handle is as
 * it was, the context stays usable; scalars outside the range are not read).
 * The engine keeps the tables of the last few (base, window width, windows): a second call on the same base, and any
 * call on the generator after the first, skips the build.  A table is at most 64 MiB of device memory.
 * Multi-device contexts: the base is resolved to bytes once (one record is downloaded if it is resident), every engine
 * multiplies its own share of the scalars, and the result is dealt like an upload; first_s != 0 is MSMZ_ERR_UNSUPPORTED
 * there (the stance of msmz_points_mul).  Like the rest of the multi-device code this has run as several engines on ONE
 * GPU only. */
typedef struct msmz_fixed_base {
  uint64_t base_handle;       /* plain point handle holding B, or 0 */
  uint64_t base_index;        /* B = base-point record base_index of base_handle (0 when base_handle == 0) */
  const uint8_t* base_xy_le;  /* base_handle == 0: canonical x || y of B (2 * fe_bytes); NULL = the curve's generator */
  uint64_t scalars_handle;    /* resident scalar set, required */
  uint64_t first_s;
  int32_t scalar_bits;        /* every scalar of the range is below 2^scalar_bits; 0 = no bound (as msmz_mul_opts) */
  uint32_t flags;             /* must be 0 */
} msmz_fixed_base;            /* 48 bytes */
int msmz_points_fixed_base(msmz_ctx* ctx, const msmz_fixed_base* f, uint64_t n, uint64_t* out_handle);

/* Arithmetic mod q over resident scalar sets: linear combinations, inner products and powers of
 * one ratio, so that a prover's witness fold a' = a_lo + u^-1 a_hi, its cross terms <a_lo, b_hi>, a random linear
 * combination of columns sum_k r^k col_k or the vector (1, z, z^2, ...) never leave the device.  The reference has no
 * analogue: its scalars live in wasm memory and its callers do this arithmetic with bigints.
 * Values: a scalar set holds 32-byte little-endian values below q, and every result written here is again below q:
 * MSM, msmz_points_mul, msmz_download_scalars and msmz_import_scalars_into take such a set unchanged.
 *
 * msmz_scalars_combine: out_i = x.c_i * x.v_i (+ y.c_i * y.v_i), i < n; y nullable.  v_i = entry first + i of `handle`;
 * c_i = entry coeff_first + i of `coeff_handle`, or with coeff_handle == 0 the one scalar `coeff` for every i (NULL = 1).
 * *out_handle == 0 on entry: a new scalar handle of n entries (first_out must be 0).  Otherwise entries
 * [first_out, first_out + n) of that handle are overwritten and nothing else.  In place: the destination range may
 * coincide exactly with any input range (a[0, n/2) = a[0, n/2) + u^-1 a[n/2, n): x = {a, 0}, y = {a, n/2, coeff u^-1},
 * *out_handle = a, first_out = 0) or be disjoint from it; a partial overlap with an input range of the same handle is
 * MSMZ_ERR_ARG.  A product with a broadcast coefficient costs one Montgomery multiplication, one with a resident
 * coefficient two; coeff == NULL costs none.
 *
 * msmz_scalars_dot: sum_i x_i * y_i mod q over entries first_x + i and first_y + i (y_handle == 0: sum_i x_i, first_y
 * must be 0) as 32 bytes little-endian, below q.  x and y may be the same handle and may overlap.  The sum is exact, so
 * two calls return the same bytes.
 *
 * msmz_scalars_powers: a new scalar handle of n entries, entry i = base * ratio^i (base NULL = 1; 0^0 = 1).
 *
 * MSMZ_ERR_ARG, before any launch: a null ctx, x, out_handle, out_le32 or ratio_le32; n == 0 or n >= 2^32; an unknown
 * handle or one that is not a scalar set; a range [first, first + n) beyond its set; first_out != 0 with a new handle; a
 * partial overlap of the destination with an input.  MSMZ_ERR_RANGE: a broadcast coefficient, base or ratio >= q (checked
 * on the host, nothing is launched), or a resident entry >= q inside an addressed range (found by the kernel; entries
 * outside the ranges are not read).  After MSMZ_ERR_RANGE no handle is created, *out_handle is as it was, the context
 * stays usable and the contents of an in-place destination range are unspecified (as after msmz_import_scalars_into).
 * Each call returns after the GPU has finished, behind one host wait.
 * Multi-device contexts: sets are dealt in blocks of 2^16 entries, so entry i of every operand lives on one device only
 * when every first is 0.  combine then runs per engine into a new handle or over a WHOLE existing one (n its length), dot
 * runs per engine and the host adds the engines' sums mod q, powers deals its entries like msmz_random_scalars; any
 * non-zero first, or a destination of another length, is MSMZ_ERR_UNSUPPORTED there.  Like the rest of the multi-device
 * code this has run as several engines on ONE GPU only. */
typedef struct msmz_scalar_term {   /* c (.) v */
  uint64_t handle;         /* v: a scalar handle ... */
  uint64_t first;          /* ... and its first entry */
  uint64_t coeff_handle;   /* c as a resident vector, or 0 = one scalar for all i (`coeff`) */
  uint64_t coeff_first;
  const uint8_t* coeff;    /* 32 bytes little-endian, < q; read only when coeff_handle == 0; NULL = 1 */
} msmz_scalar_term;
int msmz_scalars_combine(msmz_ctx* ctx, const msmz_scalar_term* x, const msmz_scalar_term* y, uint64_t n,
                         uint64_t first_out, uint64_t* out_handle);
int msmz_scalars_dot(msmz_ctx* ctx, uint64_t x_handle, uint64_t first_x, uint64_t y_handle, uint64_t first_y, uint64_t n,
                     uint8_t* out_le32);
int msmz_scalars_powers(msmz_ctx* ctx, const uint8_t* base_le32, const uint8_t* ratio_le32, uint64_t n, uint64_t* handle);

/* What is sequential in the index, and inversion, over resident scalar sets.
 *
 * msmz_scalars_recurrence: the first-order linear recurrence y_i = a_i * y_(i-1) + b_i mod q, i = 0 .. n-1, from
 * y_(-1) = init; with MSMZ_REC_REVERSE y_i = a_i * y_(i+1) + b_i, i = n-1 .. 0, from y_n = init.  Output entry
 * first_out + i is y_i; with MSMZ_REC_EXCLUSIVE it is the value the step at i started from (y_(i-1) forward, y_(i+1)
 * reverse), so the first entry in scan order is init.  last_le32 (nullable) receives the final y (y_(n-1) forward, y_0
 * reverse), the same with or without EXCLUSIVE; it comes back in the copy that brings the error word: one host wait.
 *
 *   use                  multiplier           addend         flags                 result
 *   prefix sums          a NULL               b resident     -                     running sums
 *   prefix products      a resident           none           -                     running products
 *   grand product        a resident           none           EXCLUSIVE             Z_0 = 1, Z_(i+1) = Z_i a_i; last = the full product
 *   division by X - z    a = z (broadcast)    b = p          REVERSE | EXCLUSIVE   entry i = coefficient i of the quotient
 *                                                                                  (entry n-1 = 0); last = p(z)
 * The quotient of the last row is a scalar set of n entries: an MSM takes it against the same n points as p.
 * A broadcast multiplier without an addend gives init * a^(i+1).  No multiplier and no addend is MSMZ_ERR_ARG.
 *
 * msmz_scalars_inverse: out_i = x_i^-1 mod q over entries [first, first + n) of `handle`; 0 -> 0 (the convention of
 * arkworks' batch_inversion), and *n_zero (nullable) receives the number of zero entries in the range.
 *
 * Output, errors and in-place operation are those of msmz_scalars_combine: *out_handle == 0 makes a new handle of n
 * entries (first_out must be 0), otherwise [first_out, first_out + n) of that handle is overwritten and nothing else;
 * the destination may coincide exactly with an input range or be disjoint from it, a partial overlap is MSMZ_ERR_ARG;
 * results are below q.  MSMZ_ERR_ARG before any launch: a null ctx, r or out_handle; n == 0 or n >= 2^32; unknown flag
 * bits; an unknown handle or one that is not a scalar set; a range beyond its set.  MSMZ_ERR_RANGE: a broadcast a or
 * init >= q (found on the host, nothing is launched) or a resident entry >= q inside an addressed range (found by the
 * kernel; entries outside are not read); then no handle is created, *out_handle, *last_le32 and *n_zero are as they
 * were and an in-place destination is unspecified.
 * Multi-device contexts: inverse is element-wise and takes the route of combine (every first 0, a new handle or a
 * whole existing one; anything else MSMZ_ERR_UNSUPPORTED).  recurrence is MSMZ_ERR_UNSUPPORTED there: consecutive
 * blocks of 2^16 entries live on different devices and the dependency crosses every block boundary. */
enum { MSMZ_REC_REVERSE = 1, MSMZ_REC_EXCLUSIVE = 2 };
typedef struct msmz_scalar_rec {
  uint64_t a_handle, a_first;  /* multipliers a_i as a resident range, or a_handle == 0: one scalar `a` for every i */
  const uint8_t* a;            /* 32 bytes little-endian, < q; read only when a_handle == 0; NULL = 1 */
  uint64_t b_handle, b_first;  /* addends b_i as a resident range, or b_handle == 0: none (b_i = 0) */
  const uint8_t* init;         /* the value before the first step; NULL = 0 with an addend, 1 without one */
  uint32_t flags;              /* MSMZ_REC_* */
} msmz_scalar_rec;
int msmz_scalars_recurrence(msmz_ctx* ctx, const msmz_scalar_rec* r, uint64_t n, uint64_t first_out,
                            uint64_t* out_handle, uint8_t* last_le32);
int msmz_scalars_inverse(msmz_ctx* ctx, uint64_t handle, uint64_t first, uint64_t n, uint64_t first_out,
                         uint64_t* out_handle, uint64_t* n_zero);

/* Number-theoretic transforms over resident scalar sets: a polynomial goes from coefficient
 * form to evaluation form and back without leaving the device.
 *
 * msmz_scalars_ntt runs `count` transforms of length n = 2^log_n.  Input vector k is entries [first + k * n_in,
 * first + (k + 1) * n_in) of `handle`, continued with zeros to n entries; output vector k is entries [first_out + k * n,
 * first_out + (k + 1) * n).  Input and output are in natural order, always.
 *   forward:  out_k = sum_i x_i (g w^k)^i            (g = 1 without MSMZ_NTT_COSET)
 *   inverse:  x_i = g^-i n^-1 sum_k X_k w^(-i k)      (MSMZ_NTT_INVERSE; n_in must be n or 0)
 * inverse(forward(x)) == x byte for byte.  Results are below q, like everything the scalar-set calls write.
 * w is `root`, a primitive n-th root of unity (the host checks root^(n/2) == q - 1, for n = 1 root == 1), or with
 * root == NULL the default root that msmz_scalars_root_of_unity returns: W^(2^(S - log_n)) with S the 2-adicity of q - 1
 * and W = G^((q - 1) / 2^S), G = 22 (BLS12-377), 5 (Pallas), 7 (BLS12-381), 5 (ed-on-bls12-377): quadratic
 * non-residues, believed (not verified against those libraries) to be the generators arkworks, pasta_curves and
 * bls12_381 use; pass `root` if your stack's differs.  S = 47, 32, 32 and 1 in that order, so ed-on-bls12-377 has
 * transforms of length 1 and 2 only.
 *
 * Output, in-place operation and errors follow msmz_scalars_combine.  *out_handle == 0 makes a new set of count * n
 * entries (first_out must be 0); otherwise [first_out, first_out + count * n) of that handle is overwritten and nothing
 * else.  The whole source range [first, first + count * n_in) and the whole destination range are disjoint, or, with
 * n_in == n, the same range (in place); anything between is MSMZ_ERR_ARG.
 * MSMZ_ERR_ARG before any launch: a null ctx, t or out_handle; unknown flag bits; count == 0; count * n >= 2^32;
 * n_in > n; n_in != n with MSMZ_NTT_INVERSE; shift without MSMZ_NTT_COSET or the flag without shift; a zero shift; an
 * unknown handle or one that is not a scalar set; a range beyond its set; first_out != 0 with a new handle; a root that
 * is not a primitive n-th root of unity.  MSMZ_ERR_RANGE: root or shift >= q (found on the host, nothing is launched),
 * or a resident entry >= q inside the source range (found by the first pass, which reads every addressed entry;
 * entries outside are not read); then no handle is created, *out_handle is as it was, an in-place destination is
 * unspecified and the context stays usable.  MSMZ_ERR_UNSUPPORTED: log_n > S; or a multi-device context -- the
 * butterflies cross every boundary between blocks of 2^16 entries (the stance of msmz_scalars_recurrence).
 * One host wait per call.  A transform of more than 2^10 entries goes through scratch memory of the engine, count * n
 * entries for up to 2^16 and twice that above; it grows on demand and is kept.  The twiddle tables (about 3 sqrt(n)
 * entries) of the last eight (log_n, root, direction) are kept too. */
enum { MSMZ_NTT_INVERSE = 1, MSMZ_NTT_COSET = 2 };
typedef struct msmz_ntt {
  uint64_t handle, first;  /* input: `count` vectors of n_in entries each, vector k at first + k * n_in */
  uint32_t log_n;          /* transform length n = 2^log_n */
  uint32_t flags;          /* MSMZ_NTT_* */
  uint64_t n_in;           /* entries read per vector, 1 <= n_in <= n; the rest count as 0.  0 means n.
                              Must be n (or 0) with MSMZ_NTT_INVERSE */
  uint32_t count;          /* number of transforms, >= 1; output vector k at first_out + k * n */
  const uint8_t* root;     /* nullable: a primitive n-th root of unity, 32 bytes LE, < q.  NULL = the default root */
  const uint8_t* shift;    /* MSMZ_NTT_COSET: the coset shift g != 0, 32 bytes LE, < q; must be NULL without the flag */
} msmz_ntt;
int msmz_scalars_ntt(msmz_ctx* ctx, const msmz_ntt* t, uint64_t first_out, uint64_t* out_handle);
/* the default primitive 2^log_n-th root of unity of a curve's scalar field; needs no context.  MSMZ_ERR_ARG: an unknown
 * curve or a null pointer; MSMZ_ERR_UNSUPPORTED: log_n > S */
int msmz_scalars_root_of_unity(int curve_id, uint32_t log_n, uint8_t* out_le32);

/* Multilinear polynomials over resident scalar sets: eq tables, evaluation, binding one variable
 * and the round polynomial of a sumcheck, so that a Spartan / HyperPlonk / GKR prover or a multilinear opening keeps its
 * tables on the device between its MSMs.  The reference has no analogue.
 *
 * Conventions.  A multilinear polynomial in v variables is a range of n = 2^v entries of a scalar handle; entry i is
 * f(b_0, .., b_(v-1)) with i = sum_j b_j 2^j, so variable 0 is the lowest index bit.  v <= 31 (a set has fewer than 2^32
 * entries); v = 0 is a constant.  eq(r, i) = prod_j (b_j r_j + (1 - b_j)(1 - r_j)).  Points and challenges are 32-byte
 * little-endian values below q from the host, a point of v variables v of them in a row, r_0 first.  Everything written
 * is below q; sums are exact mod q, so two calls return the same bytes whatever the order of the reduction.
 *
 * msmz_scalars_eq_table: a new scalar handle of 2^n_vars entries, entry i = scale * eq(r, i) (scale NULL = 1).
 * n_vars == 0 gives one entry equal to scale, and point_le32 may then be NULL.
 *
 * msmz_scalars_mle_eval: f(r) = sum_i f_i eq(r, i) over entries [first, first + 2^n_vars) of `handle`, as 32 bytes.  The
 * table is not materialised; the bytes are those of msmz_scalars_dot against msmz_scalars_eq_table(r).
 *
 * msmz_scalars_mle_bind: binds one variable of `count` tables to r.  Input table k is entries [first + k 2^v,
 * first + (k + 1) 2^v) of `handle`, output table k entries [first_out + k 2^(v-1), first_out + (k + 1) 2^(v-1)).
 *   default (the high variable, v - 1):   out_i = f_i + r (f_(i+h) - f_i),  h = 2^(v-1)
 *   MSMZ_MLE_LOW (variable 0):            out_i = f_(2i) + r (f_(2i+1) - f_(2i))      (arkworks' fix_variables order)
 * One Montgomery product per output.  *out_handle == 0 makes a new handle of count 2^(v-1) entries (first_out must be 0);
 * otherwise only the destination range is written.  With count == 1 and the high variable the destination may be
 * exactly the low half of the source, [first, first + h) of the same handle (in place), or disjoint from the whole
 * source.  Every other overlap of the destination with the source is MSMZ_ERR_ARG: any with MSMZ_MLE_LOW or count > 1,
 * the high half, a partial overlap with either half.
 *
 * msmz_scalars_sumcheck_round: with tables f_0 .. f_(n_tables-1), each 2^v entries from tables[j].first of
 * tables[j].handle, and terms T = (c_T, mask_T), bit j of the mask making f_j a factor ("a list of products of
 * multilinear polynomials"; Spartan's eq (A B - C) is two terms over four tables), d = the largest popcount of a mask:
 *   g(t) = sum_(i < 2^(v-1)) sum_T c_T prod_(j in T) ((1 - t) f_j[lo(i)] + t f_j[hi(i)]),   t = 0 .. d
 * with (lo, hi) = (i, i + 2^(v-1)): the round sums out the high variable; MSMZ_MLE_LOW: (2i, 2i + 1), variable 0.
 * *degree = d and evals_le32 receives d + 1 values of 32 bytes; it has room for (MSMZ_SUMCHECK_MAX_DEGREE + 1) * 32
 * bytes and the bytes beyond d + 1 values are left as they were.  Tables may share a handle and may overlap.  A prover's
 * round: sumcheck_round, a challenge from its transcript, mle_bind of every table with the same flag, n_vars - 1.
 *
 * MSMZ_ERR_ARG, before any launch: a null ctx, descriptor, point (n_vars > 0), r, tables, terms or output pointer;
 * n_vars > 31, or 0 where bind and sumcheck_round need >= 1; unknown flag bits; an unknown handle or one that is not a
 * scalar set; a range beyond its set; count == 0 or count 2^v >= 2^32; n_tables outside 1 .. MSMZ_SUMCHECK_MAX_TABLES;
 * n_terms outside 1 .. MSMZ_SUMCHECK_MAX_TERMS; a mask that is 0, has bits at or above n_tables or more than
 * MSMZ_SUMCHECK_MAX_DEGREE of them; first_out != 0 with a new handle; the overlaps above.  MSMZ_ERR_RANGE: a host value
 * (point, scale, r, coefficient) >= q, found on the host with nothing launched; or a resident entry >= q inside an
 * addressed range, found by the kernel (entries outside are not read): then no handle is created, *out_handle, *degree
 * and the output bytes are as they were, an in-place destination is unspecified and the context stays usable.
 * MSMZ_ERR_UNSUPPORTED: a multi-device context -- the two halves of every pair live in different blocks of 2^16 entries
 * (the stance of msmz_scalars_recurrence).  Each call returns behind one host wait. */
enum { MSMZ_MLE_LOW = 1 };
enum { MSMZ_SUMCHECK_MAX_TABLES = 6, MSMZ_SUMCHECK_MAX_DEGREE = 4, MSMZ_SUMCHECK_MAX_TERMS = 8 };
typedef struct msmz_mle_bind {
  uint64_t handle, first;  /* `count` tables of 2^n_vars entries each, table k at first + k * 2^n_vars */
  uint32_t n_vars;         /* >= 1 */
  uint32_t count;          /* >= 1 */
  uint32_t flags;          /* MSMZ_MLE_LOW or 0 */
  const uint8_t* r;        /* the challenge, 32 bytes little-endian, < q */
} msmz_mle_bind;           /* 40 bytes */
typedef struct msmz_sumcheck_table {
  uint64_t handle, first;
} msmz_sumcheck_table;
typedef struct msmz_sumcheck_term {
  const uint8_t* coeff;    /* 32 bytes little-endian, < q; NULL = 1 */
  uint32_t mask;           /* bit j: table j is a factor */
} msmz_sumcheck_term;      /* 16 bytes */
typedef struct msmz_sumcheck {
  const msmz_sumcheck_table* tables;
  uint32_t n_tables;       /* 1 .. MSMZ_SUMCHECK_MAX_TABLES */
  uint32_t n_vars;         /* >= 1 */
  const msmz_sumcheck_term* terms;
  uint32_t n_terms;        /* 1 .. MSMZ_SUMCHECK_MAX_TERMS */
  uint32_t flags;          /* MSMZ_MLE_LOW or 0: the variable the round sums out */
} msmz_sumcheck;           /* 32 bytes */
int msmz_scalars_eq_table(msmz_ctx* ctx, const uint8_t* point_le32, uint32_t n_vars, const uint8_t* scale_le32,
                          uint64_t* handle);
int msmz_scalars_mle_eval(msmz_ctx* ctx, uint64_t handle, uint64_t first, uint32_t n_vars, const uint8_t* point_le32,
                          uint8_t* out_le32);
int msmz_scalars_mle_bind(msmz_ctx* ctx, const msmz_mle_bind* b, uint64_t first_out, uint64_t* out_handle);
int msmz_scalars_sumcheck_round(msmz_ctx* ctx, const msmz_sumcheck* s, uint32_t* degree, uint8_t* evals_le32);

/* msmz_scalars_sumcheck_step: one step of a sumcheck prover in one call -- every table of round k
 * is bound to the challenge r_k and the polynomial of round k + 1 comes back, behind one host wait.  A prover's loop is
 * msmz_scalars_sumcheck_round once, then one step per challenge; the tables are read once and the bound tables written
 * once, where mle_bind per table followed by sumcheck_round reads the bound tables again.
 *
 * With source tables f_0 .. f_(n_tables-1) of v = n_vars variables (tables[j]: 2^v entries from `first` of `handle`),
 * destinations out_0 .. (out[j]: 2^(v-1) entries from `first` of `handle`, an EXISTING scalar set; msmz_alloc_scalars
 * makes one -- the call creates no handle), the challenge r and the order `flags` names for BOTH halves of the step:
 *   1. Bind.  out_j receives exactly what msmz_scalars_mle_bind writes for table j (count 1) with the same r and flag.
 *   2. Next round.  *degree and evals_le32 receive exactly what msmz_scalars_sumcheck_round returns over out_0 ..
 *      (n_vars - 1 variables) with the same terms and flag: byte for byte the result of the two-call route.
 *   3. Last variable, n_vars == 1.  The bound tables have one entry each and no variable is left to sum: *degree = 0 and
 *      the one value is sum_T c_T prod_(j in T) out_j[0], the final claim the verifier checks (the round body on a pair
 *      with hi = lo and degree 0).
 * evals_le32 has room for (MSMZ_SUMCHECK_MAX_DEGREE + 1) * 32 bytes; the bytes beyond *degree + 1 values stay as they were.
 *
 * Destinations.  out == NULL: every table in place, out_j = the low half [first, first + 2^(v-1)) of its own source.
 * A destination range is disjoint from every other destination range and from the source range of every OTHER table
 * index; against its own source it is disjoint, or exactly the source's low half -- and that only in the high order
 * (flags == 0).  Every other overlap is MSMZ_ERR_ARG before any launch: the high half, a partial overlap, any in-place
 * destination with MSMZ_MLE_LOW (out == NULL included).  Sources may overlap each other as far as these rules allow (two
 * tables may be one range when their destinations are apart from it and from each other).
 *
 * Errors, as the four calls above.  MSMZ_ERR_ARG, before any launch: a null ctx, descriptor, tables, terms, r or output
 * pointer; n_vars == 0 or > 31; unknown flag bits; n_tables, n_terms or a mask outside the limits of sumcheck_round; an
 * unknown handle or one that is not a scalar set; a source or destination range beyond its set; the overlaps above.
 * MSMZ_ERR_RANGE: r or a coefficient >= q, found on the host with nothing launched; or a resident entry >= q inside a
 * source range, found by the kernel (entries outside are not read): then *degree and the output bytes are as they were,
 * the destinations are unspecified and the context stays usable.  MSMZ_ERR_UNSUPPORTED: a multi-device context. */
typedef struct msmz_sumcheck_step {
  const msmz_sumcheck_table* tables;  /* sources: n_tables ranges of 2^n_vars entries */
  const msmz_sumcheck_table* out;     /* destinations: n_tables ranges of 2^(n_vars-1) entries of EXISTING scalar
                                         sets; NULL = every table in place (its own low half; high order only) */
  uint32_t n_tables;                  /* 1 .. MSMZ_SUMCHECK_MAX_TABLES */
  uint32_t n_vars;                    /* >= 1: the variables the SOURCE tables have */
  const msmz_sumcheck_term* terms;
  uint32_t n_terms;                   /* 1 .. MSMZ_SUMCHECK_MAX_TERMS */
  uint32_t flags;                     /* MSMZ_MLE_LOW or 0: the order of BOTH the bind and the round */
  const uint8_t* r;                   /* the challenge for the variable bound, 32 bytes LE, < q */
} msmz_sumcheck_step;                 /* 48 bytes */
int msmz_scalars_sumcheck_step(msmz_ctx* ctx, const msmz_sumcheck_step* s, uint32_t* degree, uint8_t* evals_le32);

/* Sparse matrices over resident scalar sets: y = M x and y = M^T x mod q with the matrix and both
 * vectors on the device -- the step from a witness z to Az, Bz, Cz of an R1CS, the table of Spartan's second sumcheck
 * (r_A A + r_B B + r_C C)^T eq(r_x), the QAP evaluations of Groth16, and any gather, selection or permutation of a
 * scalar range (a 0/1 matrix with one entry per row).  The reference has no analogue.
 *
 * A matrix is a third kind of handle.  msmz_matrix_create builds it from nnz triples (row[k], col[k], val[k]) in any
 * order; triples with the same (row, col) are kept apart and add up in the product.  The indices come from host memory,
 * the values from entries [val_first, val_first + nnz) of a scalar handle, value k belonging to triple k; with
 * val_handle == 0 every value is 1 (val_first must then be 0) and the product adds entries of x without multiplying.
 * `flags` names the orientations to build: MSMZ_MAT_ROWS for the plain product, MSMZ_MAT_COLS for the transposed one,
 * both, or 0 = MSMZ_MAT_ROWS.  Each orientation costs a sort on the host, O(nnz + n_rows + n_cols), and 8 bytes per
 * non-zero on the device plus 32 per value.  The matrix copies what it needs: the index arrays and the value set may be
 * changed or freed once the call has returned.  msmz_matrix_info reports what a matrix handle holds (every output
 * pointer nullable; *flags = the orientations built).  msmz_free frees a matrix; every other call that is handed a
 * matrix handle answers MSMZ_ERR_ARG, as for any handle of the wrong kind.
 *
 * msmz_matrix_mul:   out_i = sum over {k : row[k] == i} of val[k] * x[col[k]] mod q,   i < n_rows,
 * with x = entries [x_first, x_first + n_cols) of x_handle; a row without a triple gives 0.  MSMZ_MATVEC_TRANSPOSE swaps
 * the roles of row and col: x has n_rows entries and the result n_cols.  The plain product needs a matrix built with
 * MSMZ_MAT_ROWS, the transposed one MSMZ_MAT_COLS; asking for the other is MSMZ_ERR_ARG.  Every entry written is below q;
 * the sums are exact mod q, so two calls return the same bytes whatever the grouping of the additions.  The output rules
 * are those of msmz_scalars_combine: *out_handle == 0 makes a new set of n_rows (n_cols) entries and first_out must be
 * 0; otherwise only [first_out, first_out + n_rows) of that handle is written.  Because x is gathered, a destination
 * that meets the x range of the same handle anywhere, the exact range included, is MSMZ_ERR_ARG.
 *
 * MSMZ_ERR_ARG, before any launch: a null ctx, descriptor, row, col or output pointer; nnz == 0 or nnz >= 2^32; n_rows or
 * n_cols == 0; an index out of range (the triples are looked at in the caller's order and the first bad one decides,
 * its row before its column; nothing beyond the status is reported); unknown flag bits; an unknown handle or one of
 * the wrong kind; a range beyond its set; val_first != 0 without a value set; first_out != 0 with a new handle; the
 * orientation and the overlap above.  MSMZ_ERR_RANGE from msmz_matrix_create: a value >= q inside [val_first,
 * val_first + nnz), found by the kernel that packs the values (entries outside are not read).  MSMZ_ERR_RANGE from
 * msmz_matrix_mul: an entry of x that some non-zero reads is >= q; entries of x that no non-zero references are not
 * read.  After MSMZ_ERR_RANGE no handle is created, *handle / *out_handle is as it was, an in-place destination is
 * unspecified and the context stays usable.  MSMZ_ERR_HIP from msmz_matrix_create also covers host memory the sort
 * could not get (12 nnz + 8 max(n_rows, n_cols) bytes).  MSMZ_ERR_UNSUPPORTED: a multi-device context -- a gather reads
 * across every block of 2^16 entries (the stance of msmz_scalars_recurrence).  One host wait per call. */
enum { MSMZ_MAT_ROWS = 1, MSMZ_MAT_COLS = 2 };
enum { MSMZ_MATVEC_TRANSPOSE = 1 };
typedef struct msmz_sparse {
  const uint32_t* row;             /* host memory, nnz entries, each < n_rows */
  const uint32_t* col;             /* host memory, nnz entries, each < n_cols */
  uint64_t val_handle, val_first;  /* values: entries [val_first, val_first + nnz) of a scalar set; val_handle == 0: every value is 1 */
  uint64_t nnz;                    /* 1 .. 2^32 - 1 */
  uint32_t n_rows, n_cols;         /* >= 1 */
  uint32_t flags;                  /* MSMZ_MAT_ROWS | MSMZ_MAT_COLS; 0 means MSMZ_MAT_ROWS */
} msmz_sparse;                     /* 56 bytes */
typedef struct msmz_matvec {
  uint64_t matrix;
  uint64_t x_handle, x_first;      /* x: n_cols entries (n_rows with MSMZ_MATVEC_TRANSPOSE) of a scalar set */
  uint32_t flags;                  /* MSMZ_MATVEC_TRANSPOSE or 0 */
} msmz_matvec;                     /* 32 bytes */
int msmz_matrix_create(msmz_ctx* ctx, const msmz_sparse* s, uint64_t* handle);
int msmz_matrix_info(msmz_ctx* ctx, uint64_t handle, uint32_t* n_rows, uint32_t* n_cols, uint64_t* nnz, uint32_t* flags);
int msmz_matrix_mul(msmz_ctx* ctx, const msmz_matvec* v, uint64_t first_out, uint64_t* out_handle);

/* Lookup arguments: the multiplicities of a column in a table.  For a table t = entries
 * [table_first, table_first + table_n) of a scalar set and a column f = entries [col_first, col_first + col_n) of one,
 * msmz_scalars_lookup makes the vector m that a logUp argument (Halo2 lookups, Plonky3, Lasso's offline memory
 * checking) commits to, with nothing but the result words crossing to the host.  The reference has no analogue.
 *
 * The output is a scalar set of table_n entries, each a canonical 32-byte value:
 *     m_j = #{ i < col_n : f_i = t_j }   if j is the lowest index among the table entries that hold the value t_j,
 *     m_j = 0                            for every later duplicate of a table value.
 * With that rule  sum_j m_j / (beta + t_j) = sum_i 1 / (beta + f_i)  holds whenever n_missing == 0, and the result does
 * not depend on any execution order: two calls return the same bytes.  Values are compared as integers below q.
 *
 * A query, not a check (the stance of msmz_check_points): a column entry that equals no table entry is not an error.
 * The call returns MSMZ_OK with the counts of what was found and, if `res` is given, n_missing, first_missing and
 * n_distinct.  If `positions` is given, positions[i] = the index, relative to table_first, of the FIRST table entry
 * equal to f_i, 0xffffffff where there is none.
 *
 * The output rules are those of msmz_scalars_combine: *out_handle == 0 makes a new set of table_n entries and first_out
 * must be 0; otherwise only [first_out, first_out + table_n) of that handle is written.  One exception: both inputs are
 * gathered, so a destination that meets the table range or the column range of the same handle anywhere, the exact
 * range included, is MSMZ_ERR_ARG.  Table and column may share a handle and may overlap each other.
 *
 * MSMZ_ERR_ARG, before any launch: a null ctx, descriptor or out_handle; table_n == 0, col_n == 0, table_n > 2^30 or
 * col_n >= 2^32; non-zero flags; an unknown handle or one that is not a scalar set; a range beyond its set; first_out
 * != 0 with a new handle; the overlap above.  MSMZ_ERR_RANGE: a resident entry >= q inside either addressed range,
 * found by the kernels (entries outside the ranges are not read); no handle is created, *out_handle, *res and
 * positions are as they were, an in-place destination is unspecified and the context stays usable.
 * MSMZ_ERR_UNSUPPORTED: a multi-device context -- a probe reads across every block of 2^16 entries (the stance of
 * msmz_matrix_mul).  Device scratch: 4 S bytes for the index, S the power of two with 2 table_n <= S < 4 table_n, 4
 * table_n for the counts and, with positions, 4 col_n.  One host wait per call: the error word, the three result words
 * and the positions come back behind it. */
typedef struct msmz_lookup {
  uint64_t table_handle, table_first, table_n;  /* t: entries [table_first, table_first + table_n) of a scalar set */
  uint64_t col_handle, col_first, col_n;        /* f: the looked-up values */
  uint32_t* positions;   /* nullable, HOST memory, col_n words: index (relative to table_first) of the first table
                            entry equal to f_i, 0xffffffff where there is none */
  uint32_t flags;        /* must be 0 */
} msmz_lookup;           /* 64 bytes */
typedef struct msmz_lookup_result {
  uint64_t n_missing;      /* entries of f that equal no table entry */
  uint64_t first_missing;  /* the LOWEST such i (relative to col_first), ~0 if none */
  uint64_t n_distinct;     /* distinct values among the table entries */
} msmz_lookup_result;      /* 24 bytes */
int msmz_scalars_lookup(msmz_ctx* ctx, const msmz_lookup* l, uint64_t first_out, uint64_t* out_handle,
                        msmz_lookup_result* res /* nullable */);

/* Gate expressions: a sum of products of rotated columns, entry by entry.  The constraint
 * expression of a PLONK-ish prover -- q_L a + q_R b + q_M a b + q_O c + q_C, a permutation step Z(wX) prod(..) - Z(X)
 * prod(..), an S-box gate a^5 -- evaluated over columns that are ranges of resident scalar sets, in one launch, between
 * the coset NTT of the columns and the inverse NTT of the quotient.  The reference has no analogue.
 *
 *     out_i = sum over terms T of  c_T * prod over factors f of T of  col_(f.column)[(i + f.rot) mod n]   mod q,   i < n.
 *
 * Every column is a range of n entries, [first, first + n) of its handle, and a rotation is cyclic inside that range;
 * rot is any int32 and is reduced to [0, n) on the host; n need not be a power of two.  On an extended coset of size
 * 4 n' the rows of the original domain lie 4 apart: the caller passes 4 * rot.  A factor may repeat within a term
 * (a a a a a), the same column may appear at several rotations, columns may share a handle and may overlap each other.
 * A column that no factor names is not read and need not be below q.  A term without factors is the constant c_T.  The
 * operands of an expression are the distinct pairs (column, rot mod n) over all its terms; there may be at most
 * MSMZ_EXPR_MAX_OPERANDS of them.  Every value written is canonical, below q, and the sums are exact, so two calls
 * return the same bytes.
 *
 * The output rules are those of msmz_scalars_combine: *out_handle == 0 makes a new set of n entries and first_out must
 * be 0; otherwise only [first_out, first_out + n) of that handle is written.  A destination on the handle of a column
 * that some factor names: if every factor of that column has rot = 0 (mod n), the destination may be exactly the
 * column's range or lie apart from it, and a partial overlap is MSMZ_ERR_ARG; if any factor of the column is rotated,
 * the destination must not meet the column's range at all (as for the gathers of msmz_matrix_mul and
 * msmz_scalars_lookup).  A column that no factor names may overlap anything.  So accumulation needs no flag:
 * out = y * out + gate is the term (y, [out at rotation 0]) next to the gate's terms, evaluated in place.
 *
 * MSMZ_ERR_ARG, before any launch: a null ctx, descriptor, columns, terms or out_handle, or null factors with n_factors
 * != 0; n_columns, n_terms, n_factors or n outside the bounds below; a column index >= n_columns; non-zero flags or
 * reserved; more than MSMZ_EXPR_MAX_OPERANDS operands; an unknown handle or one that is not a scalar set; a range
 * beyond its set (every column's, named or not); first_out != 0 with a new handle; the overlaps above.  MSMZ_ERR_RANGE:
 * a coefficient >= q (checked on the host after all of the former; nothing is launched), or a resident entry >= q
 * inside the range of a column that some factor names, found by the kernel (entries outside are not read).  After
 * MSMZ_ERR_RANGE no handle is created, *out_handle is as it was, an in-place destination is unspecified and the context
 * stays usable.  MSMZ_ERR_UNSUPPORTED: a multi-device context when any operand is rotated -- a rotation reads across
 * the blocks of 2^16 entries; with every rotation = 0 (mod n) the call takes the element-wise route of
 * msmz_scalars_combine there: every first must be 0 and the output a new handle or a whole existing one.  One host wait
 * per call. */
enum { MSMZ_EXPR_MAX_COLUMNS = 16, MSMZ_EXPR_MAX_TERMS = 32, MSMZ_EXPR_MAX_DEGREE = 8, MSMZ_EXPR_MAX_OPERANDS = 32 };
typedef struct msmz_expr_column { uint64_t handle, first; } msmz_expr_column;          /* 16 bytes */
typedef struct msmz_expr_factor { uint32_t column; int32_t rot; } msmz_expr_factor;    /*  8 bytes */
typedef struct msmz_expr_term {
  const uint8_t* coeff;             /* 32 bytes LE, < q; NULL = 1 */
  const msmz_expr_factor* factors;  /* n_factors of them; may be NULL when n_factors == 0 */
  uint32_t n_factors;               /* 0 .. MSMZ_EXPR_MAX_DEGREE; 0 = the constant coeff */
  uint32_t reserved;                /* must be 0 */
} msmz_expr_term;                   /* 24 bytes */
typedef struct msmz_expr {
  const msmz_expr_column* columns;  /* n_columns of them, each a range of n entries */
  uint32_t n_columns;               /* 1 .. MSMZ_EXPR_MAX_COLUMNS */
  uint32_t n_terms;                 /* 1 .. MSMZ_EXPR_MAX_TERMS */
  const msmz_expr_term* terms;
  uint64_t n;                       /* 1 .. 2^32 - 1 */
  uint32_t flags;                   /* must be 0 */
} msmz_expr;                        /* 40 bytes */
int msmz_scalars_expr(msmz_ctx* ctx, const msmz_expr* e, uint64_t first_out, uint64_t* out_handle);

/* msmz_scalars_dot_many: every inner product of n_rows row vectors with n_cols column vectors in
 * one call -- the product of a dense n_rows x n matrix with a dense n x n_cols matrix mod q, n large, both counts small:
 * many committed polynomials at a few challenge points (columns = power vectors), many multilinear tables at one point
 * (one column = the eq table), Hyrax's L M, the cross terms of a folding scheme.  A vector is entries
 * [first, first + n) of the scalar set `handle`.
 *     result[r * n_cols + c] = sum_(i < n) rows[r][i] * cols[c][i] mod q,  canonical
 * Each value is byte for byte what msmz_scalars_dot(rows[r], cols[c], n) returns; the sums are exact, so two calls give
 * the same bytes.  Vectors may share handles, overlap and be one range (rows[r] == cols[c]: a sum of squares).  A column
 * value is read once per block of rows, not once per row, and the whole call has ONE host wait.
 *
 * Destinations, at least one of them: out_le32 (nullable) receives n_rows * n_cols * 32 bytes, row-major; out_handle
 * (nullable) as everywhere: *out_handle == 0 makes a new scalar set of n_rows * n_cols entries (first_out must be 0),
 * otherwise entries [first_out, first_out + n_rows * n_cols) of that set are written and no other.  A destination range
 * that meets any input range of the same handle is refused, whatever the order of the writes would be.  With
 * out_handle == NULL first_out must be 0.
 *
 * MSMZ_ERR_ARG, before any launch: a null ctx, descriptor, rows or cols; both destinations null; n_rows or n_cols
 * outside their limits; n == 0 or >= 2^32; unknown flag bits; first_out != 0 without an existing destination set; an
 * unknown handle or one that is not a scalar set; a range beyond its set; the overlap above.  MSMZ_ERR_RANGE: a resident
 * entry >= q inside an addressed range, found by the kernel: then no handle is made, *out_handle and out_le32 are as
 * they were, a destination range of an existing set is unspecified and the context stays usable.
 * MSMZ_ERR_UNSUPPORTED: a multi-device context.  A sum of one vector alone stays msmz_scalars_dot with y_handle == 0. */
enum { MSMZ_DOT_MANY_MAX_ROWS = 128, MSMZ_DOT_MANY_MAX_COLS = 8 };
typedef struct msmz_scalar_vec { uint64_t handle, first; } msmz_scalar_vec;   /* 16 bytes */
typedef struct msmz_dot_many {
  const msmz_scalar_vec* rows;
  uint32_t n_rows;              /* 1 .. MSMZ_DOT_MANY_MAX_ROWS */
  const msmz_scalar_vec* cols;
  uint32_t n_cols;              /* 1 .. MSMZ_DOT_MANY_MAX_COLS */
  uint64_t n;                   /* entries of every vector, 1 .. 2^32 - 1 */
  uint32_t flags;               /* must be 0 */
} msmz_dot_many;                /* 48 bytes */
int msmz_scalars_dot_many(msmz_ctx* ctx, const msmz_dot_many* d, uint8_t* out_le32, uint64_t first_out, uint64_t* out_handle);

/* Host-side group addition of two canonical affine results: combines per-GPU partial sums
 * (the reference's "partition sum" step, msm-batched-affine.ts:300-307). */
int msmz_point_add(int curve_id, const uint8_t* a_xy_le, int a_is_inf, const uint8_t* b_xy_le, int b_is_inf,
                   uint8_t* out_xy_le, int* out_is_inf);

#ifdef __cplusplus
}
#endif
#endif /* MSMZ_H */

/* msmz -- stage-level test hooks of the C ABI.
 *
 * The reference tests every wasm routine against its bigint twin (src/field.test.ts:159-211,
 * src/curve-projective.test.ts:77-209, src/glv/glv-test.ts:83-125, src/testing/equivalent-wasm.ts:97-147).  These
 * entry points give the parity tests the same granularity on the device: each one runs ONE device routine of the
 * MSM pipeline, or one phase of the engine (the bucket sort, the tree-round schedule, the bucket reduction), on
 * caller-supplied inputs and returns its raw output.  They are not part of the drop-in boundary and
 * never take part in an MSM (two pairs only steer and count one: msmz_test_set_glv_bits / _retries and
 * msmz_test_set_limits / _passes make ordinary inputs take the engine's rare host paths).  Statuses and conventions
 * as in msmz.h; on a multi-device context they use its first engine.
 *
 * Field elements travel as fe_bytes little-endian bytes holding a Montgomery residue in the engine's memory format
 * (radix R = 2^392 for the 377/381-bit fields, 2^261 for the 255-bit ones).  They are lazily reduced: the field ops
 * take any value in [0, 4p), wider than the [0, 3p) the kernels write and the point ops assume (the memory range is
 * stated once, in msm_zprize_amd/csrc/fp.h).  Results are canonical (< p).
 */
#ifndef MSMZ_TEST_H
#define MSMZ_TEST_H

#include "msmz.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  MSMZ_TF_MUL = 0,          /* a*b/R        (fe_mul, Montgomery product)                         */
  MSMZ_TF_SQR = 1,          /* a*a/R        (fe_sqr)                                             */
  MSMZ_TF_ADD = 2,          /* a+b          (lazy add, canonicalized on output)                  */
  MSMZ_TF_SUB = 3,          /* a-b                                                               */
  MSMZ_TF_INVERSE = 4,      /* R^2/a        (fe_inverse: per-lane binary GCD; 0 for a = 0)       */
  MSMZ_TF_INVERSE_WAVE = 5, /* R^2/a        (fe_inverse_wave: the wave-wide form of k_batch_add) */
  MSMZ_TF_ROUNDTRIP = 6,    /* a            (fe_store -> fe_unpack: the memory format)           */
  MSMZ_TF_IS_ZERO = 7,      /* a == b mod p ? 1 : 0 in byte 0  (fe_is_zero of a lazy difference) */
  MSMZ_TF_SLOT_ROUNDTRIP = 8 /* a+b after (a, b) went through a slot record of the tree rounds    */
};
enum {
  MSMZ_TP_ADD = 0,     /* accumulator + accumulator (XYZZ add / extended twisted-Edwards add), all edge cases */
  MSMZ_TP_ADD_X4 = 1,  /* the 4-lane form used by the upper reduction levels                                 */
  MSMZ_TP_MADD = 2,    /* a + b with b stored as an input record (affine / Niels) and folded in by the mixed add */
  MSMZ_TP_DBL = 3,     /* doubling of the first operand                                                      */
  MSMZ_TP_DBL_X4 = 4   /* 2 (a + b): 4-lane addition, then the 4-lane doubling of that (general) accumulator  */
};

/* field routines on RAW register limbs (msm_zprize_amd/csrc/test_ops.h): an element is N signed int32 limbs
 * (N = 14 for the 377/381-bit fields, 9 for the 255-bit ones; value = sum l[j] * 2^(W j), W = 28 / 29), loaded into
 * the registers unchanged, so the caller controls the limb form.  Operands must lie inside the routine's contract
 * (fp.h).  out_raw[i] (N int32): the output limbs, or the memory words (STORE, STORE_MULOUT), or the flag in limb 0
 * (IS_ZERO); out_canon[i] (fe_bytes): the canonical value of that output (0 for IS_ZERO, CARRY, NORMALIZE).
 * SLOT_MULOUT parks a mul output in a slot record and loads it back (out_raw = loaded limbs); SLOT_POINT stores (a, b)
 * as a slot point record and loads it back (out_raw = the limbs of y, out_canon = x). */
enum {
  MSMZ_TFL_MUL = 0, MSMZ_TFL_SQR = 1, MSMZ_TFL_REDUCE_SMALL = 2, MSMZ_TFL_STORE = 3, MSMZ_TFL_STORE_MULOUT = 4,
  MSMZ_TFL_IS_ZERO = 5, MSMZ_TFL_CARRY = 6, MSMZ_TFL_NORMALIZE = 7, MSMZ_TFL_INVERSE = 8, MSMZ_TFL_INVERSE_WAVE = 9,
  MSMZ_TFL_SLOT_MULOUT = 10, MSMZ_TFL_SLOT_POINT = 11
};
int msmz_test_field_limbs(msmz_ctx* ctx, int op, const int32_t* a, const int32_t* b, uint64_t n, int32_t* out_raw,
                          uint8_t* out_canon);
/* The row form of the field routines (msm_zprize_amd/csrc/fp_rows.h): an element is spread over the 16 lanes of a DPP
 * row, limb j in lane j, and the four rows of a wave run four elements at once.  Operands and outputs are raw limbs as
 * for msmz_test_field_limbs.  MUL: out_raw = the limbs of fe_mul_row(a, b), out_canon its canonical value (through
 * fe_store_row).  ROUNDTRIP: the first NW int32 of a[i] are memory words; out_raw = the words after fe_load_row ->
 * fe_store_row (the rest zero), out_canon their canonical value.  IS_ZERO: out_raw[0] = fe_is_zero_row(a), out_canon 0.
 * live_rows (1 .. 15): a wave takes one element in each row whose bit is set and runs the other rows on zero operands;
 * 15 = four elements per wave. */
enum { MSMZ_TFR_MUL = 0, MSMZ_TFR_ROUNDTRIP = 1, MSMZ_TFR_IS_ZERO = 2 };
int msmz_test_field_rows(msmz_ctx* ctx, int op, const int32_t* a, const int32_t* b, uint64_t n, uint32_t live_rows,
                         int32_t* out_raw, uint8_t* out_canon);

/* GLV half-scalar bound (src/wasm/glv.ts:216-226 `maxBits`).  The engine sizes the windows for halves below 2^127 and
 * lets the slicing kernel flag a longer half, in which case the MSM is redone with windows for the analytic bound
 * (GLV_PROVEN_BITS, tools/gen_constants.py).  No scalar below the group order can take that path: the exact supremum
 * of the halves is below 2^127 on all three curves (oracle/glv_edges.py supremum, pinned by
 * tests/test_glv_edges_cpu.py::test_supremum_facts).  The path stays as a guard, so this hook shrinks the
 * ASSUMED bit length (8 .. 127; 0 restores the default): ordinary halves then overflow, the flag is raised and the
 * redone MSM must still equal the oracle.  msmz_test_retries = number of MSMs (per-engine passes) redone so far. */
int msmz_test_set_glv_bits(msmz_ctx* ctx, int bits);
int msmz_test_retries(msmz_ctx* ctx);
/* The engine cuts a call into several device pipelines at two size limits, which ordinary test inputs never reach:
 * one index-range pass sorts at most 2^24 (half-)scalars, the partial sums of the passes folded on the host, and one
 * batched pass takes at most 2^26 entries, a longer batch running as consecutive sub-batches.
 * Lower the engine's two size limits for later calls on this context; 0 = the built-in value.
 *   pass_entries : (half-)scalars one index-range pass takes, 2 .. 2^24 (kMaxEntriesPerPass);
 *                  with GLV a pass takes pass_entries / 2 points, as with the built-in value.
 *   batch_entries: entries (problems x K x M) one batched pass takes, 1 .. 2^26 (kMaxBatchEntries).
 * MSMZ_ERR_ARG outside those ranges. The limits can only be lowered. Neither changes a result.  A precomputed set
 * longer than a lowered pass limit is not supported (production refuses such sets at 2^24). */
int msmz_test_set_limits(msmz_ctx* ctx, uint64_t pass_entries, uint64_t batch_entries);
/* Totals since the context was created (either pointer nullable; a multi-device context: summed over its engines):
 *   range_passes: iterations of run_problems' range loop (an ordinary single-problem MSM adds 1);
 *   sub_batches : batched pipelines (more than one problem) that ran to a result (not PER_PROBLEM). */
int msmz_test_passes(msmz_ctx* ctx, uint64_t* range_passes, uint64_t* sub_batches);
/* Scratch is undefined at the start of every call: this makes it so.  pattern 0..255:
 *   (a) fills every device scratch buffer the context's engines own with the byte, over its whole capacity (the
 *       allocation's headroom included), on the engine's stream, and waits;
 *   (b) arms the context: from now on every device buffer that is newly allocated -- scratch that grows, the memory of
 *       every new handle (result sets, precomputed sets, matrix forms), a new cached table -- is filled with the byte
 *       before anything else touches it.
 * pattern -1 disarms (and fills nothing); any other value is MSMZ_ERR_ARG, as is a null context.  Not filled by (a),
 * because they hold what stays valid across calls: the records of existing handles, the twiddle and fixed-base table
 * caches, the generator table; pinned host memory is outside the hook.  *buffers / *bytes (either nullable): the
 * buffers of non-zero capacity that (a) filled and the bytes written; a multi-device context: summed over its engines.
 * Launches nothing but memsets; a context never armed pays one test of a flag where a buffer is allocated. */
int msmz_test_poison(msmz_ctx* ctx, int pattern, uint64_t* buffers, uint64_t* bytes);
/* What fill (a) of msmz_test_poison would write on engine `engine` (0 .. msmz_ctx_n_devices - 1) of the context alone,
 * without writing it: its scratch buffers of non-zero capacity and their bytes (either pointer nullable).  So a test can
 * hold the sums that a multi-device context reports against its engines' own counts.  MSMZ_ERR_ARG: a null context, no
 * such engine. */
int msmz_test_scratch(msmz_ctx* ctx, int engine, uint64_t* buffers, uint64_t* bytes);
/* The geometry of msmz_scalars_dot (csrc/scalar_kernels.h), so a test can size itself at its edges (either pointer
 * nullable; needs no context):
 *   tile_elements    : elements one workgroup of the first level sums into one partial sum (SDOT_TILE);
 *   partials_per_pass: partial sums the second level's one workgroup takes per pass of its loop (SDOT_PASS). */
void msmz_test_scalar_dot_geometry(uint32_t* tile_elements, uint32_t* partials_per_pass);
/* The geometry of msmz_scalars_recurrence and msmz_scalars_inverse (csrc/scan_kernels.h), for the same purpose (every
 * pointer nullable; needs no context):
 *   rec_tile : scan positions one workgroup composes into one aggregate map (SREC_TILE);
 *   rec_pass : tile aggregates the one workgroup of the carry launch takes per pass of its loop (SREC_PASS);
 *   inv_chunk: elements that share one field inversion, one wave's share (SINV_CHUNK). */
void msmz_test_scalar_scan_geometry(uint32_t* rec_tile, uint32_t* rec_pass, uint32_t* inv_chunk);
/* The plan of msmz_scalars_ntt for a transform of 2^log_n entries (csrc/ntt_plan.h), so a test can size itself at the
 * edges of the plan; neither call needs a context.
 *   msmz_test_ntt_plan: *n_passes = the launches of the transform, stages[j] = the stages pass j runs in LDS (8 words,
 *     zero beyond n_passes); their sum is log_n.  MSMZ_ERR_ARG: an unknown curve, a null pointer or log_n > 32;
 *     MSMZ_ERR_UNSUPPORTED: log_n above the 2-adicity of the curve's scalar field.
 *   msmz_test_ntt_geometry: *pass_log = the most stages one pass runs (NTT_PASS_LOG; a tile is 2^pass_log entries). */
int msmz_test_ntt_plan(int curve_id, uint32_t log_n, uint32_t* n_passes, uint32_t* stages);
void msmz_test_ntt_geometry(uint32_t* pass_log);
/* The geometry of the multilinear calls (csrc/mle_kernels.h), for the same purpose (every pointer nullable; needs no
 * context):
 *   run       : consecutive eq values one thread of msmz_scalars_eq_table / _mle_eval owns (MLE_RUN);
 *   eval_tile : entries one workgroup of msmz_scalars_mle_eval sums into one partial sum (MLE_TILE);
 *   round_tile: pair indices one workgroup of msmz_scalars_sumcheck_round sums into one partial sum per value
 *               (MSC_TILE).  The second level of both is that of msmz_scalars_dot (partials_per_pass above). */
void msmz_test_mle_geometry(uint32_t* run, uint32_t* eval_tile, uint32_t* round_tile);
/* The geometry of msmz_scalars_sumcheck_step (csrc/mle_kernels.h), for the same purpose (nullable; needs no context):
 *   step_tile: NEW pair indices (those of the bound tables, 2^(n_vars-2) of them) one workgroup binds and sums into one
 *              partial sum per value -- the round's tile, over them. */
void msmz_test_sumcheck_step_geometry(uint32_t* step_tile);
/* msmz_scalars_dot_many (csrc/dot_kernels.h).
 *   msmz_test_dot_many_geometry (every pointer nullable; needs no context): tile_elements = the element indices of one
 *     tile (that of msmz_scalars_dot); max_groups = the most workgroups along n a call launches, each striding over the
 *     tiles (DOT_MANY_GROUPS); rows_per_block[c - 1], c = 1 .. MSMZ_DOT_MANY_MAX_COLS (8 words) = the rows of a thread's
 *     register block for c columns (dot_many_rg).
 *   msmz_test_set_dot_many_groups: lowers max_groups for later calls on this context (1 .. the built-in value; 0 = the
 *     built-in value again), so that a vector of a few tiles makes every workgroup stride more than once.  Changes no
 *     result.  MSMZ_ERR_ARG: a null context, a larger value; MSMZ_ERR_UNSUPPORTED: a multi-device context. */
void msmz_test_dot_many_geometry(uint32_t* tile_elements, uint32_t* max_groups, uint32_t* rows_per_block);
int msmz_test_set_dot_many_groups(msmz_ctx* ctx, uint32_t max_groups);
/* The geometry of msmz_matrix_mul (csrc/matrix_kernels.h), for the same purpose (every pointer nullable; needs no
 * context):
 *   tile            : consecutive non-zeros one workgroup takes and leaves one carry for (MAT_TILE);
 *   run             : consecutive non-zeros one thread walks (MAT_RUN);
 *   carries_per_pass: tile carries the one workgroup of the fold takes per pass of its loop (MAT_FOLD_PASS). */
void msmz_test_matrix_geometry(uint32_t* tile, uint32_t* run, uint32_t* carries_per_pass);
/* msmz_scalars_lookup (csrc/lookup_kernels.h); both need no context.
 *   msmz_test_lookup_geometry: min_slots = the slots of the smallest index (a table of one entry: lk_slots(1));
 *     threads_per_workgroup = the threads of a workgroup of all three kernels (LK_THREADS).  Every pointer nullable.
 *   msmz_test_lookup_small_table: the largest table whose counts k_lookup_count_small keeps in LDS (LK_SMALL_TABLE; one
 *     entry more and k_lookup_count runs); *passes = the passes of threads_per_workgroup column entries a workgroup of it
 *     takes at the least (LK_SMALL_PASSES), *max_groups = the most workgroups it launches (LK_SMALL_GROUPS): a column of
 *     more than passes * threads * max_groups entries makes every workgroup loop longer.  Both pointers nullable.
 *   msmz_test_lookup_slot: the first slot the engine probes for the canonical value le32 (32 little-endian bytes) in a
 *     table of table_n entries, from the host by the same hash the kernels run -- for tests that build tables whose keys
 *     all start at one slot, or at the last slot.  0xffffffff for an unknown curve, a null pointer, a value >= q or a
 *     table_n that msmz_scalars_lookup refuses. */
void msmz_test_lookup_geometry(uint32_t* min_slots, uint32_t* threads_per_workgroup);
uint32_t msmz_test_lookup_small_table(uint32_t* passes, uint32_t* max_groups);
uint32_t msmz_test_lookup_slot(int curve_id, const uint8_t* le32, uint64_t table_n);
/* msmz_scalars_expr (csrc/expr_kernels.h); needs no context.  threads_per_workgroup = the output entries of one workgroup
 * of k_scalars_expr; register_slots = the largest operand count that takes the register-resident kernel
 * (k_scalars_expr_slots; 0 would mean there is none and every expression takes k_scalars_expr). */
void msmz_test_expr_geometry(uint32_t* threads_per_workgroup, uint32_t* register_slots);
/* msmz_points_fixed_base (msm_zprize_amd/csrc/fixed_base.h).
 *   msmz_test_fixed_base_plan: what the planner picks for n points of a curve and a bound of `bits` (0 or >= the bit
 *     length of q: none) -- the window width, the windows K = ceil((bound + 1) / c) and the table's entries
 *     K 2^(c-1).  Needs no context.  MSMZ_ERR_ARG: an unknown curve, a null pointer, n == 0, bits < 0 or > 256.
 *   msmz_test_set_fixed_base_window: later calls on this context cut their digits c wide (4 .. 16) whatever the planner
 *     says; 0 = the planner's choice again.  MSMZ_ERR_ARG: another c, or one whose full-width table passes 64 MiB.
 *   msmz_test_fixed_base_tables: *built = the tables this context has built so far (a call served from the cache adds
 *     none; a multi-device context: the sum over its engines). */
int msmz_test_fixed_base_plan(int curve_id, uint64_t n, int bits, int32_t* c, int32_t* K, uint64_t* entries);
int msmz_test_set_fixed_base_window(msmz_ctx* ctx, int c);
int msmz_test_fixed_base_tables(msmz_ctx* ctx, uint64_t* built);
/* The caches of an engine and the grid of a transform, for tests that fill a cache past its size or run more vectors
 * than a launch has rows of workgroups.
 *   msmz_test_cache_geometry (every pointer nullable; needs no context): ntt_sets = the twiddle sets an engine keeps,
 *     the oldest leaves first (NTT_CACHE); fixed_tables = the fixed-base tables it keeps, the one unused longest leaves
 *     first (FIXED_CACHE); ntt_grid_vectors = the most vectors of a batch that get a workgroup row of their own in a pass
 *     of msmz_scalars_ntt (NTT_GRID_VECTORS): with a larger count a workgroup takes every ntt_grid_vectors-th vector.
 *   msmz_test_ntt_tables: *built = the twiddle sets this context has built so far (a transform served from the cache adds
 *     none; a multi-device context: the sum over its engines). */
void msmz_test_cache_geometry(uint32_t* ntt_sets, uint32_t* fixed_tables, uint32_t* ntt_grid_vectors);
int msmz_test_ntt_tables(msmz_ctx* ctx, uint64_t* built);
/* out[i] = op(a[i], b[i]) for i < n; a, b, out: n * fe_bytes */
int msmz_test_field(msmz_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out);
/* GLV split of n 32-byte scalars: s0, s1 = magnitudes (16 bytes each), neg = 2 sign bytes per scalar
 * (glv.ts:68-169 `decompose`).  MSMZ_ERR_UNSUPPORTED on a curve without endomorphism. */
int msmz_test_glv(msmz_ctx* ctx, const uint8_t* scalars_le32, uint64_t n, uint8_t* s0_le16, uint8_t* s1_le16,
                  uint8_t* neg);
/* signed c-bit digits as the sort kernels slice them (msm-batched-affine.ts:180-199): K digits per (half) scalar,
 * digits[(h*n + i)*K + k] = l | negate << 31 */
int msmz_test_digits(msmz_ctx* ctx, const uint8_t* scalars_le32, uint64_t n, int c, int K, int glv, uint32_t* digits);
/* the bucket sort alone: scalars -> bucket offsets `off` (nb + 1 words) and sorted references `refs`
 * (index | negate << 31; GLV: index >= n = endomorphism half of point index - n).  Geometry in geom[8] =
 * {c, K, Keff, L, nb, n_entries, max_bucket, spread}.  off / refs may be NULL to query the geometry only;
 * force_fallback = 1 runs the one-pass atomic sort.  Capacities in words. */
int msmz_test_sort(msmz_ctx* ctx, const uint8_t* scalars_le32, uint64_t n, int c, int glv, int force_fallback,
                   uint32_t* geom, uint32_t* off, uint64_t off_cap, uint32_t* refs, uint64_t refs_cap);

/* The bucket sort alone at every geometry an MSM runs it in: the engine's own Planner::make_plan, sort_layout and
 * BucketSort::run of csrc/sort.h (k_hist, k_bin_scan or the three-launch scan, k_coarse, k_fine; or the fallback k_digits, k_scan_*,
 * k_scatter), the template instances an MSM launches.  Pure integers: no point is read.  msmz_test_sort above is this
 * hook with nprob = 1, factor = 1, pts_n = n and no bound or fold.
 *   scalars_le32: nprob * n scalars, problem after problem;  n: 1 .. 2^22;  nprob: 1 .. 64 (a batched MSM);
 *   c (0 = the planner's choice), glv, force_fallback: as msmz_test_sort;
 *   scalar_bits: the caller's bound, msmz_opts.reserved[1] (0 .. 256; 0 = none);  allow_fold: the thin top window may be
 *     folded, as an MSM on the batched-affine path allows;
 *   pts_n >= n (0 = n): size of the point set the MSM would cover a prefix of; with GLV the second halves' references are
 *     moved up by endo_delta = pts_n - n;
 *   factor (0 or 1 = plain; .. 128): windows per bucket set of a precomputed point set (F of make_plan; the layout uses
 *     min(factor, K));  copy_stride: records per copy -- window k references index + (k mod F) * copy_stride.
 * Outputs, each nullable, capacities in words:
 *   geom (>= MSMZ_TS_GEOM_WORDS): the geometry, indexed by the MSMZ_TS_* names below: Plan / SortGeom / SortLayout of
 *     csrc/plan.h, F = the windows per bucket set in effect, min(factor, K); tiles = workgroups of k_hist / k_coarse per
 *     problem.  With every other output null the hook plans only and launches nothing;
 *   meta (3 words, no capacity): the RAW meta words after the sort -- error (bit 1 = value 2: a (half-)scalar does not
 *     fit K windows, or its top digit left a folded window -- that digit is in no bucket; bit 2 = value 4: a scalar >=
 *     the group order or >= 2^scalar_bits -- none of its digits is in a bucket), n_entries, max_bucket.  The error word is data: the hook returns
 *     MSMZ_OK with it set.  max_bucket: the largest bucket size when some bucket has two entries; when none has, the
 *     two-level sort leaves 0 and the fallback sort 1 (0 without any entry) -- every consumer treats 0 and 1 alike
 *     (plan_rounds: no round; the msmBasic chunk size; msmz_log.max_bucket reports it as it is);
 *   off (>= nprob * nb + 1): bucket offsets of all problems, problem p's buckets from p * nb on;
 *   refs, packed (>= nprob * K * M each, the most entries there can be): the n_entries sorted references
 *     (index | negate << 31), and the n_entries words k_coarse wrote, bin after bin in scan order:
 *     ((fine << 1 | negate) << idx_bits) | (k mod F) << mbits | entry, entry = half * n + scalar index;
 *   bins (>= nprob * sbins + 1): the scanned bin bases; bin p * sbins + s, s = ((k / F) * ncb + coarse) * F + k mod F
 *     for window k < K - 1 or F > 1, and (K - 1) * ncb + sub * ncbt + coarse for the plain top window's sub-window sub.
 *   packed and bins exist in the two-level sort only; with two_level = 0 they are left untouched.
 * MSMZ_ERR_ARG, before any launch: a null scalars / args, n, nprob, c, scalar_bits or factor out of range, pts_n < n or
 * > 2^30, an index + (F - 1) * copy_stride that leaves 31 bits, a plan make_plan refuses or with more than 2^26 entries,
 * a capacity below the above.  MSMZ_ERR_UNSUPPORTED: GLV on a curve without endomorphism; nprob > 1 or factor > 1 where
 * the layout is not two-level (BucketSort::run refuses them). */
enum {
  MSMZ_TS_C = 0, MSMZ_TS_K = 1, MSMZ_TS_KEFF = 2, MSMZ_TS_L = 3, MSMZ_TS_NB = 4, MSMZ_TS_FB = 5, MSMZ_TS_FBT = 6,
  MSMZ_TS_NCB = 7, MSMZ_TS_NCBT = 8, MSMZ_TS_NBINS = 9, MSMZ_TS_SBINS = 10, MSMZ_TS_FBINS = 11, MSMZ_TS_FINE_TOP = 12,
  MSMZ_TS_SPREAD = 13, MSMZ_TS_FOLD_SHIFT = 14, MSMZ_TS_FOLD_ROWS = 15, MSMZ_TS_F = 16, MSMZ_TS_MBITS = 17,
  MSMZ_TS_IDX_BITS = 18, MSMZ_TS_CSPEC = 19, MSMZ_TS_TWO_LEVEL = 20, MSMZ_TS_TILES = 21,
  MSMZ_TS_SBITS = 22 /* the bound as the kernels get it, 256 = none */, MSMZ_TS_ENDO_DELTA = 23,
  MSMZ_TS_GEOM_WORDS = 24
};
typedef struct msmz_test_sort_args {
  const uint8_t* scalars_le32;
  uint64_t n, pts_n;
  uint32_t nprob, factor, copy_stride;
  int32_t c, glv, force_fallback, scalar_bits, allow_fold;
  uint64_t geom_cap, off_cap, refs_cap, bins_cap, packed_cap;
  uint32_t* geom;
  uint32_t* meta;
  uint32_t* off;
  uint32_t* refs;
  uint32_t* bins;
  uint32_t* packed;
} msmz_test_sort_args;
int msmz_test_sort_ex(msmz_ctx* ctx, const msmz_test_sort_args* args);
/* point arithmetic on canonical affine inputs (x || y, 2*fe_bytes; infinity flags nullable, Weierstrass only):
 * out[i] = op(a[i], b[i]) as canonical affine, all-zero = infinity */
int msmz_test_point(msmz_ctx* ctx, int op, const uint8_t* a_xy, const uint8_t* a_inf, const uint8_t* b_xy,
                    const uint8_t* b_inf, uint64_t n, uint8_t* out_xy);

/* point arithmetic on operands in the kernels' own form (no conversion): every coordinate a lazy memory-format
 * Montgomery residue (fe_bytes each, [0, 3p)).  a: n accumulators of 4 coordinates -- XYZZ (X, Y, ZZ, ZZZ; ZZ = 0 is
 * infinity) or extended twisted Edwards (X, Y, Z, T).  b: n records of 4 coordinates -- an accumulator (ADD, ADD_X4,
 * CHAIN, CHAIN_X4), an affine record (x, y, 0, 0; all zero = infinity) for MADD / MDBL, or a Niels record
 * (y - x, y + x, 2d x y, 0) for the twisted-Edwards MADD.  neg (nullable): per element, negate the MADD / MDBL record
 * as the bucket accumulation does.  CHAIN(_X4): L steps (L <= 4096) from r = a, r <- r + b on even steps and r <- 2r
 * on odd ones, in registers.  out: canonical affine (x || y), all-zero = infinity (Weierstrass). */
enum {
  MSMZ_TPR_ADD = 0, MSMZ_TPR_ADD_X4 = 1, MSMZ_TPR_MADD = 2, MSMZ_TPR_DBL = 3, MSMZ_TPR_DBL_X4 = 4,
  MSMZ_TPR_MDBL = 5 /* Weierstrass only */, MSMZ_TPR_CHAIN = 6, MSMZ_TPR_CHAIN_X4 = 7,
  /* the row form (kernels.h, "row-form point addition"): one wave per addition, a field element per DPP row */
  MSMZ_TPR_ADD_ROWS = 8, MSMZ_TPR_DBL_ROWS = 9, MSMZ_TPR_CHAIN_ROWS = 10
};
int msmz_test_point_raw(msmz_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, const uint8_t* neg, uint64_t n,
                        int L, uint8_t* out_xy);

/* ONE launch of the tree rounds' batched-affine addition (k_batch_add, the template instance the MSM runs) with B
 * pairs per thread (1 .. 16) and the safe (1) or unsafe (0) variant, on caller-built operands (Weierstrass only).
 *   points_xy / points_inf (inf nullable): n_points original points as canonical affine (x || y, 2*fe_bytes), converted
 *     to the resident point format of the MSM;
 *   slots_xy / slots_inf (inf nullable): n_slots input slot records 0 .. n_slots-1, canonical affine, stored as the
 *     tree rounds store their results (infinity = the all-zero record);
 *   desc: n_pairs descriptors of two location words (operand a, operand b): 0x40000000 | i = point i, with bit 31
 *     set = its negative; j (bit 31 clear) = slot record j.  Pair t adds a + b and writes slot record out_base + t
 *     (out_base >= n_slots, any alignment);
 *   out_xy: the n_pairs results as canonical affine, all-zero = infinity;  error: the meta error word after the
 *     launch (bit 0: the unsafe variant met a zero denominator).
 * MSMZ_ERR_ARG for a location outside the supplied arrays, B outside 1 .. 16 or out_base < n_slots; MSMZ_ERR_RANGE
 * for a coordinate >= p. */
int msmz_test_batch_add(msmz_ctx* ctx, int safe, int B, const uint8_t* points_xy, const uint8_t* points_inf,
                        uint64_t n_points, const uint8_t* slots_xy, const uint8_t* slots_inf, uint64_t n_slots,
                        const uint32_t* desc, uint64_t n_pairs, uint64_t out_base, uint8_t* out_xy, uint32_t* error);

/* The bucket reduction alone, on caller-built buckets: the line sums and the weighted sums of the two-dimensional
 * reduction (csrc/reduce2d_kernels.h) and the upper levels (k_reduce_quad / k_reduce_quad16 / k_reduce_rows /
 * k_reduce_tail), through
 * the engine's own reduction stage (BucketReduce, csrc/reduce.h) and the template instances an MSM launches.  Run it before and after
 * touching a reduction kernel: it names the problem and the line an MSM's single result point cannot.
 *
 * 2-D modes: window size c (2 .. 16) fixes L = 2^(c-1), H = 2^ceil((c-1)/2), D = L / H as the planner's split does;
 * `nsets` bucket sets (1 .. 16) of L buckets, bucket g = set * L + (j - 1) holding weight j = 1 .. L.  Problem 2 s is
 * the row problem of set s (sum_h h R_h, R_h = sum_d E[h D + d], the weight-L bucket twice in R_(H/2)), problem 2 s + 1
 * its column problem (sum_d d C_d, C_d = sum_h E[h D + d]; its lines D .. H-1 are neutral).
 *   MSMZ_TR_LOCATIONS (Weierstrass): points_xy / points_inf = n_points original points, slots_xy / slots_inf = n_slots
 *     slot records (both as msmz_test_batch_add takes them); loc = 4 location words per bucket in that hook's encoding
 *     (0x40000000 | i = point i, bit 31 = its negative; j = slot record j), read up to the first 0xffffffff
 *     (LOC_NONE).  Drives k_reduce2d_partial.
 *   MSMZ_TR_ACCS: points_xy = n_points points (all-zero or flagged = infinity on Weierstrass; twisted Edwards has no
 *     flag, its neutral element is (0, 1)), each stored as an accumulator record; bucket g is the sum of records
 *     cscan[g] .. cscan[g+1]-1 (nsets * L + 1 offsets).  Drives k_reduce2d_partial_acc with chunk ranges.
 *   MSMZ_TR_ACCS_SUMMED: the same through k_bucket_sums and the one-accumulator-per-bucket mode of that kernel.
 * MSMZ_TR_LEVELS: BucketReduce::levels alone on `nsets` problems (1 .. 64) of n_in entries (1 .. 4096):  points_xy = the
 *   nsets * n_in rows, then the nsets * n_in C inputs (n_points = 2 * nsets * n_in); result j = sum_e (C_e + e row_e).
 * scale (nullable; ACCS, ACCS_SUMMED, LEVELS): one canonical field element lambda != 0 per input point; the record is
 *   stored as (lambda^2 x, lambda^3 y, lambda^2, lambda^3), resp. (lambda x, lambda y, lambda, lambda x y), so that
 *   equal points meet in different representations.
 * Level selection, each 0 = the engine's value, for this call only: nc = chunks per line (a power of two <= D);
 *   tail_n = entries per problem at which k_reduce_tail takes over (1 .. 4096); quad16_max = levels with at most this
 *   many groups run k_reduce_quad16, larger ones k_reduce_quad; pairsum_x4_max = pair-sum launches of at most this many
 *   additions run k_pairsum_x4, larger ones k_pairsum (both 1 .. 2^20); rows_max = levels of at most this many groups
 *   (1 .. 2^20, and within quad16_max) run the row form k_reduce_rows, also below tail_n, so that k_reduce_tail starts
 *   at the first level that is too large for it or at one entry; 1 keeps the row form to levels of a single group.
 * out_xy: the results as canonical affine (x || y; Weierstrass: all-zero = infinity), 2 * nsets for the 2-D modes,
 *   nsets for LEVELS.  lines_xy (nullable, 2-D modes): the 2 * nsets * H line sums after the pair-sum launches, problem
 *   by problem.
 * MSMZ_ERR_ARG for anything that would read outside the supplied arrays (a location beyond its table, a cscan that
 * decreases or ends beyond n_points, c / nsets / n_in / a threshold out of range, lambda = 0); MSMZ_ERR_RANGE for a
 * coordinate or lambda >= p; MSMZ_ERR_UNSUPPORTED for LOCATIONS on twisted Edwards. */
enum { MSMZ_TR_LOCATIONS = 0, MSMZ_TR_ACCS = 1, MSMZ_TR_ACCS_SUMMED = 2, MSMZ_TR_LEVELS = 3 };
typedef struct msmz_test_reduce_args {
  int32_t mode, c;
  uint32_t nsets, n_in;
  uint32_t nc, tail_n, quad16_max, pairsum_x4_max;
  const uint8_t* points_xy;
  const uint8_t* points_inf;
  uint64_t n_points;
  const uint8_t* slots_xy;
  const uint8_t* slots_inf;
  uint64_t n_slots;
  const uint8_t* scale;
  const uint32_t* loc;
  const uint32_t* cscan;
  uint8_t* out_xy;
  uint8_t* lines_xy;
  uint32_t rows_max;   /* appended: callers that leave it 0 get the engine's value */
} msmz_test_reduce_args;
int msmz_test_reduce(msmz_ctx* ctx, const msmz_test_reduce_args* args);

/* The schedule of the tree rounds alone (k_plan_count / k_plan_emit, csrc/plan_kernels.h), through the engine's own
 * plan_phase, on caller-built sorted buckets (Weierstrass only).  Pure integers: no point is read.
 *   nb, off (nb + 1 words, off[0] = 0, non-decreasing): the buckets; refs (off[nb] words; nullable when that is 0):
 *     the sorted references, index | negate << 31, bit 30 clear;
 *   chunk, nb_main, chunk_top: the PlanChunks of the launch (plan.h) -- buckets [0, nb_main) in workgroups of `chunk`
 *     buckets (1 .. PLAN_CHUNK = 1024), the rest in workgroups of `chunk_top` (1 .. chunk);
 *   tail_skip (0 .. 2): rounds = ceil(log2 max bucket) - tail_skip, at least 1 when a bucket has two entries.
 * The hook writes the largest bucket size and error = 0 into the device meta block, as the sort would have, and launches.
 *   meta (68 words): the device meta block after the launch -- max_bucket, n_entries, error, rounds, round_pairs[32],
 *     round_base[32];
 *   desc (desc_cap pairs of 2 words): {locA, locB} of every addition, round after round; as many pairs as the rule gives
 *     for these buckets (sum over the rounds), whatever the device counted.  A location word: 0x40000000 | index, with
 *     bit 31 = negate, is an original point; any other word is the record (result) number of an earlier pair;
 *   bfin (bfin_cap buckets of 4 words): the locations of what the rounds leave of each bucket, then 0xffffffff;
 *   chunk_pairs (nullable; chunk_pairs_cap words): the 26 x n_chunks table of pairs per round and workgroup,
 *     chunk_pairs[r * n_chunks + w].
 * MSMZ_ERR_ARG, before any launch, for anything that would read or write outside an array: a null required pointer,
 * nb = 0 or nb > 2^22, off[0] != 0, a decreasing off, off[nb] > 2^25, a bucket of 2^26 entries or more, a reference with
 * bit 30 set, chunk outside 1 .. 1024, chunk_top outside 1 .. chunk, nb_main > nb, tail_skip outside 0 .. 2, or a
 * capacity below what these buckets need (desc: the pairs of all rounds; bfin: nb; chunk_pairs: 26 n_chunks);
 * MSMZ_ERR_UNSUPPORTED on twisted Edwards (no tree rounds there). */
typedef struct msmz_test_plan_args {
  uint32_t nb, chunk, nb_main, chunk_top;
  int32_t tail_skip;
  uint32_t reserved;
  const uint32_t* off;
  const uint32_t* refs;
  uint64_t desc_cap, bfin_cap, chunk_pairs_cap;
  uint32_t* meta;
  uint32_t* desc;
  uint32_t* bfin;
  uint32_t* chunk_pairs;
} msmz_test_plan_args;
int msmz_test_plan(msmz_ctx* ctx, const msmz_test_plan_args* args);

#ifdef __cplusplus
}
#endif
#endif /* MSMZ_TEST_H */

"""ctypes binding of the C ABI in include/msmz.h (libmsmz.so, built in-tree by msm_zprize_amd.build).

There is no CPU fallback: if the HIP library is missing or no GPU is visible, every entry point
raises.  The library is loaded lazily so that CPU-only tooling (tests of the host logic) can import
the package.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSMZ_LIB") or os.path.join(HERE, "libmsmz.so")   # MSMZ_LIB: development builds

MSMZ_N_STAGES = 8
STAGE_NAMES = ["digits", "scan", "scatter", "plan", "accumulate", "reduce", "final", "total"]


class MsmzOpts(C.Structure):
    _fields_ = [("c", C.c_int32), ("glv", C.c_int32), ("safe", C.c_int32), ("buckets", C.c_int32),
                ("timing", C.c_int32), ("reserved", C.c_int32 * 3)]


class MsmzLog(C.Structure):
    _fields_ = [("stage_ms", C.c_float * MSMZ_N_STAGES), ("c", C.c_int32), ("K", C.c_int32), ("rounds", C.c_int32),
                ("glv", C.c_int32), ("n_entries", C.c_uint64), ("n_pairs", C.c_uint64), ("max_bucket", C.c_uint32),
                ("scatter_launches", C.c_uint32), ("scatter_kernel_ms", C.c_float), ("batch_add_ms", C.c_float * 32)]


MSMZ_SRC_DEVICE, MSMZ_SRC_MONTGOMERY, MSMZ_SRC_DEFAULT_STREAM = 1, 2, 4
MSMZ_SRC_COMPRESSED, MSMZ_SRC_SIGN_PARITY = 8, 16   # compressed point records and their second sign convention
MSMZ_ERR_POINT = 7                                  # a compressed record is not a point of the curve


class MsmzSrc(C.Structure):   # msmz_src (include/msmz.h): where an imported set lies and in which form
    _fields_ = [("ptr", C.c_void_p), ("stride", C.c_uint64), ("width", C.c_uint32), ("flags", C.c_uint32),
                ("stream", C.c_void_p), ("is_inf", C.c_void_p)]


class MsmzDst(C.Structure):   # msmz_dst (include/msmz.h): msmz_src read in the other direction, where an export goes
    _fields_ = list(MsmzSrc._fields_)


MSMZ_CHECK_CURVE, MSMZ_CHECK_SUBGROUP = 1, 2
NO_INDEX = (1 << 64) - 1   # msmz_check_result.first_bad: no bad point


class MsmzCheckResult(C.Structure):   # msmz_check_result (include/msmz.h)
    _fields_ = [("off_curve", C.c_uint64), ("off_subgroup", C.c_uint64), ("first_bad", C.c_uint64)]


class MsmzMul(C.Structure):   # msmz_mul (include/msmz.h): out_i = [s_i] P_i (+ Q_i)
    _fields_ = [("points_handle", C.c_uint64), ("first_p", C.c_uint64), ("scalars_handle", C.c_uint64),
                ("first_s", C.c_uint64), ("scalar", C.c_char_p), ("addend_handle", C.c_uint64), ("first_q", C.c_uint64)]


MSMZ_MUL_SUBGROUP = 1


class MsmzMulOpts(C.Structure):   # msmz_mul_opts (include/msmz.h): the caller's bound on the scalars and vouch for the points
    _fields_ = [("flags", C.c_uint32), ("scalar_bits", C.c_int32), ("reserved", C.c_int32 * 2)]


class MsmzFixedBase(C.Structure):   # msmz_fixed_base (include/msmz.h): out_i = [s_i] B for one base B
    _fields_ = [("base_handle", C.c_uint64), ("base_index", C.c_uint64), ("base_xy_le", C.c_char_p),
                ("scalars_handle", C.c_uint64), ("first_s", C.c_uint64), ("scalar_bits", C.c_int32), ("flags", C.c_uint32)]


class MsmzScalarTerm(C.Structure):   # msmz_scalar_term (include/msmz.h): one term c (.) v of msmz_scalars_combine
    _fields_ = [("handle", C.c_uint64), ("first", C.c_uint64), ("coeff_handle", C.c_uint64), ("coeff_first", C.c_uint64),
                ("coeff", C.c_char_p)]


MSMZ_REC_REVERSE, MSMZ_REC_EXCLUSIVE = 1, 2


class MsmzScalarRec(C.Structure):   # msmz_scalar_rec (include/msmz.h): y_i = a_i y_(i-1) + b_i
    _fields_ = [("a_handle", C.c_uint64), ("a_first", C.c_uint64), ("a", C.c_char_p), ("b_handle", C.c_uint64),
                ("b_first", C.c_uint64), ("init", C.c_char_p), ("flags", C.c_uint32)]


MSMZ_NTT_INVERSE, MSMZ_NTT_COSET = 1, 2


class MsmzNtt(C.Structure):   # msmz_ntt (include/msmz.h): `count` transforms of length 2^log_n
    _fields_ = [("handle", C.c_uint64), ("first", C.c_uint64), ("log_n", C.c_uint32), ("flags", C.c_uint32),
                ("n_in", C.c_uint64), ("count", C.c_uint32), ("root", C.c_char_p), ("shift", C.c_char_p)]


MSMZ_MLE_LOW = 1
MSMZ_SUMCHECK_MAX_TABLES, MSMZ_SUMCHECK_MAX_DEGREE, MSMZ_SUMCHECK_MAX_TERMS = 6, 4, 8


class MsmzMleBind(C.Structure):   # msmz_mle_bind (include/msmz.h): `count` tables of 2^n_vars entries, one variable bound to r
    _fields_ = [("handle", C.c_uint64), ("first", C.c_uint64), ("n_vars", C.c_uint32), ("count", C.c_uint32),
                ("flags", C.c_uint32), ("r", C.c_char_p)]


class MsmzSumcheckTable(C.Structure):   # msmz_sumcheck_table: one table of a round
    _fields_ = [("handle", C.c_uint64), ("first", C.c_uint64)]


class MsmzSumcheckTerm(C.Structure):   # msmz_sumcheck_term: coeff * the product of the tables of `mask`
    _fields_ = [("coeff", C.c_char_p), ("mask", C.c_uint32)]


class MsmzSumcheck(C.Structure):   # msmz_sumcheck (include/msmz.h): the round polynomial of a sum of products
    _fields_ = [("tables", C.POINTER(MsmzSumcheckTable)), ("n_tables", C.c_uint32), ("n_vars", C.c_uint32),
                ("terms", C.POINTER(MsmzSumcheckTerm)), ("n_terms", C.c_uint32), ("flags", C.c_uint32)]


class MsmzSumcheckStep(C.Structure):   # msmz_sumcheck_step (include/msmz.h): bind every table to r, the next round's polynomial
    _fields_ = [("tables", C.POINTER(MsmzSumcheckTable)), ("out", C.POINTER(MsmzSumcheckTable)), ("n_tables", C.c_uint32),
                ("n_vars", C.c_uint32), ("terms", C.POINTER(MsmzSumcheckTerm)), ("n_terms", C.c_uint32), ("flags", C.c_uint32),
                ("r", C.c_char_p)]


MSMZ_MAT_ROWS, MSMZ_MAT_COLS = 1, 2
MSMZ_MATVEC_TRANSPOSE = 1


class MsmzSparse(C.Structure):   # msmz_sparse (include/msmz.h): nnz triples (row, col, value) of a sparse matrix
    _fields_ = [("row", C.POINTER(C.c_uint32)), ("col", C.POINTER(C.c_uint32)), ("val_handle", C.c_uint64),
                ("val_first", C.c_uint64), ("nnz", C.c_uint64), ("n_rows", C.c_uint32), ("n_cols", C.c_uint32),
                ("flags", C.c_uint32)]


class MsmzMatvec(C.Structure):   # msmz_matvec (include/msmz.h): one product of a matrix handle with a scalar range
    _fields_ = [("matrix", C.c_uint64), ("x_handle", C.c_uint64), ("x_first", C.c_uint64), ("flags", C.c_uint32)]


LOOKUP_NONE = 0xffffffff   # msmz_lookup.positions: no table entry equals this column entry


class MsmzLookup(C.Structure):   # msmz_lookup (include/msmz.h): a table range, a column range, where the positions go
    _fields_ = [("table_handle", C.c_uint64), ("table_first", C.c_uint64), ("table_n", C.c_uint64),
                ("col_handle", C.c_uint64), ("col_first", C.c_uint64), ("col_n", C.c_uint64),
                ("positions", C.POINTER(C.c_uint32)), ("flags", C.c_uint32)]


class MsmzLookupResult(C.Structure):   # msmz_lookup_result (include/msmz.h)
    _fields_ = [("n_missing", C.c_uint64), ("first_missing", C.c_uint64), ("n_distinct", C.c_uint64)]


MSMZ_EXPR_MAX_COLUMNS, MSMZ_EXPR_MAX_TERMS, MSMZ_EXPR_MAX_DEGREE, MSMZ_EXPR_MAX_OPERANDS = 16, 32, 8, 32


class MsmzExprColumn(C.Structure):   # msmz_expr_column: one column of an expression, n entries from `first`
    _fields_ = [("handle", C.c_uint64), ("first", C.c_uint64)]


class MsmzExprFactor(C.Structure):   # msmz_expr_factor: a column read `rot` rows ahead (cyclically)
    _fields_ = [("column", C.c_uint32), ("rot", C.c_int32)]


class MsmzExprTerm(C.Structure):   # msmz_expr_term: coeff * the product of its factors
    _fields_ = [("coeff", C.c_char_p), ("factors", C.POINTER(MsmzExprFactor)), ("n_factors", C.c_uint32),
                ("reserved", C.c_uint32)]


class MsmzExpr(C.Structure):   # msmz_expr (include/msmz.h): a sum of products of rotated columns
    _fields_ = [("columns", C.POINTER(MsmzExprColumn)), ("n_columns", C.c_uint32), ("n_terms", C.c_uint32),
                ("terms", C.POINTER(MsmzExprTerm)), ("n", C.c_uint64), ("flags", C.c_uint32)]


assert (C.sizeof(MsmzExprColumn), C.sizeof(MsmzExprFactor), C.sizeof(MsmzExprTerm), C.sizeof(MsmzExpr)) == (16, 8, 24, 40)

MSMZ_DOT_MANY_MAX_ROWS, MSMZ_DOT_MANY_MAX_COLS = 128, 8


class MsmzScalarVec(C.Structure):   # msmz_scalar_vec: one vector of msmz_dot_many, entries [first, first + n) of `handle`
    _fields_ = [("handle", C.c_uint64), ("first", C.c_uint64)]


class MsmzDotMany(C.Structure):   # msmz_dot_many (include/msmz.h): every inner product of rows x cols
    _fields_ = [("rows", C.POINTER(MsmzScalarVec)), ("n_rows", C.c_uint32), ("cols", C.POINTER(MsmzScalarVec)),
                ("n_cols", C.c_uint32), ("n", C.c_uint64), ("flags", C.c_uint32)]


assert (C.sizeof(MsmzScalarVec), C.sizeof(MsmzDotMany)) == (16, 48)


class MsmzSegment(C.Structure):   # msmz_segment (include/msmz.h): one problem of msmz_msm_segments
    _fields_ = [("first_p", C.c_uint64), ("first_s", C.c_uint64), ("n", C.c_uint64)]


class MsmzTestReduceArgs(C.Structure):   # msmz_test_reduce_args (include/msmz_test.h)
    _fields_ = [("mode", C.c_int32), ("c", C.c_int32), ("nsets", C.c_uint32), ("n_in", C.c_uint32),
                ("nc", C.c_uint32), ("tail_n", C.c_uint32), ("quad16_max", C.c_uint32), ("pairsum_x4_max", C.c_uint32),
                ("points_xy", C.c_char_p), ("points_inf", C.c_char_p), ("n_points", C.c_uint64),
                ("slots_xy", C.c_char_p), ("slots_inf", C.c_char_p), ("n_slots", C.c_uint64),
                ("scale", C.c_char_p), ("loc", C.c_void_p), ("cscan", C.c_void_p),
                ("out_xy", C.c_void_p), ("lines_xy", C.c_void_p), ("rows_max", C.c_uint32)]


class MsmzTestPlanArgs(C.Structure):   # msmz_test_plan_args (include/msmz_test.h)
    _fields_ = [("nb", C.c_uint32), ("chunk", C.c_uint32), ("nb_main", C.c_uint32), ("chunk_top", C.c_uint32),
                ("tail_skip", C.c_int32), ("reserved", C.c_uint32),
                ("off", C.c_void_p), ("refs", C.c_void_p),
                ("desc_cap", C.c_uint64), ("bfin_cap", C.c_uint64), ("chunk_pairs_cap", C.c_uint64),
                ("meta", C.c_void_p), ("desc", C.c_void_p), ("bfin", C.c_void_p), ("chunk_pairs", C.c_void_p)]


class MsmzTestSortArgs(C.Structure):   # msmz_test_sort_args (include/msmz_test.h)
    _fields_ = [("scalars_le32", C.c_void_p), ("n", C.c_uint64), ("pts_n", C.c_uint64),
                ("nprob", C.c_uint32), ("factor", C.c_uint32), ("copy_stride", C.c_uint32),
                ("c", C.c_int32), ("glv", C.c_int32), ("force_fallback", C.c_int32), ("scalar_bits", C.c_int32),
                ("allow_fold", C.c_int32),
                ("geom_cap", C.c_uint64), ("off_cap", C.c_uint64), ("refs_cap", C.c_uint64), ("bins_cap", C.c_uint64),
                ("packed_cap", C.c_uint64),
                ("geom", C.c_void_p), ("meta", C.c_void_p), ("off", C.c_void_p), ("refs", C.c_void_p),
                ("bins", C.c_void_p), ("packed", C.c_void_p)]


# the geometry words of msmz_test_sort_ex, in order (MSMZ_TS_* of include/msmz_test.h)
TEST_SORT_GEOM = ["c", "K", "Keff", "L", "nb", "fb", "fbt", "ncb", "ncbt", "nbins", "sbins", "fbins", "fine_top", "spread",
                  "fold_shift", "fold_rows", "F", "mbits", "idx_bits", "cspec", "two_level", "tiles", "sbits", "endo_delta"]


EXPORTS = {
    # name: (restype, argtypes)
    "msmz_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int), C.c_int]),
    "msmz_destroy": (None, [C.c_void_p]),
    "msmz_strerror": (C.c_char_p, [C.c_int]),
    "msmz_curve_fe_bytes": (C.c_int, [C.c_int]),
    "msmz_ctx_fe_bytes": (C.c_int, [C.c_void_p]),
    "msmz_ctx_n_devices": (C.c_int, [C.c_void_p]),
    "msmz_upload_points": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_upload_scalars": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_import_scalars": (C.c_int, [C.c_void_p, C.POINTER(MsmzSrc), C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_import_scalars_into": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(MsmzSrc), C.c_uint64]),
    "msmz_alloc_scalars": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_import_points": (C.c_int, [C.c_void_p, C.POINTER(MsmzSrc), C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_random_points": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_random_scalars": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_download_points": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p, C.c_char_p]),
    "msmz_download_points_compressed": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p, C.c_char_p,
                                                  C.c_uint32]),
    "msmz_download_scalars": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p]),
    "msmz_export_scalars": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(MsmzDst)]),
    "msmz_export_points": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(MsmzDst)]),
    "msmz_free": (C.c_int, [C.c_void_p, C.c_uint64]),
    "msmz_msm": (C.c_int, [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(MsmzOpts), C.c_char_p,
                           C.POINTER(C.c_int), C.POINTER(MsmzLog)]),
    "msmz_msm_resident": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(MsmzOpts), C.c_char_p,
                                    C.POINTER(C.c_int), C.POINTER(MsmzLog)]),
    "msmz_msm_batch": (C.c_int, [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(MsmzOpts),
                                 C.c_char_p, C.POINTER(C.c_int), C.POINTER(MsmzLog)]),
    "msmz_msm_batch_resident": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                          C.POINTER(MsmzOpts), C.c_char_p, C.POINTER(C.c_int), C.POINTER(MsmzLog)]),
    "msmz_msm_segments": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(MsmzSegment), C.c_uint32,
                                    C.POINTER(MsmzOpts), C.c_char_p, C.POINTER(C.c_int), C.POINTER(MsmzLog)]),
    "msmz_precompute_points": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(MsmzOpts), C.c_uint32,
                                         C.POINTER(C.c_uint64)]),
    "msmz_precomputed_info": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "msmz_precomputed_scalar_bits": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_int32)]),
    "msmz_check_points": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                    C.POINTER(MsmzCheckResult), C.c_char_p]),
    "msmz_points_mul": (C.c_int, [C.c_void_p, C.POINTER(MsmzMul), C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_points_mul_opts": (C.c_int, [C.c_void_p, C.POINTER(MsmzMul), C.c_uint64, C.POINTER(MsmzMulOpts),
                                       C.POINTER(C.c_uint64)]),
    "msmz_points_fixed_base": (C.c_int, [C.c_void_p, C.POINTER(MsmzFixedBase), C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_scalars_combine": (C.c_int, [C.c_void_p, C.POINTER(MsmzScalarTerm), C.POINTER(MsmzScalarTerm), C.c_uint64,
                                       C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_scalars_dot": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p]),
    "msmz_scalars_powers": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_scalars_recurrence": (C.c_int, [C.c_void_p, C.POINTER(MsmzScalarRec), C.c_uint64, C.c_uint64,
                                          C.POINTER(C.c_uint64), C.c_char_p]),
    "msmz_scalars_inverse": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64)]),
    "msmz_scalars_ntt": (C.c_int, [C.c_void_p, C.POINTER(MsmzNtt), C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_scalars_root_of_unity": (C.c_int, [C.c_int, C.c_uint32, C.c_char_p]),
    "msmz_scalars_eq_table": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint64)]),
    "msmz_scalars_mle_eval": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_char_p, C.c_char_p]),
    "msmz_scalars_mle_bind": (C.c_int, [C.c_void_p, C.POINTER(MsmzMleBind), C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_scalars_sumcheck_round": (C.c_int, [C.c_void_p, C.POINTER(MsmzSumcheck), C.POINTER(C.c_uint32), C.c_char_p]),
    "msmz_scalars_sumcheck_step": (C.c_int, [C.c_void_p, C.POINTER(MsmzSumcheckStep), C.POINTER(C.c_uint32), C.c_char_p]),
    "msmz_scalars_dot_many": (C.c_int, [C.c_void_p, C.POINTER(MsmzDotMany), C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_matrix_create": (C.c_int, [C.c_void_p, C.POINTER(MsmzSparse), C.POINTER(C.c_uint64)]),
    "msmz_matrix_info": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint32)]),
    "msmz_matrix_mul": (C.c_int, [C.c_void_p, C.POINTER(MsmzMatvec), C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_scalars_lookup": (C.c_int, [C.c_void_p, C.POINTER(MsmzLookup), C.c_uint64, C.POINTER(C.c_uint64),
                                      C.POINTER(MsmzLookupResult)]),
    "msmz_scalars_expr": (C.c_int, [C.c_void_p, C.POINTER(MsmzExpr), C.c_uint64, C.POINTER(C.c_uint64)]),
    "msmz_point_add": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_int)]),
    # stage-level test hooks (include/msmz_test.h)
    "msmz_test_set_glv_bits": (C.c_int, [C.c_void_p, C.c_int]),
    "msmz_test_retries": (C.c_int, [C.c_void_p]),
    "msmz_test_set_limits": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "msmz_test_poison": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "msmz_test_scratch": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "msmz_test_passes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "msmz_test_scalar_dot_geometry": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "msmz_test_scalar_scan_geometry": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "msmz_test_ntt_plan": (C.c_int, [C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "msmz_test_ntt_geometry": (None, [C.POINTER(C.c_uint32)]),
    "msmz_test_matrix_geometry": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "msmz_test_expr_geometry": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "msmz_test_lookup_geometry": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "msmz_test_lookup_slot": (C.c_uint32, [C.c_int, C.c_char_p, C.c_uint64]),
    "msmz_test_lookup_small_table": (C.c_uint32, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "msmz_test_mle_geometry": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "msmz_test_sumcheck_step_geometry": (None, [C.POINTER(C.c_uint32)]),
    "msmz_test_dot_many_geometry": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "msmz_test_set_dot_many_groups": (C.c_int, [C.c_void_p, C.c_uint32]),
    "msmz_test_fixed_base_plan": (C.c_int, [C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_uint64)]),
    "msmz_test_set_fixed_base_window": (C.c_int, [C.c_void_p, C.c_int]),
    "msmz_test_fixed_base_tables": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "msmz_test_ntt_tables": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "msmz_test_cache_geometry": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "msmz_test_field": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_uint64, C.c_char_p]),
    "msmz_test_field_limbs": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                        C.c_char_p]),
    "msmz_test_field_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                       C.c_char_p]),
    "msmz_test_glv": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_char_p, C.c_char_p]),
    "msmz_test_digits": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "msmz_test_sort": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_uint64, C.c_void_p, C.c_uint64]),
    "msmz_test_sort_ex": (C.c_int, [C.c_void_p, C.POINTER(MsmzTestSortArgs)]),
    "msmz_test_point_raw": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int,
                                      C.c_char_p]),
    "msmz_test_point": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64,
                                  C.c_char_p]),
    "msmz_test_batch_add": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_uint64, C.c_char_p,
                                      C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p,
                                      C.POINTER(C.c_uint32)]),
    "msmz_test_reduce": (C.c_int, [C.c_void_p, C.POINTER(MsmzTestReduceArgs)]),
    "msmz_test_plan": (C.c_int, [C.c_void_p, C.POINTER(MsmzTestPlanArgs)]),
}

_lib = None


class MsmzError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        msg = lib().msmz_strerror(status).decode() if _lib is not None else "?"
        super().__init__(f"{where}: msmz status {status} ({msg})")


def lib():
    """Load libmsmz.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -m msm_zprize_amd.build` "
                               "(the MSM has no CPU fallback)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(status, where):
    if status != 0:
        raise MsmzError(status, where)

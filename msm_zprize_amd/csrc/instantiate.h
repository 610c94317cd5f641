// Explicit-instantiation lists: each (kernel family, curve) pair is compiled in its own translation
// unit (kern_<family>.hip with -DMSMZ_CURVE=<id>) so the build parallelizes; msmz.hip only sees
// `extern template` declarations.
#pragma once
#include "check_kernels.h"
#include "dot_kernels.h"
#include "export_kernels.h"
#include "expr_kernels.h"
#include "fixed_kernels.h"
#include "gen_kernels.h"
#include "import_kernels.h"
#include "kernels.h"
#include "lookup_kernels.h"
#include "matrix_kernels.h"
#include "mle_kernels.h"
#include "mul_kernels.h"
#include "ntt_kernels.h"
#include "scalar_kernels.h"
#include "scan_kernels.h"
#include "test_kernels.h"

// curve ids as in include/msmz.h
#if !defined(MSMZ_CURVE) || MSMZ_CURVE == 0
#define MSMZ_W0(X) X(Bls377Fp, Bls377Fr)
#else
#define MSMZ_W0(X)
#endif
#if !defined(MSMZ_CURVE) || MSMZ_CURVE == 1
#define MSMZ_W1(X) X(PallasFp, PallasFr)
#else
#define MSMZ_W1(X)
#endif
#if !defined(MSMZ_CURVE) || MSMZ_CURVE == 2
#define MSMZ_W2(X) X(Bls381Fp, Bls381Fr)
#else
#define MSMZ_W2(X)
#endif
#if !defined(MSMZ_CURVE) || MSMZ_CURVE == 3
#define MSMZ_T3(X) X(Ed377Fp, Ed377Fr)
#else
#define MSMZ_T3(X)
#endif
#define MSMZ_WEIERSTRASS_FIELDS(X) MSMZ_W0(X) MSMZ_W1(X) MSMZ_W2(X)
#define MSMZ_TE_FIELDS(X) MSMZ_T3(X)

#ifndef MSMZ_BATCH_T
#define MSMZ_BATCH_T 256
#endif
#ifndef MSMZ_BATCH_OCC
#define MSMZ_BATCH_OCC 4
#endif
#ifndef MSMZ_BATCH_BMAX
#define MSMZ_BATCH_BMAX 16
#endif

#define MSMZ_INST_BATCH(F, Fr, PFX)                                                                               \
  PFX template __global__ void k_batch_add<F, MSMZ_BATCH_T, true, MSMZ_BATCH_OCC, MSMZ_BATCH_BMAX>(              \
      uint32_t*, const uint32_t*, const uint2*, uint32_t, uint32_t, int, MsmMeta*);                              \
  PFX template __global__ void k_batch_add<F, MSMZ_BATCH_T, false, MSMZ_BATCH_OCC, MSMZ_BATCH_BMAX>(             \
      uint32_t*, const uint32_t*, const uint2*, uint32_t, uint32_t, int, MsmMeta*);

#define MSMZ_INST_POLICY(P, PFX)                                                                                 \
  PFX template __global__ void k_reduce_quad<P>(uint32_t*, uint32_t*, const uint32_t*, const uint32_t*, uint32_t, \
                                                uint32_t, uint32_t);                                             \
  PFX template __global__ void k_reduce_quad16<P>(uint32_t*, uint32_t*, const uint32_t*, const uint32_t*,        \
                                                  uint32_t, uint32_t, uint32_t);                                 \
  PFX template __global__ void k_reduce_tail<P>(uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t, \
                                                uint32_t);                                                       \
  PFX template __global__ void k_reduce_rows<P>(uint32_t*, uint32_t*, const uint32_t*, const uint32_t*, uint32_t, \
                                                uint32_t, uint32_t);                                             \
  PFX template __global__ void k_pairsum<P>(uint32_t*, const uint32_t*, uint32_t);                               \
  PFX template __global__ void k_fill_neutral<P>(uint32_t*, uint32_t);                                           \
  PFX template __global__ void k_bucket_sums<P>(uint32_t*, const uint32_t*, const uint32_t*, uint32_t);          \
  PFX template __global__ void k_reduce2d_partial_acc<P>(uint32_t*, const uint32_t*, const uint32_t*, R2Geom, uint32_t); \
  PFX template __global__ void k_pairsum_x4<P>(uint32_t*, const uint32_t*, uint32_t);                            \
  PFX template __global__ void k_bucket_accumulate<P>(uint32_t*, const uint32_t*, const uint32_t*,               \
                                                      const uint32_t*, const uint32_t*, uint32_t, uint32_t, int);

#define MSMZ_INST_REDUCE(F, Fr, PFX)                                                                              \
  PFX template __global__ void k_reduce2d_partial<F>(uint32_t*, const uint32_t*, const uint32_t*, const uint4*,   \
                                                     R2Geom, uint32_t);                                          \
  PFX template __global__ void k_reduce_affine_finish<F>(uint32_t*, uint32_t*, const uint32_t*, const uint32_t*,  \
                                                         const uint2*, const uint4*, F2Geom);                     \
  MSMZ_INST_POLICY(WeierPolicy<F>, PFX)

#define MSMZ_INST_REDUCE_TE(F, Fr, PFX) MSMZ_INST_POLICY(TePolicy<F>, PFX)

#define MSMZ_INST_TEST(F, Fr, P, PFX)                                                                             \
  PFX template __global__ void k_test_field<F>(uint32_t*, const uint32_t*, const uint32_t*, uint32_t, int, uint32_t*); \
  PFX template __global__ void k_test_field_limbs<F>(int32_t*, uint32_t*, const int32_t*, const int32_t*, uint32_t,  \
                                                      int, uint32_t*);                                            \
  PFX template __global__ void k_test_field_rows<F>(int32_t*, uint32_t*, const int32_t*, const int32_t*, uint32_t,   \
                                                     int, uint32_t);                                              \
  PFX template __global__ void k_test_glv<Fr>(uint32_t*, uint32_t*, uint8_t*, const uint32_t*, uint32_t);         \
  PFX template __global__ void k_test_digits<Fr, false>(uint32_t*, const uint32_t*, uint32_t, int, int);          \
  PFX template __global__ void k_test_point<P>(uint32_t*, const uint32_t*, const uint32_t*, const uint8_t*,   \
                                                   const uint8_t*, uint32_t, int);                                \
  PFX template __global__ void k_test_point_raw<P>(uint32_t*, const uint32_t*, const uint32_t*, const uint8_t*, \
                                                       uint32_t, int, int);                                       \
  PFX template __global__ void k_test_accs_in<P>(uint32_t*, const uint32_t*, const uint8_t*, const uint32_t*, \
                                                     uint32_t, uint32_t*);                                        \
  PFX template __global__ void k_test_accs_out<P>(uint32_t*, const uint32_t*, uint32_t);

// one instance of the sort kernels (the list: MSMZ_SORT_INSTANCES, sort_kernels.h)
#define MSMZ_INST_SORT(Fr, PFX, GLV, C, SEG)                                                                      \
  PFX template __global__ void k_hist<Fr, GLV, C, SEG>(uint32_t*, uint16_t*, uint32_t*, MsmMeta*, const uint32_t*, SortGeom, uint32_t, const SegDesc*); \
  PFX template __global__ void k_coarse<Fr, GLV, C, SEG>(uint32_t*, const uint32_t*, const uint32_t*, const uint16_t*, const uint32_t*, SortGeom, uint32_t, const SegDesc*);

// the recurrence kernels of one mode (scan_kernels.h): AM = how the multiplier arrives, HB = is there an addend
#define MSMZ_INST_SCAN(Fr, AM, HB, PFX)                                                                           \
  PFX template __global__ void k_scalars_rec_tile<Fr, AM, HB>(uint32_t*, uint32_t*, const uint32_t*, const uint32_t*, FrConst, uint32_t, uint32_t, uint32_t*); \
  PFX template __global__ void k_scalars_rec_apply<Fr, AM, HB>(uint32_t*, const uint32_t*, const uint32_t*, FrConst, const uint32_t*, uint32_t, uint32_t);

#define MSMZ_INST_SCALAR(Fr, PFX)                                                                                 \
  PFX template __global__ void k_digits<Fr, false>(uint32_t*, uint32_t*, MsmMeta*, const uint32_t*, uint32_t, int, int, int, int); \
  MSMZ_SORT_INSTANCES(MSMZ_INST_SORT, Fr, PFX)                                                                    \
  PFX template __global__ void k_check_scalars<Fr>(uint32_t*, const uint32_t*, uint32_t);                         \
  PFX template __global__ void k_gen_scalars<Fr>(uint32_t*, uint32_t, uint64_t, GenMap);                          \
  PFX template __global__ void k_import_scalars<Fr>(uint32_t*, const uint8_t*, uint64_t, int, uint32_t, int, uint32_t*); \
  PFX template __global__ void k_export_scalars<Fr>(uint8_t*, uint64_t, int, const uint32_t*, uint32_t, int, uint32_t*); \
  PFX template __global__ void k_scalars_combine<Fr>(uint32_t*, ScalarTerm, ScalarTerm, uint32_t, uint32_t*);     \
  PFX template __global__ void k_scalars_dot<Fr>(uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t*); \
  PFX template __global__ void k_scalars_dot_fold<Fr>(uint32_t*, const uint32_t*, uint32_t, int);                 \
  PFX template __global__ void k_scalars_powers<Fr>(uint32_t*, FrConst, FrPowTable, uint32_t, GenMap);                \
  MSMZ_INST_SCAN(Fr, SREC_A_NONE, true, PFX)                                                                      \
  MSMZ_INST_SCAN(Fr, SREC_A_BROADCAST, false, PFX)                                                                \
  MSMZ_INST_SCAN(Fr, SREC_A_BROADCAST, true, PFX)                                                                 \
  MSMZ_INST_SCAN(Fr, SREC_A_RESIDENT, false, PFX)                                                                 \
  MSMZ_INST_SCAN(Fr, SREC_A_RESIDENT, true, PFX)                                                                  \
  PFX template __global__ void k_scalars_rec_carry<Fr, false, true>(uint32_t*, uint32_t*, const uint32_t*, const uint32_t*, FrConst, uint32_t); \
  PFX template __global__ void k_scalars_rec_carry<Fr, true, false>(uint32_t*, uint32_t*, const uint32_t*, const uint32_t*, FrConst, uint32_t); \
  PFX template __global__ void k_scalars_rec_carry<Fr, true, true>(uint32_t*, uint32_t*, const uint32_t*, const uint32_t*, FrConst, uint32_t); \
  PFX template __global__ void k_scalars_inverse<Fr>(uint32_t*, const uint32_t*, uint32_t, uint32_t*);         \
  PFX template __global__ void k_ntt_pass<Fr>(NttArgs);

// the multilinear kernels (mle_kernels.h), a translation unit of their own (kern_mle.hip); NT = the tables of a round
#define MSMZ_INST_SUMCHECK(Fr, NT, PFX)                                                                           \
  PFX template __global__ void k_scalars_sumcheck_round<Fr, NT>(uint32_t*, ScTables, FrScTerms, uint32_t, int, uint32_t*);
#define MSMZ_INST_SUMCHECK_STEP(Fr, NT, PFX)   /* NT = 1 .. MSC_STEP_FUSED_TABLES */                               \
  PFX template __global__ void k_scalars_sumcheck_step<Fr, NT>(uint32_t*, ScOuts, ScTables, FrScTerms, FrConst, uint32_t, int, uint32_t*);
#define MSMZ_INST_MLE(F, Fr, PFX)                                                                                 \
  PFX template __global__ void k_scalars_eq_table<Fr>(uint32_t*, FrConst, FrEqPoint, uint32_t);                   \
  PFX template __global__ void k_scalars_mle_eval<Fr>(uint32_t*, const uint32_t*, FrEqPoint, uint32_t, uint32_t*); \
  PFX template __global__ void k_scalars_mle_bind<Fr>(uint32_t*, const uint32_t*, FrConst, uint32_t, uint32_t, int, uint32_t*); \
  PFX template __global__ void k_scalars_sumcheck_last<Fr>(uint32_t*, ScOuts, ScTables, FrScTerms, FrConst, uint32_t, uint32_t*); \
  MSMZ_INST_SUMCHECK(Fr, 1, PFX) MSMZ_INST_SUMCHECK(Fr, 2, PFX) MSMZ_INST_SUMCHECK(Fr, 3, PFX)                    \
  MSMZ_INST_SUMCHECK(Fr, 4, PFX) MSMZ_INST_SUMCHECK(Fr, 5, PFX) MSMZ_INST_SUMCHECK(Fr, 6, PFX)                    \
  MSMZ_INST_SUMCHECK_STEP(Fr, 1, PFX) MSMZ_INST_SUMCHECK_STEP(Fr, 2, PFX) MSMZ_INST_SUMCHECK_STEP(Fr, 3, PFX)     \
  MSMZ_INST_SUMCHECK_STEP(Fr, 4, PFX) MSMZ_INST_SUMCHECK_STEP(Fr, 5, PFX)

// the sparse-matrix kernels (matrix_kernels.h), a translation unit of their own (kern_matrix.hip)
#define MSMZ_INST_MATRIX(F, Fr, PFX)                                                                              \
  PFX template __global__ void k_matrix_pack<Fr>(uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t*); \
  PFX template __global__ void k_matrix_mul<Fr>(uint32_t*, MatView, const uint32_t*, uint32_t, uint32_t*, uint32_t*); \
  PFX template __global__ void k_matrix_fold<Fr>(uint32_t*, const uint32_t*, uint32_t);

// the lookup kernels (lookup_kernels.h), a translation unit of their own (kern_lookup.hip)
#define MSMZ_INST_LOOKUP(F, Fr, PFX)                                                                              \
  PFX template __global__ void k_lookup_insert<Fr>(uint32_t*, uint32_t, const uint32_t*, uint32_t, uint32_t*);    \
  PFX template __global__ void k_lookup_count<Fr>(uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t, const uint32_t*, const uint32_t*, uint32_t); \
  PFX template __global__ void k_lookup_count_small<Fr>(uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t, const uint32_t*, uint32_t, const uint32_t*, uint32_t); \
  PFX template __global__ void k_lookup_emit<Fr>(uint32_t*, const uint32_t*, uint32_t);

// the gate-expression kernels (expr_kernels.h), a translation unit of their own (kern_expr.hip)
#define MSMZ_INST_EXPR(F, Fr, PFX)                                                                                \
  PFX template __global__ void k_scalars_expr<Fr>(uint32_t*, ExprProgram, uint32_t*);                             \
  PFX template __global__ void k_scalars_expr_slots<Fr, EXPR_REGISTER_SLOTS>(uint32_t*, ExprProgram, uint32_t*);

// the batched inner products (dot_kernels.h), a translation unit of their own (kern_dot.hip); NC = the columns
#define MSMZ_INST_DOT_MANY(Fr, NC, PFX)                                                                           \
  PFX template __global__ void k_scalars_dot_many<Fr, NC>(uint32_t*, DotManyVecs, uint32_t, uint32_t, uint32_t, uint32_t*);
#define MSMZ_INST_DOT(F, Fr, PFX)                                                                                 \
  MSMZ_INST_DOT_MANY(Fr, 1, PFX) MSMZ_INST_DOT_MANY(Fr, 2, PFX) MSMZ_INST_DOT_MANY(Fr, 3, PFX)                    \
  MSMZ_INST_DOT_MANY(Fr, 4, PFX) MSMZ_INST_DOT_MANY(Fr, 5, PFX) MSMZ_INST_DOT_MANY(Fr, 6, PFX)                    \
  MSMZ_INST_DOT_MANY(Fr, 7, PFX) MSMZ_INST_DOT_MANY(Fr, 8, PFX)

// every curve, by policy P = WeierPolicy<F> / TePolicy<F>
#define MSMZ_INST_MISC_P(F, Fr, P, PFX)                                                                           \
  PFX template __global__ void k_points_to_resident<P>(uint32_t*, const uint32_t*, const uint8_t*, uint32_t, int, uint32_t*); \
  PFX template __global__ void k_points_from_resident<P>(uint32_t*, const uint32_t*, uint32_t);                   \
  PFX template __global__ void k_import_points<P>(uint32_t*, const uint8_t*, uint64_t, const uint8_t*, uint32_t, int, int, uint32_t*); \
  PFX template __global__ void k_import_points_compressed<P>(uint32_t*, const uint8_t*, uint64_t, const uint8_t*, uint32_t, int, int, uint32_t*); \
  PFX template __global__ void k_points_compress<P>(uint32_t*, uint8_t*, const uint32_t*, uint32_t, int);         \
  PFX template __global__ void k_export_points<P>(uint8_t*, uint64_t, uint8_t*, const uint32_t*, uint32_t, int); \
  PFX template __global__ void k_check_curve<P>(uint8_t*, CheckResult*, const uint32_t*, uint32_t, uint32_t);     \
  PFX template __global__ void k_check_subgroup<P, Fr>(uint8_t*, CheckResult*, const uint32_t*, uint32_t, uint32_t); \
  PFX template __global__ void k_points_mul<P, Fr, false>(uint32_t*, const uint32_t*, const uint32_t*, MulScalar, const uint32_t*, uint32_t, int, int, uint32_t*); \
  PFX template __global__ void k_points_mul<P, Fr, true>(uint32_t*, const uint32_t*, const uint32_t*, MulScalar, const uint32_t*, uint32_t, int, int, uint32_t*); \
  MSMZ_INST_TEST(F, Fr, P, PFX)                                                                                   \
  MSMZ_INST_SCALAR(Fr, PFX)

// ... and what only the Weierstrass pipeline has
#define MSMZ_INST_MISC(F, Fr, PFX)                                                                                \
  MSMZ_INST_MISC_P(F, Fr, WeierPolicy<F>, PFX)                                                                    \
  PFX template __global__ void k_precompute_copy<F>(uint32_t*, const uint32_t*, uint32_t, int, int);              \
  PFX template __global__ void k_points_mul_glv<WeierPolicy<F>, Fr>(uint32_t*, const uint32_t*, const uint32_t*, MulGlvScalar, const uint32_t*, uint32_t, int, int, uint32_t*); \
  PFX template __global__ void k_digits<Fr, true>(uint32_t*, uint32_t*, MsmMeta*, const uint32_t*, uint32_t, int, int, int, int); \
  MSMZ_SORT_INSTANCES_WEIERSTRASS(MSMZ_INST_SORT, Fr, PFX)                                                        \
  PFX template __global__ void k_test_digits<Fr, true>(uint32_t*, const uint32_t*, uint32_t, int, int);           \
  PFX template __global__ void k_test_slots_in<F>(uint32_t*, const uint32_t*, const uint8_t*, uint32_t, uint32_t*); \
  PFX template __global__ void k_test_slots_out<F>(uint32_t*, const uint32_t*, uint32_t, uint32_t);

#define MSMZ_INST_MISC_TE(F, Fr, PFX) MSMZ_INST_MISC_P(F, Fr, TePolicy<F>, PFX)

// the generators, and the fixed-base kernels beside them (fixed_kernels.h)
#define MSMZ_INST_GEN_P(P, Fr, PFX)                                              \
  PFX template __global__ void k_gen_table<P>(uint32_t*, const uint32_t*);       \
  PFX template __global__ void k_gen_points<P>(uint32_t*, const uint32_t*, uint32_t, uint64_t, int, GenMap); \
  PFX template __global__ void k_fixed_table<P>(uint32_t*, const uint32_t*, uint32_t, int); \
  PFX template __global__ void k_fixed_mul<P, Fr, false>(uint32_t*, const uint32_t*, const uint32_t*, uint32_t, int, int, int, int, uint32_t*); \
  PFX template __global__ void k_fixed_mul<P, Fr, true>(uint32_t*, const uint32_t*, const uint32_t*, uint32_t, int, int, int, int, uint32_t*);
#define MSMZ_INST_GEN(F, Fr, PFX) MSMZ_INST_GEN_P(WeierPolicy<F>, Fr, PFX)
#define MSMZ_INST_GEN_TE(F, Fr, PFX) MSMZ_INST_GEN_P(TePolicy<F>, Fr, PFX)

#define MSMZ_EXTERN extern
#define MSMZ_DEFINE

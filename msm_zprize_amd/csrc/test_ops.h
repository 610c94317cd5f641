// Field operations on raw register limbs, shared by the device test hook (k_test_field_limbs, test_kernels.h) and the
// host contract driver (tests/native/fp_contract_test.cpp), so both run the same code on the same limbs and their
// outputs can be compared bit for bit.  Never part of an MSM.
#pragma once
#include "curve.h"

namespace msmz {

enum {   // ops of msmz_test_field_limbs (include/msmz_test.h)
  TFL_MUL = 0, TFL_SQR = 1, TFL_REDUCE_SMALL = 2, TFL_STORE = 3, TFL_STORE_MULOUT = 4, TFL_IS_ZERO = 5, TFL_CARRY = 6,
  TFL_NORMALIZE = 7, TFL_INVERSE = 8, TFL_INVERSE_WAVE = 9, TFL_SLOT_MULOUT = 10, TFL_SLOT_POINT = 11, TFL_COUNT = 12
};

// raw[N]: the routine's output limbs, or its memory words (STORE, STORE_MULOUT; words NW..N-1 zero), or the flag
// (IS_ZERO: raw[0]).  canon[NW]: the canonical value of that output, through fe_to_canon_words; 0 for IS_ZERO and
// for CARRY / NORMALIZE, whose input may lie outside fe_store's |v| < 2^4 p (their value is the sum of the raw limbs).
// Returns false for an op this function does not run (the device-only ones: INVERSE_WAVE, SLOT_*).
template <class F>
MSMZ_HD bool field_limbs_op(int op, const Fe<F>& a, const Fe<F>& b, int32_t* raw, uint32_t* canon) {
  constexpr int N = F::N, NW = F::NW;
  Fe<F> r;
  uint32_t w[NW];
  bool words = false;
  fe_zero(r);
  switch (op) {
    case TFL_MUL: fe_mul(r, a, b); break;
    case TFL_SQR: fe_sqr(r, a); break;
    case TFL_REDUCE_SMALL: r = a; fe_reduce_small(r); break;
    case TFL_STORE: fe_store<F>(w, a); words = true; break;
    case TFL_STORE_MULOUT: fe_store_mulout<F>(w, a); words = true; break;
    case TFL_IS_ZERO: r.l[0] = fe_is_zero(a) ? 1 : 0; break;
    case TFL_CARRY: r = a; fe_carry(r); break;
    case TFL_NORMALIZE: r = a; fe_normalize(r); break;
    case TFL_INVERSE: fe_inverse(r, a); break;
    default: return false;
  }
  if (words) {
#pragma unroll
    for (int j = 0; j < N; j++) raw[j] = j < NW ? (int32_t)w[j] : 0;
    fe_unpack<F>(r, w);
  } else {
#pragma unroll
    for (int j = 0; j < N; j++) raw[j] = r.l[j];
  }
  if (op == TFL_IS_ZERO || op == TFL_CARRY || op == TFL_NORMALIZE) {
#pragma unroll
    for (int j = 0; j < NW; j++) canon[j] = 0;
  } else {
    fe_to_canon_words<F>(canon, r);
  }
  return true;
}

}  // namespace msmz

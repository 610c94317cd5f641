// Gate expressions over resident scalar sets (msmz_scalars_expr, include/msmz.h):
//     out_i = sum_T c_T prod_(f in T) col_(f.column)[(i + f.rot) mod n]   mod q,   i < n
// on canonical 8-word records with the F_q functions of fr.h.  The first part of this file is host/device code: the
// index function, the program a kernel takes, the compile step that turns the caller's description into it (host
// only: it answers in the status codes of include/msmz.h and knows nothing of handles), the overlap rule and the
// body of one entry, all of which tests/native/expr_test.cpp runs on the CPU.  The kernels follow, for the device
// compiler only.
#pragma once
#include "../../include/msmz.h"
#include "mle_kernels.h"   // fr_sc_coeff, static_for (sqrt.h)
#include "ranges.h"

namespace msmz {

constexpr int EXPR_MAX_COLUMNS = 16;
constexpr int EXPR_MAX_TERMS = 32;
constexpr int EXPR_MAX_DEGREE = 8;
constexpr int EXPR_MAX_OPERANDS = 32;
constexpr int EXPR_THREADS = 256;   // one thread per output entry
// the register-resident variant (k_scalars_expr_slots) holds at most this many operands, whatever instance is built
constexpr int EXPR_SLOTS_MAX = 8;
// Programs of at most EXPR_REGISTER_SLOTS operands take the register-resident kernel, the others k_scalars_expr.  4 is
// what the measurements of DESIGN.md section 29 leave: 5 to 7 % ahead on a gate with a repeated factor (a^5 + c b -
// a[+1], 3 operands), level on gates without one, while 8 slots (220+ VGPRs, 2 waves per SIMD) lose everywhere.
constexpr int EXPR_REGISTER_SLOTS = 4;
static_assert(EXPR_REGISTER_SLOTS >= 1 && EXPR_REGISTER_SLOTS <= EXPR_SLOTS_MAX, "a slot count the exponent word can name");
static_assert(EXPR_MAX_COLUMNS == MSMZ_EXPR_MAX_COLUMNS && EXPR_MAX_TERMS == MSMZ_EXPR_MAX_TERMS &&
                  EXPR_MAX_DEGREE == MSMZ_EXPR_MAX_DEGREE && EXPR_MAX_OPERANDS == MSMZ_EXPR_MAX_OPERANDS,
              "the limits of include/msmz.h are those of expr_kernels.h");
static_assert(EXPR_MAX_DEGREE == 8 && EXPR_MAX_OPERANDS <= 256, "a term's operand indices are the eight bytes of one word");
static_assert(EXPR_MAX_DEGREE < 16 && EXPR_SLOTS_MAX == 8, "a term's exponents are the eight nibbles of one word");

// (i + rot) mod n for i < n, rot < n, 1 <= n < 2^32.  No sum is formed that can wrap: i + rot is only taken where it
// stays below n.
MSMZ_HD uint32_t expr_index(uint32_t i, uint32_t rot, uint32_t n) {
  const uint32_t left = n - rot;   // entries from i = 0 up to the wrap; n when rot == 0
  return i >= left ? i - left : i + rot;
}

// a caller's rotation, any int32, brought to [0, n)
inline uint32_t expr_reduce_rot(int32_t rot, uint64_t n) {
  const int64_t r = (int64_t)rot % (int64_t)n;
  return (uint32_t)(r < 0 ? r + (int64_t)n : r);
}

// One distinct (column, rotation) pair: the first record of the column's range and the reduced rotation.
struct ExprOperand {
  const uint32_t* base;
  uint32_t rot;
  uint32_t column;   // the caller's column index (host: resolving the base, the overlap rule; the kernels ignore it)
};

// The program of one call, passed to the kernels by value (it arrives in the argument segment, 1.9 KB).  Term k is
// coeff[k] times the operands ops[k] names in its low n_factors[k] bytes, a repeated factor named as often as it
// occurs; coeff[k] = c 2^(256 f) mod q for a term of f factors (fr_sc_coeff), so that f products through fr_mont_mul
// with canonical records leave c prod, canonical, and terms of different degree add as they are.  expo[k] holds the
// same term as one exponent per operand, a nibble each, for the register-resident kernel; it is filled only while the
// program has at most EXPR_SLOTS_MAX operands.
struct ExprProgram {
  ExprOperand op[EXPR_MAX_OPERANDS];
  uint32_t coeff[EXPR_MAX_TERMS][8];
  uint64_t ops[EXPR_MAX_TERMS];
  uint32_t expo[EXPR_MAX_TERMS];
  uint8_t n_factors[EXPR_MAX_TERMS];
  uint32_t n_terms, n_ops, n;
  uint32_t rotated;   // does any operand have rot != 0?
};
static_assert(sizeof(ExprProgram) <= 2048, "the program travels as a kernel argument");

// The compile step, part one: the structure.  MSMZ_ERR_ARG for a null pointer, a count outside its bounds, non-zero
// flags or `reserved`, a column index >= n_columns, or more than EXPR_MAX_OPERANDS distinct (column, rot mod n) pairs.
// The bases stay null: the engine fills them from the handles.  named[c] = 1: some factor reads column c at rotation
// 0 only, 3: some factor reads it rotated, 0: no factor reads it.
inline int expr_compile(const msmz_expr& e, ExprProgram* P, uint8_t named[EXPR_MAX_COLUMNS]) {
  if (!e.columns || !e.terms || e.n_columns < 1 || e.n_columns > (uint32_t)EXPR_MAX_COLUMNS || e.n_terms < 1 ||
      e.n_terms > (uint32_t)EXPR_MAX_TERMS || e.n == 0 || e.n >> 32 || e.flags)
    return MSMZ_ERR_ARG;
  *P = ExprProgram{};
  for (int c = 0; c < EXPR_MAX_COLUMNS; c++) named[c] = 0;
  P->n = (uint32_t)e.n;
  P->n_terms = e.n_terms;
  for (uint32_t k = 0; k < e.n_terms; k++) {
    const msmz_expr_term& t = e.terms[k];
    if (t.reserved || t.n_factors > (uint32_t)EXPR_MAX_DEGREE || (t.n_factors && !t.factors)) return MSMZ_ERR_ARG;
    P->n_factors[k] = (uint8_t)t.n_factors;
    for (uint32_t f = 0; f < t.n_factors; f++) {
      const uint32_t col = t.factors[f].column;
      if (col >= e.n_columns) return MSMZ_ERR_ARG;
      const uint32_t rot = expr_reduce_rot(t.factors[f].rot, e.n);
      named[col] |= rot ? 3 : 1;
      uint32_t o = 0;
      while (o < P->n_ops && !(P->op[o].column == col && P->op[o].rot == rot)) o++;
      if (o == P->n_ops) {
        if (o == (uint32_t)EXPR_MAX_OPERANDS) return MSMZ_ERR_ARG;
        P->op[o].column = col, P->op[o].rot = rot;
        P->n_ops++;
        if (rot) P->rotated = 1;
      }
      P->ops[k] |= (uint64_t)o << (8 * f);
    }
  }
  for (uint32_t k = 0; k < e.n_terms && P->n_ops <= (uint32_t)EXPR_SLOTS_MAX; k++)
    for (uint32_t f = 0; f < P->n_factors[k]; f++) P->expo[k] += 1u << (4 * ((P->ops[k] >> (8 * f)) & 0xff));
  return MSMZ_OK;
}

// Part two, once every MSMZ_ERR_ARG is behind: the coefficients, 32 little-endian bytes each or null = 1, brought to
// c 2^(256 f).  MSMZ_ERR_RANGE for one >= q.
template <class Fr>
inline int expr_coeffs(const msmz_expr& e, ExprProgram* P) {
  for (uint32_t k = 0; k < e.n_terms; k++) {
    uint32_t c[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    if (e.terms[k].coeff) {
      for (int w = 0; w < 8; w++) {
        const uint8_t* b = e.terms[k].coeff + 4 * w;
        c[w] = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
      }
      if (words_geq<8>(c, Fr::Q)) return MSMZ_ERR_RANGE;
    }
    fr_sc_coeff<Fr>(P->coeff[k], c, P->n_factors[k]);
  }
  return MSMZ_OK;
}

// The overlap rule for ONE column range [first, first + n) on the destination's handle against the destination
// [first_out, first_out + n): may the call go ahead?  named: 0 = no factor reads the column (anything goes), 1 = read
// at rotation 0 only (the exact range or apart), 3 = read rotated (apart).
inline bool expr_overlap_ok(uint8_t named, uint64_t first, uint64_t first_out, uint64_t n) {
  if (!named) return true;
  return named & 2 ? !ranges_meet(first, n, first_out, n) : !partial_overlap(first, first_out, n);
}

// The body of one entry: acc = sum_T c_T prod ..., canonical; true if a record read for it is >= q.  load(v, base, at)
// reads record `at` behind `base` and says whether it is >= q: every operand of entry i is read through it here, and
// the caller writes entry i only afterwards (the in-place rule rests on that).  The loops, the operand indices and the
// coefficients are the same in every lane: `o` indexes the program in the argument segment, never a register array.
template <class Fr, class Load>
MSMZ_HD bool fr_expr_entry(uint32_t* acc, const ExprProgram& P, uint32_t i, Load load) {
#pragma unroll
  for (int w = 0; w < 8; w++) acc[w] = 0;
  bool bad = false;
#pragma unroll 1
  for (uint32_t k = 0; k < P.n_terms; k++) {
    uint32_t p[8];
#pragma unroll
    for (int w = 0; w < 8; w++) p[w] = P.coeff[k][w];
    uint64_t ops = P.ops[k];
#pragma unroll 1
    for (uint32_t f = P.n_factors[k]; f; f--, ops >>= 8) {
      const ExprOperand& op = P.op[ops & 0xff];
      uint32_t v[8];
      bad |= load(v, op.base, expr_index(i, op.rot, P.n));
      fr_mont_mul<Fr>(p, p, v);   // (p < q: the product ends below q whatever the record is)
    }
    fr_add<Fr>(acc, acc, p);
  }
  return bad;
}

// The same entry with every operand read ONCE into v[S], S >= P.n_ops, and the terms applied from there: slot J enters
// term k expo-nibble-J times.  Every index into v is a constant after unrolling; the exponents are uniform.  The
// products of a term run in slot order, not in the caller's factor order: multiplication mod q is exact, so the bytes
// are those of fr_expr_entry.
template <class Fr, int S, class Load>
MSMZ_HD bool fr_expr_entry_slots(uint32_t* acc, const ExprProgram& P, uint32_t i, Load load) {
  uint32_t v[S][8];
  bool bad = false;
  static_for<0, S>([&](auto J) {
    if ((uint32_t)J < P.n_ops) bad |= load(v[J], P.op[J].base, expr_index(i, P.op[J].rot, P.n));
  });
#pragma unroll
  for (int w = 0; w < 8; w++) acc[w] = 0;
#pragma unroll 1
  for (uint32_t k = 0; k < P.n_terms; k++) {
    uint32_t p[8];
#pragma unroll
    for (int w = 0; w < 8; w++) p[w] = P.coeff[k][w];
    const uint32_t ex = P.expo[k];
    static_for<0, S>([&](auto J) {
#pragma unroll 1
      for (uint32_t e = (ex >> (4 * J)) & 15u; e; e--) fr_mont_mul<Fr>(p, p, v[J]);
    });
    fr_add<Fr>(acc, acc, p);
  }
  return bad;
}

}  // namespace msmz

#if defined(__HIPCC__)
namespace msmz {

// out_i = the expression at entry i, one thread per entry (fr_expr_entry): every operand of i is read, then record i is
// written, so `out` may be exactly the range of a column that is read at rotation 0 only; the host refuses every other
// overlap with a column some factor names.  A record >= q raises bit 2 of *err.  No occupancy bound: left to the compiler
// the kernel takes 82 to 84 VGPRs without scratch, 5 waves per SIMD; bound to 8 waves it fits 64 VGPRs by spilling 80
// bytes per lane inside the factor loop and is 10 to 45 % slower on every gate measured.
template <class Fr>
__global__ void __launch_bounds__(EXPR_THREADS) k_scalars_expr(uint32_t* out, ExprProgram P, uint32_t* err) {
  const uint64_t at = (uint64_t)blockIdx.x * EXPR_THREADS + threadIdx.x;
  if (at >= P.n) return;
  uint32_t acc[8];
  const bool bad = fr_expr_entry<Fr>(acc, P, (uint32_t)at,
                                     [](uint32_t* v, const uint32_t* base, uint32_t j) { return fr_load<Fr>(v, base, j); });
  if (bad) atomicOr(err, 4u);
  fr_store(out, at, acc);
}

// the register-resident variant for programs of at most S operands (fr_expr_entry_slots): the same bytes
template <class Fr, int S>
__global__ void __launch_bounds__(EXPR_THREADS) k_scalars_expr_slots(uint32_t* out, ExprProgram P, uint32_t* err) {
  const uint64_t at = (uint64_t)blockIdx.x * EXPR_THREADS + threadIdx.x;
  if (at >= P.n) return;
  uint32_t acc[8];
  const bool bad = fr_expr_entry_slots<Fr, S>(acc, P, (uint32_t)at, [](uint32_t* v, const uint32_t* base, uint32_t j) {
    return fr_load<Fr>(v, base, j);
  });
  if (bad) atomicOr(err, 4u);
  fr_store(out, at, acc);
}

}  // namespace msmz
#endif

// Row-form field arithmetic (device only): one field element spread over the 16 lanes of a DPP row.
//
// fe_mul (fp.h) sums 2 N^2 products into ONE 64-bit accumulator, so a lane that runs it alone waits for ~2 N^2
// dependent v_mad_i64_i32.  Where a kernel is bound by that latency and not by VALU throughput (a few waves on the
// whole device, every product waiting for the one before) the same product is done here by 16 lanes at once:
// 2 N dependent multiply-adds plus the row exchanges.  It costs several times more wave-instructions per product and
// belongs nowhere near a throughput-bound kernel.
//
// Layout
//   A row element is ONE int32_t per lane: lane j < F::N of the row holds limb j (radix 2^W, signed, lazy, exactly
//   the limbs of Fe<F>), lanes N..15 hold 0.  Every routine keeps lanes N..15 at 0.  The four rows of a wave are four
//   independent elements.  All 64 lanes must be active: DPP moves read their neighbours' registers, and
//   limb_row_ripple / fe_is_zero_row vote over the wave.
//   RowLane<F> holds what a lane needs to know about its own limb position (limb index, p_j, -p_j, (2p)_j); a kernel
//   builds it once.
//
// Contracts (the per-lane ones of fp.h, limb for limb)
//   fe_mul_row inputs : |value| < 2^5 p (2^3 p for the 255-bit fields); limb magnitudes A, B of the two operands with
//                       A*B + 2^(2W) + 2^(W+1) < 2^62.  That is looser than fe_mul's N*A*B + N*2^(2W) < 2^63 for
//                       every N >= 2, so whatever fe_mul accepts is accepted here.
//   fe_mul_row output : as fe_mul: value in (-1.5p, 0.5p), limbs 0..N-2 in [0, 2^W), signed top limb.
//   fe_reduce_small_row, fe_store_row, fe_is_zero_row : |value| < 2^4 p, any limb form fe_reduce_small accepts.
//   fe_store_row writes THE memory range [0, 3p) -- the same words fe_store writes for the same limbs.
#pragma once
#include "fp.h"

#if defined(__HIPCC__)
namespace msmz {

template <class F>
struct RowLane {
  int j;         // limb index of this lane within its row, 0..15
  int32_t pl;    // p_j      (0 for j >= N)
  int32_t npl;   // -p_j
  int32_t p2;    // (2p)_j, normalized limbs
  int32_t one;   // limb j of the Montgomery form of 1
};

// limb j of a constant element (a select chain over the N limbs: fetch once, outside loops)
template <class F>
__device__ __forceinline__ int32_t row_const(const int32_t (&c)[F::N], int j) {
  int32_t v = 0;
#pragma unroll
  for (int i = 0; i < F::N; i++) v = j == i ? c[i] : v;
  return v;
}

template <class F>
__device__ __forceinline__ RowLane<F> row_lane() {
  static_assert(F::N <= 15, "one DPP row per element");
  RowLane<F> k;
  k.j = (int)(__lane_id() & 15u);
  k.pl = row_const<F>(F::PL, k.j);
  k.npl = -k.pl;
  k.p2 = row_const<F>(F::P2, k.j);
  k.one = row_const<F>(F::ONE, k.j);
  return k;
}

// ---------------------------------------------------------------------------------- row moves
template <int I>
__device__ __forceinline__ int32_t row_bcast(int32_t x) {   // row_newbcast:I : every lane takes lane I of its row
  return __builtin_amdgcn_update_dpp(0, x, 0x150 + I, 0xf, 0xf, false);
}
__device__ __forceinline__ int32_t row_down1(int32_t x) {    // row_shl:1 : lane j takes lane j+1, lane 15 takes 0
  return __builtin_amdgcn_update_dpp(0, x, 0x101, 0xf, 0xf, true);
}
__device__ __forceinline__ int32_t row_up1(int32_t x) {      // row_shr:1 : lane j takes lane j-1, lane 0 takes 0
  return __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);
}

// Full carry of a row: limbs 0..N-2 to [0, 2^W), the top limb keeps the sign.  A carry moves up one limb per pass;
// after the second pass a further carry needs a limb within 4 of 2^W, so the loop almost always ends after two or
// three passes (and always within N - 1).  The vote is over the wave: a row that is done repeats passes that no longer
// change it.
template <int W, int N>
__device__ __forceinline__ int32_t limb_row_ripple(int32_t val, int j) {
  constexpr int32_t MASK = (1 << W) - 1;
  const bool low = j < N - 1;          // limbs below the (signed) top limb are reduced to [0, 2^W)
#pragma unroll 1
  for (int pass = 0; pass < N - 1; pass++) {
    const int32_t c = low ? (val >> W) : 0;
    val = low ? (val & MASK) : val;
    val += row_up1(c);
    if (__ballot(low && (uint32_t)val > (uint32_t)MASK) == 0) break;
  }
  return val;
}

// ---------------------------------------------------------------------------------- limb-wise operations
// add, subtract and negate are plain integer operations on the one register (a + b, a - b, -a): no routine needed.

// One parallel carry pass (fe_carry): limbs 0..N-2 come back within [0, 2^W + small), value unchanged.
template <class F>
__device__ __forceinline__ int32_t fe_carry_row(int32_t a, const RowLane<F>& k) {
  constexpr int32_t MASK = (1 << F::W) - 1;
  const bool low = k.j < F::N - 1;
  const int32_t c = low ? (a >> F::W) : 0;
  return (low ? (a & MASK) : a) + row_up1(c);
}

__device__ __forceinline__ int32_t fe_select_row(bool c, int32_t a, int32_t b) { return c ? a : b; }

// ---------------------------------------------------------------------------------- Montgomery product
// Operand scanning with the reduction interleaved.  Lane j carries column j in a 64-bit sum; step i:
//     acc_j += a_i b_j                    a_i by row_newbcast:i (off the dependent chain: a does not change)
//     m      = acc_0 p^-1 mod 2^W         the low word of lane 0 by row_newbcast:0
//     acc_j += m (-p_j)                   now acc_0 = 0 mod 2^W
//     acc_j  = (acc_j >> W) + (acc_{j+1} mod 2^W)     division by 2^W: the low parts move down one lane (row_shl:1),
//                                                     the high part stays where it is
// After N steps the row holds a b / R - (sum m_i 2^(W i)) p / R, in (-1.5p, 0.5p) as for fe_mul.
// No overflow: before a step |acc_j| <= (|acc'_j| >> W) + 2^W, and a step adds at most A*B + 2^(2W); so
// |acc_j| < (A*B + 2^(2W) + 2^W) (1 + 2^-W + ...) < 2^62 under the contract above.  After the last step the low
// columns are below 2^(63-W) in magnitude; one 64-bit carry pass brings them to 32 bits (|carry| < 2^(63-2W) <= 2^7),
// and the top column is small because the value is (|top| 2^(W(N-1)) <= |value| + the columns below).
template <class F, int I>
struct RowMulStep {
  static __device__ __forceinline__ void run(int64_t& acc, int32_t a, int32_t b, int32_t npl) {
    constexpr uint32_t MASK = (1u << F::W) - 1u;
    int32_t ai = row_bcast<I>(a);
    MSMZ_OPAQUE_LIMB(ai);
    acc += (int64_t)ai * (int64_t)b;
    uint32_t q = (uint32_t)row_bcast<0>((int32_t)(uint32_t)acc);
    if (F::PINV != 1u) q *= F::PINV;
    int32_t m = (int32_t)(q & MASK);
    MSMZ_OPAQUE_LIMB(m);
    acc += (int64_t)m * (int64_t)npl;
    const int32_t lo = (int32_t)((uint32_t)acc & MASK);
    acc = (acc >> F::W) + (int64_t)row_down1(lo);
    if constexpr (I + 1 < F::N) RowMulStep<F, I + 1>::run(acc, a, b, npl);
  }
};

template <class F>
__device__ __forceinline__ int32_t fe_mul_row(int32_t a, int32_t b, const RowLane<F>& k) {
  constexpr int N = F::N, W = F::W;
  constexpr uint32_t MASK = (1u << W) - 1u;
  int32_t npl = k.npl;
  MSMZ_OPAQUE_LIMB(b);
  MSMZ_OPAQUE_LIMB(npl);
  int64_t acc = 0;
  RowMulStep<F, 0>::run(acc, a, b, npl);
  const bool low = k.j < N - 1;
  const int32_t c = low ? (int32_t)(acc >> W) : 0;
  int32_t v = low ? (int32_t)((uint32_t)acc & MASK) : (int32_t)acc;
  v += row_up1(c);
  return limb_row_ripple<W, N>(v, k.j);
}

template <class F>
__device__ __forceinline__ int32_t fe_sqr_row(int32_t a, const RowLane<F>& k) {   // latency-bound: halving the products buys nothing
  return fe_mul_row<F>(a, a, k);
}

// ---------------------------------------------------------------------------------- reduction, zero test
// fe_reduce_small on a row: the same quotient estimate from the two top limbs (broadcast to the row), a -= q p, full
// carry.  Result in [0, 3p) with normalized limbs -- limb for limb what fe_reduce_small gives.
template <class F>
__device__ __forceinline__ int32_t fe_reduce_small_row(int32_t a, const RowLane<F>& k) {
  constexpr int N = F::N, W = F::W;
  constexpr uint32_t MASK = (1u << W) - 1u;
  const int32_t est = row_bcast<N - 1>(a) + (row_bcast<N - 2>(a) >> W);
  constexpr int SH = (F::PL[N - 1] >= (1 << 16)) ? 8 : 0;
  const float x = (float)(est >> SH) * (1.0f / (float)((F::PL[N - 1] >> SH) + 1));
  const int32_t q = (int32_t)__builtin_floorf(x) - 1;
  const int64_t t = (int64_t)a + (int64_t)q * (int64_t)k.npl;   // q p_j may exceed 32 bits
  const bool low = k.j < N - 1;
  const int32_t c = low ? (int32_t)(t >> W) : 0;
  int32_t v = low ? (int32_t)((uint32_t)t & MASK) : (int32_t)t;
  v += row_up1(c);
  return limb_row_ripple<W, N>(v, k.j);
}

// is the element 0 mod p?  The same answer in all 16 lanes of the row.
template <class F>
__device__ __forceinline__ bool fe_is_zero_row(int32_t a, const RowLane<F>& k) {
  if constexpr (F::PL[0] == 1) {
    // p = 1 mod 2^W: k p has limb 0 = k mod 2^W, |k| <= 15 (the filter of fe_is_zero, curve.h); no row passes: done
    constexpr uint32_t MASK = (1u << F::W) - 1u;
    if (__ballot(k.j == 0 && (((uint32_t)a + 15u) & MASK) <= 30u) == 0) return false;
  }
  const int32_t v = fe_reduce_small_row<F>(a, k);   // [0, 3p), normalized: zero iff it is 0, p or 2p
  const int sh = (int)(__lane_id() & 48u);
  const uint32_t n0 = (uint32_t)(__ballot(v != 0) >> sh) & 0xffffu;
  const uint32_t n1 = (uint32_t)(__ballot(v != k.pl) >> sh) & 0xffffu;
  const uint32_t n2 = (uint32_t)(__ballot(v != k.p2) >> sh) & 0xffffu;
  return n0 == 0 || n1 == 0 || n2 == 0;
}

// ---------------------------------------------------------------------------------- memory format
// words (saturated, any value below 2^(32 NW)) -> normalized row limbs; lane j reads the one or two words its limb
// straddles.  All lanes of the row pass the same pointer.
template <class F>
__device__ __forceinline__ int32_t fe_load_row(const uint32_t* w, const RowLane<F>& k) {
  constexpr int N = F::N, W = F::W, NW = F::NW;
  constexpr uint32_t MASK = (1u << W) - 1u;
  if (k.j >= N) return 0;
  const int bit = W * k.j;
  const int w0 = bit >> 5, sh = bit & 31;
  uint32_t v = w[w0] >> sh;
  if (sh + W > 32 && w0 + 1 < NW) v |= w[w0 + 1] << (32 - sh);
  return (int32_t)(v & MASK);
}

// normalized, non-negative row limbs -> words: lane i < NW gathers the (up to three) limbs of word i and writes it
// (write = false: this row only takes part in the moves, e.g. a copy of an element another row stores)
template <class F>
__device__ __forceinline__ void fe_pack_row(uint32_t* w, int32_t a, const RowLane<F>& k, bool write = true) {
  constexpr int W = F::W, NW = F::NW;
  static_assert((32 * (NW - 1)) / W + 2 <= 15, "a word's limbs lie within the row");
  const int i = k.j < NW ? k.j : 0;
  const int j0 = (32 * i) / W, o = 32 * i - W * j0;
  const int base = (int)(__lane_id() & 48u) + j0;
  const uint32_t l0 = (uint32_t)__shfl(a, base, 64);
  const uint32_t l1 = (uint32_t)__shfl(a, base + 1, 64);   // lanes N..15 hold 0
  const uint32_t l2 = (uint32_t)__shfl(a, base + 2, 64);
  uint32_t v = (l0 >> o) | (l1 << (W - o));
  if (2 * W - o < 32) v |= l2 << (2 * W - o);
  if (write && k.j < NW) w[k.j] = v;
}

// store a lazy row (|v| < 2^4 p) as a memory-format residue in [0, 3p)
template <class F>
__device__ __forceinline__ void fe_store_row(uint32_t* w, int32_t a, const RowLane<F>& k, bool write = true) {
  fe_pack_row<F>(w, fe_reduce_small_row<F>(a, k), k, write);
}

// move an element between rows: every lane takes the limb of its own position from row `src_row` (0..3)
__device__ __forceinline__ int32_t fe_from_row(int32_t a, int src_row) {
  return __shfl(a, src_row * 16 + (int)(__lane_id() & 15u), 64);
}

}  // namespace msmz
#endif  // __HIPCC__

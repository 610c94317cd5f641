// Number-theoretic transforms over resident scalar sets (msmz_scalars_ntt, include/msmz.h):
//     forward:  out_k = sum_i x_i (g w^k)^i             inverse:  x_i = g^-i n^-1 sum_k X_k w^(-i k)
// mod q, natural order in and out, on the 8-word canonical records of a scalar set with the F_q functions of fr.h.
// ntt_plan.h splits a transform into passes and says where every entry lies between them; this file is one pass.
//
// Forms (the rule of section 19): data is canonical from load to store, every twiddle and every scaling factor is kept
// in Montgomery form, so a butterfly is one fr_mont_mul, one fr_add and one fr_sub and nothing is ever converted.
//
// One pass, one workgroup, one tile of C columns x R rows (R = 2^s, C R <= NTT_TILE):
//     load    entry (a, c) from m + (n / R) a, m = tile C + c (runs of C entries); the first pass reads zeros beyond n_in,
//             flags a record >= q, and multiplies by the coset factor g^i;
//     stages  decimation in frequency over a, in LDS, two stages at a time on the four entries a thread holds in
//             registers (one radix-2 step at the end when s is odd): s / 2 exchanges through LDS, row a' then holds
//             output digit k = bitrev(a');
//     store   entry (k, c) to (m mod T) + T k + T R (m div T), times the inter-pass twiddle w^(S' i' K') -- i' the next
//             pass's digit, K' = (m mod T) + T k, S' the stride of that digit -- or, in the last pass of an inverse
//             transform, times n^-1 (g^-k).
// No workgroup waits on another: the passes of a plan are separate launches and launch order is the only order.
//
// The first part of this file is host/device code: the LDS slot map, the index maps and the three per-thread bodies,
// over an abstract tile memory.  tests/native/ntt_test.cpp chains them on the CPU exactly as the kernel does.  The
// kernel follows, for the device compiler only.
#pragma once
#if defined(__HIPCC__)
#include "kernels.h"
#endif
#include "fr.h"
#include "ntt_plan.h"
#include "scalar_kernels.h"

namespace msmz {

// LDS: eight word planes (plane j holds word j of every entry), accessed 32 bits at a time, and NTT_LDS_PAD words of
// padding after every 32 entries.  A 32-bit access is served in groups of 32 lanes over 32 banks.  A radix-4 step with
// lower bit b makes a group touch runs of L = C 2^b consecutive entries that start 4 L apart: without padding the runs
// fall on the same banks once 4 L >= 32, up to 32 ways.  With 5 words after every 32 entries every access of every
// pass shape the planner makes -- load, each step, the bit-reversed read of the store -- is at worst 2-way (derived with
// tools/ntt_lds_model.py, not measured; DESIGN.md section 20 has the table).
constexpr int NTT_LDS_PAD = 5;
constexpr int NTT_LDS_WORDS = NTT_TILE + (NTT_TILE >> 5) * NTT_LDS_PAD;   // per plane: 1184 words, 37 KiB in all

MSMZ_HD uint32_t ntt_lds_slot(uint32_t pos) { return pos + (pos >> 5) * (uint32_t)NTT_LDS_PAD; }

// the low `bits` bits of x reversed (bits <= 32; 0 -> 0)
MSMZ_HD uint32_t ntt_bitrev(uint32_t x, uint32_t bits) {
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
  x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
  x = (x >> 16) | (x << 16);
  return bits ? x >> (32 - bits) : 0u;
}

// record i of a set -> s / s -> record i (16-byte aligned records: the device compiler makes two 128-bit accesses)
MSMZ_HD void ntt_rec_load(uint32_t* s, const uint32_t* set, uint64_t i) {
  const uint32_t* p = static_cast<const uint32_t*>(__builtin_assume_aligned(set + i * 8, 16));
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = p[j];
}
MSMZ_HD void ntt_rec_store(uint32_t* set, uint64_t i, const uint32_t* s) {
  uint32_t* p = static_cast<uint32_t*>(__builtin_assume_aligned(set + i * 8, 16));
#pragma unroll
  for (int j = 0; j < 8; j++) p[j] = s[j];
}

// Powers of one ratio on two levels: ratio^e = lo[e mod 2^h] (.) hi[e div 2^h], both tables in Montgomery form (lo may
// carry a constant factor): two loads, and two products to multiply a canonical value by the power.
struct NttPowers {
  const uint32_t* lo;
  const uint32_t* hi;
  uint32_t h;
};

template <class Fr>
MSMZ_HD void ntt_mul_power(uint32_t* x, const NttPowers& t, uint64_t e) {
  uint32_t w[8];
  ntt_rec_load(w, t.lo, e & ((1ull << t.h) - 1));
  fr_mont_mul<Fr>(x, x, w);
  ntt_rec_load(w, t.hi, e >> t.h);
  fr_mont_mul<Fr>(x, x, w);
}

enum { NTT_COSET_NONE = 0, NTT_COSET_LOAD = 1, NTT_COSET_STORE = 2 };

// what one launch receives
struct NttArgs {
  NttPass pass;
  const uint32_t* in;       // vector v of the batch starts at in + 8 v in_stride
  uint32_t* out;
  uint64_t in_stride, out_stride;
  uint64_t n_in;            // first pass: entries read per vector
  uint32_t count;           // vectors
  uint32_t tile_log;        // tile_tw[e] = (w^(n / 2^tile_log))^e, e < 2^(tile_log - 1)
  const uint32_t* tile_tw;
  NttPowers tw;             // powers of w (inter-pass twiddles)
  NttPowers coset;          // NTT_COSET_LOAD: powers of g; NTT_COSET_STORE: n^-1 times powers of g^-1
  uint32_t coset_at;
  uint32_t has_scale;       // last pass: multiply by `scale`, n^-1 in Montgomery form
  FrConst scale;
  uint32_t* err;            // bit 2: a record >= q
};

// ------------------------------------------------------------------------------------------------ per-thread bodies
// `Lds` is the tile memory: load(slot, x) / store(slot, x) of one 8-word entry.  `u` is the thread, of NTT_THREADS.

// load: returns true if a record it read is >= q
template <class Fr, class Lds>
MSMZ_HD bool ntt_thread_load(Lds& lds, const NttArgs& A, const uint32_t* in, uint32_t tile, uint32_t u) {
  const NttPass& P = A.pass;
  const uint32_t entries = 1u << (P.s + P.log_c);
  const uint64_t row = 1ull << (P.log_n - P.s);   // n / R
  bool bad = false;
  for (uint32_t o = u; o < entries; o += NTT_THREADS) {   // LDS position o = a C + c
    const uint32_t c = o & ((1u << P.log_c) - 1), a = o >> P.log_c;
    const uint64_t idx = (((uint64_t)tile << P.log_c) + c) + row * a;
    uint32_t x[8];
    if (!P.first || idx < A.n_in) {
      ntt_rec_load(x, in, idx);
      if (P.first) {
        bad |= words_geq<8>(x, Fr::Q);
        if (A.coset_at == NTT_COSET_LOAD) ntt_mul_power<Fr>(x, A.coset, idx);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) x[j] = 0;
    }
    lds.store(ntt_lds_slot(o), x);
  }
  return bad;
}

// (u, v) -> (u + v, (u - v) w)
template <class Fr>
MSMZ_HD void ntt_bfly(uint32_t* u, uint32_t* v, const uint32_t* w) {
  uint32_t d[8];
  fr_sub<Fr>(d, u, v);
  fr_add<Fr>(u, u, v);
  fr_mont_mul<Fr>(v, d, w);
}

// stages b + 1 and b of the transform over the rows (b = rem - 2 with `rem` stages still to go), radix4; or the
// stage b = 0 alone, whose twiddle is 1
template <class Fr, class Lds>
MSMZ_HD void ntt_thread_step(Lds& lds, const NttArgs& A, uint32_t b, bool radix4, uint32_t u) {
  const NttPass& P = A.pass;
  const uint32_t entries = 1u << (P.s + P.log_c);
  const uint32_t cmask = (1u << P.log_c) - 1;
  if (!radix4) {
    for (uint32_t bu = u; bu < entries / 2; bu += NTT_THREADS) {
      const uint32_t c = bu & cmask, a0 = (bu >> P.log_c) << 1;
      const uint32_t p0 = ntt_lds_slot((a0 << P.log_c) + c), p1 = ntt_lds_slot(((a0 + 1) << P.log_c) + c);
      uint32_t x0[8], x1[8], d[8];
      lds.load(p0, x0);
      lds.load(p1, x1);
      fr_sub<Fr>(d, x0, x1);
      fr_add<Fr>(x0, x0, x1);
      lds.store(p0, x0);
      lds.store(p1, d);
    }
    return;
  }
  const uint32_t sh = A.tile_log - b - 2;
  for (uint32_t bu = u; bu < entries / 4; bu += NTT_THREADS) {
    const uint32_t c = bu & cmask, q = bu >> P.log_c;
    const uint32_t lo = q & ((1u << b) - 1), a0 = ((q >> b) << (b + 2)) | lo;
    const uint32_t p0 = ntt_lds_slot((a0 << P.log_c) + c), p1 = ntt_lds_slot(((a0 + (1u << b)) << P.log_c) + c);
    const uint32_t p2 = ntt_lds_slot(((a0 + (2u << b)) << P.log_c) + c), p3 = ntt_lds_slot(((a0 + (3u << b)) << P.log_c) + c);
    uint32_t x0[8], x1[8], x2[8], x3[8], w[8];
    lds.load(p0, x0);
    lds.load(p1, x1);
    lds.load(p2, x2);
    lds.load(p3, x3);
    ntt_rec_load(w, A.tile_tw, (uint64_t)lo << sh);                 // stage b + 1: rows a and a + 2^(b+1)
    ntt_bfly<Fr>(x0, x2, w);
    ntt_rec_load(w, A.tile_tw, (uint64_t)(lo + (1u << b)) << sh);
    ntt_bfly<Fr>(x1, x3, w);
    ntt_rec_load(w, A.tile_tw, (uint64_t)lo << (sh + 1));           // stage b: rows a and a + 2^b
    ntt_bfly<Fr>(x0, x1, w);
    ntt_bfly<Fr>(x2, x3, w);
    lds.store(p0, x0);
    lds.store(p1, x1);
    lds.store(p2, x2);
    lds.store(p3, x3);
  }
}

// where entry (k, c) of a tile goes, and the exponent of its inter-pass twiddle
MSMZ_HD uint64_t ntt_out_index(const NttPass& P, uint32_t tile, uint32_t c, uint32_t k, uint64_t* twiddle) {
  const uint64_t m = ((uint64_t)tile << P.log_c) + c;
  const uint64_t klow = m & ((1ull << P.log_t) - 1), r = m >> P.log_t;
  const uint64_t knext = klow + ((uint64_t)k << P.log_t);
  if (!P.last) {
    const uint32_t log_s = P.log_n - P.log_t - P.s - P.s_next;   // the stride of the next pass's digit
    *twiddle = ((r >> log_s) * knext) << log_s;
  }
  return knext + (r << (P.log_t + P.s));
}

template <class Fr, class Lds>
MSMZ_HD void ntt_thread_store(Lds& lds, const NttArgs& A, uint32_t* out, uint32_t tile, uint32_t u) {
  const NttPass& P = A.pass;
  const uint32_t entries = 1u << (P.s + P.log_c);
  for (uint32_t o = u; o < entries; o += NTT_THREADS) {
    // neighbours in memory to neighbouring threads: k runs fastest in the first pass (T = 1), c in a later one
    const uint32_t k = P.log_t == 0 ? o & ((1u << P.s) - 1) : o >> P.log_c;
    const uint32_t c = P.log_t == 0 ? o >> P.s : o & ((1u << P.log_c) - 1);
    uint32_t x[8];
    lds.load(ntt_lds_slot((ntt_bitrev(k, P.s) << P.log_c) + c), x);
    uint64_t e = 0;
    const uint64_t idx = ntt_out_index(P, tile, c, k, &e);
    if (!P.last) ntt_mul_power<Fr>(x, A.tw, e);
    else if (A.coset_at == NTT_COSET_STORE) ntt_mul_power<Fr>(x, A.coset, idx);
    else if (A.has_scale) fr_mont_mul<Fr>(x, x, A.scale.w);
    ntt_rec_store(out, idx, x);
  }
}

// ------------------------------------------------------------------------------------------------ roots of unity (host)
// out = the default primitive 2^log_n-th root of unity, ROOT_MAX^(2^(TWO_ADICITY - log_n)); log_n <= TWO_ADICITY
template <class Fr>
inline void fr_root_of_unity(uint32_t* out, uint32_t log_n) {
  for (int j = 0; j < 8; j++) out[j] = Fr::ROOT_MAX[j];
  for (uint32_t k = log_n; k < (uint32_t)Fr::TWO_ADICITY; k++) fr_mul<Fr>(out, out, out);
}

// is w (canonical) a primitive 2^log_n-th root of unity: w^(n / 2) == q - 1, or w == 1 for n = 1
template <class Fr>
inline bool fr_is_primitive_root(const uint32_t* w, uint32_t log_n) {
  uint32_t t[8], want[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < 8; j++) t[j] = w[j];
  for (uint32_t k = 1; k < log_n; k++) fr_mul<Fr>(t, t, t);
  if (log_n) words_sub<8>(want, Fr::Q, want);
  for (int j = 0; j < 8; j++)
    if (t[j] != want[j]) return false;
  return true;
}

// ------------------------------------------------------------------------------------------------ tables and launches (host)
// A table of powers: entry i = base ratio^i, i < count.  `ratio` canonical, `base` as it is to be stored: with the
// Montgomery form of 1 (or of a constant) as base every entry is in Montgomery form.  k_scalars_powers builds it on the
// device (ResidentSets::scalars_ntt), fr_pow_run on the host (tests/native/ntt_test.cpp).
struct NttTableSpec {
  uint32_t ratio[8];
  uint32_t base[8];
  uint64_t count;
};

// r = w^(2^k), canonical
template <class Fr>
inline void fr_pow2k(uint32_t* r, const uint32_t* w, uint32_t k) {
  for (int j = 0; j < 8; j++) r[j] = w[j];
  for (uint32_t i = 0; i < k; i++) fr_mul<Fr>(r, r, r);
}

// entries of the three twiddle tables of a plan, which lie one behind the other: in-tile, low, high
static inline uint64_t ntt_tile_table_count(const NttPlan& p) { return p.tile_log ? 1ull << (p.tile_log - 1) : 1; }
static inline uint64_t ntt_low_count(const NttPlan& p) { return 1ull << p.split; }
static inline uint64_t ntt_high_count(const NttPlan& p) { return 1ull << (p.log_n - p.split); }
static inline uint64_t ntt_twiddle_entries(const NttPlan& p) {
  return ntt_tile_table_count(p) + ntt_low_count(p) + ntt_high_count(p);
}

// the two levels of the powers of `ratio` below n; the low table starts from `base`, the high one from 1
template <class Fr>
inline void ntt_two_level_specs(const NttPlan& p, const uint32_t* ratio, const uint32_t* base, NttTableSpec* lo,
                                NttTableSpec* hi) {
  for (int j = 0; j < 8; j++) lo->ratio[j] = ratio[j], lo->base[j] = base[j], hi->base[j] = Fr::ONE[j];
  lo->count = ntt_low_count(p);
  fr_pow2k<Fr>(hi->ratio, ratio, p.split);
  hi->count = ntt_high_count(p);
}

// the twiddle tables of a plan for the root w (the inverse root for an inverse transform): spec[0] in-tile, [1] low, [2] high
template <class Fr>
inline void ntt_twiddle_specs(const NttPlan& p, const uint32_t* w, NttTableSpec spec[3]) {
  fr_pow2k<Fr>(spec[0].ratio, w, p.log_n - p.tile_log);
  for (int j = 0; j < 8; j++) spec[0].base[j] = Fr::ONE[j];
  spec[0].count = ntt_tile_table_count(p);
  ntt_two_level_specs<Fr>(p, w, Fr::ONE, &spec[1], &spec[2]);
}

// What does not depend on the pass: the tables (`twiddles`: the three tables of ntt_twiddle_specs; `coset`: the two of
// ntt_two_level_specs for g, or for g^-1 from the base n^-1, or null), the direction, the batch.
struct NttCall {
  NttPlan plan;
  const uint32_t* twiddles;
  const uint32_t* coset;
  bool inverse;
  uint64_t n_in;
  uint32_t count;
  FrConst ninv;   // n^-1 in Montgomery form
  uint32_t* err;
};

// the arguments of pass j, from `in` (vectors in_stride entries apart) to `out` (vectors n apart)
static inline NttArgs ntt_pass_args(const NttCall& c, uint32_t j, const uint32_t* in, uint64_t in_stride, uint32_t* out) {
  const NttPlan& p = c.plan;
  NttArgs a{};
  a.pass = p.pass[j];
  a.in = in;
  a.out = out;
  a.in_stride = in_stride;
  a.out_stride = 1ull << p.log_n;
  a.n_in = c.n_in;
  a.count = c.count;
  a.tile_log = p.tile_log;
  a.tile_tw = c.twiddles;
  a.tw.lo = c.twiddles + ntt_tile_table_count(p) * 8;
  a.tw.hi = a.tw.lo + ntt_low_count(p) * 8;
  a.tw.h = p.split;
  a.coset_at = NTT_COSET_NONE;
  if (c.coset) {
    a.coset.lo = c.coset;
    a.coset.hi = c.coset + ntt_low_count(p) * 8;
    a.coset.h = p.split;
    if (!c.inverse && a.pass.first) a.coset_at = NTT_COSET_LOAD;
    if (c.inverse && a.pass.last) a.coset_at = NTT_COSET_STORE;
  }
  a.has_scale = c.inverse && a.pass.last && !c.coset;
  a.scale = c.ninv;
  a.err = c.err;
  return a;
}

}  // namespace msmz

#if defined(__HIPCC__)
namespace msmz {

// the tile in LDS: plane j holds word j of every entry
struct NttLds {
  uint32_t (*w)[NTT_LDS_WORDS];
  __device__ __forceinline__ void load(uint32_t slot, uint32_t* x) const {
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = w[j][slot];
  }
  __device__ __forceinline__ void store(uint32_t slot, const uint32_t* x) const {
#pragma unroll
    for (int j = 0; j < 8; j++) w[j][slot] = x[j];
  }
};

// One pass of a plan.  grid.x: the tiles of one vector; grid.y: vectors, a workgroup taking vector blockIdx.y and every
// gridDim.y-th after it.  A tile is loaded whole before any of it is stored, so a one-pass transform may run in place;
// a plan of several passes goes through scratch (ResidentSets::scalars_ntt).
template <class Fr>
__global__ void __launch_bounds__(NTT_THREADS) k_ntt_pass(NttArgs A) {
  __shared__ uint32_t planes[8][NTT_LDS_WORDS];
  NttLds lds{planes};
  const uint32_t u = threadIdx.x, tile = blockIdx.x;
  bool bad = false;
#pragma unroll 1
  for (uint32_t v = blockIdx.y; v < A.count; v += gridDim.y) {
    bad |= ntt_thread_load<Fr>(lds, A, A.in + (uint64_t)v * A.in_stride * 8, tile, u);
    __syncthreads();
    uint32_t rem = A.pass.s;
#pragma unroll 1
    for (; rem >= 2; rem -= 2) {
      ntt_thread_step<Fr>(lds, A, rem - 2, true, u);
      __syncthreads();
    }
    if (rem) {
      ntt_thread_step<Fr>(lds, A, 0, false, u);
      __syncthreads();
    }
    ntt_thread_store<Fr>(lds, A, A.out + (uint64_t)v * A.out_stride * 8, tile, u);
    __syncthreads();   // (the next vector's load overwrites the tile)
  }
  if (bad) atomicOr(A.err, 4u);
}

}  // namespace msmz
#endif

// The plan of a number-theoretic transform over a resident scalar set (msmz_scalars_ntt, include/msmz.h; DESIGN.md
// section 20): log_n -> the train of passes, each with its stages, its column width and its strides.  Host only, no
// HIP: tests/native/ntt_test.cpp compiles it for the CPU.  This is the single place that decides the split; the engine
// (NttOps::scalars_ntt, ntt_ops.h) launches one kernel per pass of the plan and ntt_kernels.h reads nothing but an NttPass.
//
// The split.  n = R_1 R_2 ... R_P with R_j = 2^(s_j).  Write an input index i = sum_j i_j S_j with S_j = R_(j+1) .. R_P
// (i_1 is the most significant digit) and an output index k = sum_j k_j T_j with T_j = R_1 .. R_(j-1) (k_1 is the least
// significant).  Then w^(i k) = prod_j [ w^(S_j T_j i_j k_j) * w^(S_j i_j K_j) ] with K_j = sum_(m<j) k_m T_m, because
// S_j T_m is a multiple of n for m > j.  The first factor is the R_j-point transform of pass j over the digit i_j (root
// w^(n / R_j)); the second is the inter-pass twiddle, applied when pass j - 1 stores.  Between the passes the vector
// lies at
//     position after pass j = K_(j+1) + T_(j+1) r_j,      r_j = sum_(m>j) i_m S_m  (the digits still to go),
// which is the natural input order for j = 0 and the natural output order for j = P.  With m = K_j + T_j r_j (one
// value per column, m < n / R_j) pass j
//     reads   m + (n / R_j) a                              a = i_j < R_j,
//     writes  (m mod T_j) + T_j k + T_(j+1) (m div T_j)     k = k_j < R_j:
// columns that are neighbours in m are neighbours in memory on both sides, and the first pass (T_1 = 1) writes whole
// runs of R_1 entries.  A workgroup takes C = 2^log_c neighbouring columns, so every run in global memory is C entries
// long: NTT_RUN_LOG sets the least, 4 entries = 128 bytes.  A one-pass plan has one column per vector and is contiguous.
#pragma once
#include <cstdint>

namespace msmz {

constexpr int NTT_PASS_LOG = 10;                  // a tile: 2^10 entries = 32 KiB in LDS, 256 threads x 4 entries
constexpr int NTT_TILE = 1 << NTT_PASS_LOG;
constexpr int NTT_THREADS = NTT_TILE / 4;
constexpr int NTT_RUN_LOG = 2;                    // a strided pass moves runs of at least 2^2 entries = 128 bytes
constexpr int NTT_STRIDED_LOG = NTT_PASS_LOG - NTT_RUN_LOG;   // ... and therefore covers at most 8 stages
constexpr int NTT_MAX_LOG = 32;                   // indices of a set fit 32 bits
constexpr int NTT_MAX_PASSES = (NTT_MAX_LOG + NTT_STRIDED_LOG - 1) / NTT_STRIDED_LOG;   // 4
constexpr uint32_t NTT_GRID_VECTORS = 65535;     // grid.y of a pass at the most: a workgroup takes every NTT_GRID_VECTORS-th vector
constexpr uint32_t NTT_CACHE = 8;                // twiddle sets an engine keeps (NttOps::ntt_twiddles, ntt_ops.h)

// One pass, as the kernel receives it (by value).  n / R_j columns, tiles of C = 2^log_c of them.
struct NttPass {
  uint32_t log_n;
  uint32_t s;        // stages: R_j = 2^s
  uint32_t log_c;    // columns per tile
  uint32_t log_t;    // T_j = 2^log_t: the transform sizes of the passes before this one
  uint32_t s_next;   // stages of the next pass (the inter-pass twiddle needs its digit); 0 in the last pass
  uint32_t first;    // 1: reads the caller's vector (n_in entries, range check, forward coset factors)
  uint32_t last;     // 1: writes the result (inverse scaling), no inter-pass twiddle
};

struct NttPlan {
  uint32_t log_n = 0;
  uint32_t n_passes = 0;
  NttPass pass[NTT_MAX_PASSES] = {};
  uint32_t tile_log = 0;   // the in-tile twiddle table holds 2^(tile_log - 1) powers of w^(n / 2^tile_log); tile_log = max s
  uint32_t split = 0;      // two-level tables: e = e_hi 2^split + e_lo; 2^split low and 2^(log_n - split) high entries
};

static inline uint32_t ntt_pass_count(uint32_t log_n) {
  return log_n <= (uint32_t)NTT_PASS_LOG ? 1u : (log_n + NTT_STRIDED_LOG - 1) / NTT_STRIDED_LOG;
}

// log_n <= NTT_MAX_LOG.  The fewest passes; their stages as even as they go, the larger ones first.
static inline NttPlan ntt_plan(uint32_t log_n) {
  NttPlan p;
  p.log_n = log_n;
  p.n_passes = ntt_pass_count(log_n);
  p.split = (log_n + 1) / 2;
  uint32_t done = 0;
  for (uint32_t j = 0; j < p.n_passes; j++) {
    NttPass& ps = p.pass[j];
    ps.log_n = log_n;
    ps.s = log_n / p.n_passes + (j < log_n % p.n_passes ? 1u : 0u);
    ps.log_t = done;
    ps.first = j == 0;
    ps.last = j + 1 == p.n_passes;
    // as many columns as fill the tile, of those that are neighbours in memory on both sides: all n / R_1 columns of
    // the first pass, the T_j low ones of a later pass
    const uint32_t room = NTT_PASS_LOG - ps.s;
    const uint32_t have = j == 0 ? log_n - ps.s : done;
    ps.log_c = room < have ? room : have;
    if (ps.s > p.tile_log) p.tile_log = ps.s;
    done += ps.s;
  }
  for (uint32_t j = 0; j + 1 < p.n_passes; j++) p.pass[j].s_next = p.pass[j + 1].s;
  return p;
}

// tiles of one vector in a pass
static inline uint32_t ntt_pass_tiles(const NttPass& ps) { return 1u << (ps.log_n - ps.s - ps.log_c); }

}  // namespace msmz

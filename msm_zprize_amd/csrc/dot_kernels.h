// Batched inner products of resident scalar sets (msmz_scalars_dot_many, include/msmz.h): the
// product of a dense n_rows x n matrix with a dense n x n_cols matrix mod q, n large, n_rows and n_cols small,
//     result[r n_cols + c] = sum_(i < n) rows[r][i] cols[c][i]
// each value byte for byte what msmz_scalars_dot returns for that pair.  Every thread keeps a block of RG x NC sums in
// registers: per element index it loads the NC column values once and then the RG row values of its row group, so a
// column value is fetched once per RG rows and a row value once.  The first part of this file is host/device code: the
// limits, the block per column count, the planner and the body of one element index, which
// tests/native/dot_many_test.cpp runs on the CPU.  The kernel follows, for the device compiler only; the second level is
// k_scalars_dot_fold (scalar_kernels.h), one workgroup per result.
#pragma once
#include "scalar_kernels.h"
#include "sqrt.h"   // static_for

namespace msmz {

constexpr int DOT_MANY_MAX_ROWS = 128;
constexpr int DOT_MANY_MAX_COLS = 8;
// workgroups along n (grid x) a call launches at the most: each strides over the tiles of SDOT_TILE element indices.
// msmz_test_set_dot_many_groups lowers it for a context.
constexpr uint32_t DOT_MANY_GROUPS = 2048;
// the record of a call: 64 bytes (word 8: the error word), then the results, then the partial sums -- at most this much
constexpr uint64_t DOT_MANY_SCRATCH_MAX = 16ull << 20;
constexpr uint32_t DOT_MANY_HEAD_BYTES = 64;

// Rows per register block for a column count, chosen off the register counts of the blocks compiled (DESIGN.md section
// 32 has the table): 4 rows for one column (114 VGPRs, four waves per SIMD; 8 rows would save a ninth of the bytes for
// a wave), 2 rows for two and three columns (138 and 182), one row from four columns on (150 to 256 and some AGPRs).
// No instance has scratch.  None of the alternatives has been timed.
constexpr int dot_many_rg(int nc) { return nc == 1 ? 4 : nc <= 3 ? 2 : 1; }

// the first record of every vector, resolved on the host: a kernel argument of 1088 bytes (uniform reads)
struct DotManyVecs {
  const uint32_t* row[DOT_MANY_MAX_ROWS];
  const uint32_t* col[DOT_MANY_MAX_COLS];
};
static_assert(sizeof(DotManyVecs) == 8 * (DOT_MANY_MAX_ROWS + DOT_MANY_MAX_COLS), "two tables of pointers");
static_assert(sizeof(DotManyVecs) + 64 <= 4096, "the pointer tables and the other arguments fit one kernel argument segment");

// What a call launches.  Grid x = groups workgroups, workgroup g takes tiles g, g + groups, ..; grid y = row_groups,
// row group y takes rows [y rg, (y + 1) rg) below n_rows (the last group may hold fewer: predicated).  Partial sum
// (result, g) is record result * groups + g behind the results; k_scalars_dot_fold folds `groups` of them per result.
struct DotManyPlan {
  uint32_t nc, rg;              // the kernel instance: columns (= n_cols) and rows of a thread's register block
  uint32_t tiles;               // ceil(n / SDOT_TILE)
  uint32_t groups, row_groups;  // the grid
  uint32_t results;             // n_rows * n_cols
  uint64_t scratch_bytes;       // head + results + partial sums, <= DOT_MANY_SCRATCH_MAX
};

// n: 1 .. 2^32 - 1, n_rows: 1 .. DOT_MANY_MAX_ROWS, n_cols: 1 .. DOT_MANY_MAX_COLS (the caller has checked);
// max_groups: 1 .. DOT_MANY_GROUPS.  groups is bounded by the tiles there are, by max_groups and by the scratch cap
// (1024 results leave room for 510 groups, one result for more than DOT_MANY_GROUPS).
inline DotManyPlan dot_many_plan(uint64_t n, uint32_t n_rows, uint32_t n_cols, uint32_t max_groups = DOT_MANY_GROUPS) {
  DotManyPlan p{};
  p.nc = n_cols;
  p.rg = (uint32_t)dot_many_rg((int)n_cols);
  p.tiles = (uint32_t)((n + SDOT_TILE - 1) / SDOT_TILE);
  p.results = n_rows * n_cols;
  p.row_groups = (n_rows + p.rg - 1) / p.rg;
  const uint64_t room = (DOT_MANY_SCRATCH_MAX - DOT_MANY_HEAD_BYTES) / (32ull * p.results) - 1;   // records per result, less its own
  uint64_t g = p.tiles;
  if (g > max_groups) g = max_groups;
  if (g > room) g = room;
  p.groups = (uint32_t)g;
  p.scratch_bytes = DOT_MANY_HEAD_BYTES + 32ull * p.results * (1 + (uint64_t)p.groups);
  return p;
}

// The body of one element index for one thread: acc[j][c] += row_j col_c 2^-256 for the first `live` rows of the block
// (1 .. RG; fewer than RG in the last row group of a row count that is no multiple of RG: the row tail is predicated,
// a surplus row is neither loaded nor multiplied) and the NC columns.  load_col(C, dst) brings the column value,
// load_row(J, dst) the row value (C, J integral constants); both return whether the record was >= q.  The column values
// are loaded first and stay in registers while the rows go by one at a time.  Returns whether any record was >= q; the
// sums are then not below q and the caller discards them.
template <class Fr, int NC, int RG, class LoadCol, class LoadRow>
MSMZ_HD bool fr_dot_many_index(uint32_t (&acc)[RG][NC][8], uint32_t live, LoadCol load_col, LoadRow load_row) {
  uint32_t col[NC][8];
  bool bad = false;
  static_for<0, NC>([&](auto C) { bad |= load_col(C, col[C]); });
  static_for<0, RG>([&](auto J) {
    if ((uint32_t)decltype(J)::value < live) {   // (uniform over the workgroup)
      uint32_t row[8];
      bad |= load_row(J, row);
      if (!bad) {   // (a flagged record is not below q: it stays out of the sums, as in k_scalars_dot)
        static_for<0, NC>([&](auto C) {
          uint32_t p[8];
          fr_mont_mul<Fr>(p, row, col[C]);
          fr_add<Fr>(acc[J][C], acc[J][C], p);
        });
      }
    }
  });
  return bad;
}

}  // namespace msmz

#if defined(__HIPCC__)
namespace msmz {

// partial[(row NC + c) gridDim.x + blockIdx.x] = sum over the workgroup's tiles of rows[row][i] cols[c][i] 2^-256, for
// the rows of row group blockIdx.y.  Thread t takes elements tile SDOT_TILE + e SDOT_THREADS + t of every tile of its
// workgroup, as k_scalars_dot does: a wave reads 2 KiB of one vector in a row.  Vectors may overlap and be the same;
// nothing is written but the partial sums.  A record >= q raises bit 2 of *err.  n < 2^32, so tiles <= 2^21.
template <class Fr, int NC, int RG = dot_many_rg(NC)>
__global__ void __launch_bounds__(SDOT_THREADS) k_scalars_dot_many(uint32_t* partial, DotManyVecs V, uint32_t n_rows,
                                                                   uint32_t n, uint32_t tiles, uint32_t* err) {
  const uint32_t row0 = blockIdx.y * RG;
  const uint32_t live = n_rows - row0 < (uint32_t)RG ? n_rows - row0 : (uint32_t)RG;   // (row0 < n_rows: the grid's y)
  uint32_t acc[RG][NC][8];
  static_for<0, RG>([&](auto J) {
    static_for<0, NC>([&](auto C) {
#pragma unroll
      for (int w = 0; w < 8; w++) acc[J][C][w] = 0;
    });
  });
  bool bad = false;
#pragma unroll 1
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t base = (uint64_t)tile * SDOT_TILE + threadIdx.x;
#pragma unroll 1
    for (int e = 0; e < SDOT_E; e++) {
      const uint64_t i = base + (uint64_t)e * SDOT_THREADS;
      if (i < n) {
        bad |= fr_dot_many_index<Fr, NC, RG>(
            acc, live, [&](auto C, uint32_t* dst) { return fr_load<Fr>(dst, V.col[C], i); },
            [&](auto J, uint32_t* dst) { return fr_load<Fr>(dst, V.row[row0 + J], i); });
      }
    }
  }
  if (bad) atomicOr(err, 4u);
  static_for<0, RG>([&](auto J) {
    if ((uint32_t)decltype(J)::value < live) {   // (uniform: every thread of the workgroup reaches the same block sums)
      static_for<0, NC>([&](auto C) {
        fr_block_sum<Fr>(acc[J][C]);
        if (threadIdx.x == 0) fr_store(partial, ((uint64_t)(row0 + J) * NC + C) * gridDim.x + blockIdx.x, acc[J][C]);
        __syncthreads();   // (fr_block_sum's LDS words are free for the next sum)
      });
    }
  });
}

}  // namespace msmz
#endif

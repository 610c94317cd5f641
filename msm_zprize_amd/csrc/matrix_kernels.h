// Sparse matrices over resident scalar sets (msmz_matrix_create / _matrix_mul, include/msmz.h):
//     out_i = sum over the non-zeros k with row[k] = i of val[k] x[col[k]]   mod q
// and the same with the roles of row and col swapped (the transposed product).  A matrix is kept in up to two sorted
// FORMS, one per orientation.  A form lists the non-zeros sorted by their output index and holds, per non-zero in
// that order,
//     seg   the output index (the "segment": all non-zeros of one output entry lie next to each other),
//     gidx  the index of the entry of x it reads (the gathered index),
//     val   the value as v 2^256 mod q, so that val (.) x is ONE Montgomery product with a canonical result
//           (absent: every value is 1 and x is added as it is).
// The product is a segmented sum of nnz terms whose segment lengths the caller chose, so the work is split over
// non-zeros, never over rows: a workgroup takes a tile of MAT_TILE consecutive non-zeros, a thread a run of MAT_RUN of
// them, whatever rows they belong to.  No atomics on the sums; addition mod q is exact, so the bytes do not depend on
// the grouping.
//
// The first part of this file is host/device code: the geometry, the host sort that builds a form, the walk of one
// thread's run, the combination of two neighbouring partial sums and what a thread and the carry fold do with the
// outcome.  tests/native/matrix_test.cpp runs whole tiles of it on the CPU.  The kernels follow, for the device
// compiler only.
#pragma once
#include <cstddef>
#include <vector>

#include "scalar_kernels.h"

namespace msmz {

constexpr int MAT_THREADS = 256;
constexpr int MAT_RUN = 8;                          // consecutive non-zeros one thread walks
constexpr int MAT_TILE = MAT_THREADS * MAT_RUN;     // consecutive non-zeros of one workgroup
constexpr int MAT_FOLD_PASS = MAT_THREADS;          // tile carries ONE workgroup folds per pass of its loop
constexpr int MAT_CARRY_WORDS = 16;                 // a tile carry: word 0 = the segment, words 8..15 = the partial sum

// ------------------------------------------------------------------------------------------------ host: the forms
// The stable counting sort of nnz triples by `key` (each < n_keys): position p of the sorted order holds triple
// perm[p], seg[p] = key[perm[p]], gidx[p] = other[perm[p]].  Triples of one key keep the caller's order, duplicates
// stay separate entries (they add up in the product).  O(nnz + n_keys) time, 8 n_keys bytes of scratch.
inline void mat_sort_form(const uint32_t* key, const uint32_t* other, uint64_t nnz, uint32_t n_keys, uint32_t* seg,
                          uint32_t* gidx, uint32_t* perm) {
  std::vector<uint64_t> start((size_t)n_keys + 1, 0);
  for (uint64_t k = 0; k < nnz; k++) start[(size_t)key[k] + 1]++;
  for (size_t i = 0; i < n_keys; i++) start[i + 1] += start[i];
  for (uint64_t k = 0; k < nnz; k++) {
    const uint64_t p = start[key[k]]++;
    perm[p] = (uint32_t)k;
    seg[p] = key[k];
    gidx[p] = other[k];
  }
}

// a form's buffer: nnz segment indices, nnz gathered indices, then (with values) nnz records of 8 words from this byte
// offset, which is a multiple of 32
inline size_t mat_val_offset(uint64_t nnz) { return (size_t)((2 * nnz * 4 + 31) / 32 * 32); }

// the first k with row[k] >= n_rows or col[k] >= n_cols (the row is looked at before the column of the same triple),
// or nnz if every index is in range
inline uint64_t mat_first_bad_index(const uint32_t* row, const uint32_t* col, uint64_t nnz, uint32_t n_rows,
                                    uint32_t n_cols) {
  for (uint64_t k = 0; k < nnz; k++)
    if (row[k] >= n_rows || col[k] >= n_cols) return k;
  return nnz;
}

// ------------------------------------------------------------------------------------------------ host/device: a tile
// one form as the kernels read it; val == nullptr: every value is 1
struct MatView {
  const uint32_t* gidx;
  const uint32_t* seg;
  const uint32_t* val;
};

// A partial sum of a segmented scan: `reset` says that it starts at a segment's first term inside the tile (or at the
// tile's first term), so nothing to its left belongs to it.
struct MatPart {
  uint32_t reset;
  uint32_t v[8];
};

// What the walk of one run leaves.  The run's first segment is the head, its last one -- the same one if the run never
// changes segment -- the tail; every segment between them begins and ends inside the run and was stored by the walk.
enum { MAT_HAS_TAIL = 1, MAT_OPEN_LEFT = 2, MAT_OPEN_RIGHT = 4, MAT_BAD = 8, MAT_ENDS_TILE = 16 };
struct MatRun {
  uint32_t hkey, lkey;   // the segments of head and tail
  uint32_t flags;        // HAS_TAIL: head and tail differ; OPEN_LEFT: the term before the run, in this tile, belongs to
                         // the head; OPEN_RIGHT: the term after it, in this tile, belongs to the tail; BAD: an entry of x
                         // it read is >= q; ENDS_TILE: the run's last term is the tile's
  uint32_t head[8], last[8];   // their sums over the run (last == head without HAS_TAIL)
};

MSMZ_HD void mat_store(uint32_t* out, uint32_t i, const uint32_t* s) {
  uint32_t* o = static_cast<uint32_t*>(__builtin_assume_aligned(out + (size_t)i * 8, 16));
#pragma unroll
  for (int j = 0; j < 8; j++) o[j] = s[j];
}

MSMZ_HD void mat_load(uint32_t* s, const uint32_t* set, uint64_t i) {
  const uint32_t* p = static_cast<const uint32_t*>(__builtin_assume_aligned(set + (size_t)i * 8, 16));
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = p[j];
}

// The walk of non-zeros [first, first + count), 1 <= count <= MAT_RUN, of the tile [tile_first, tile_end): one entry of
// x gathered, one product (none without values) and one addition per non-zero.  A segment that begins and ends strictly
// inside the run is stored to `out` here.  One look at the segment index on either side of the run, where that lies in
// the tile, tells whether head and tail go on there.
//
// The loop is a pipeline of two stages, because a gather is two dependent loads (the index, then the entry of x) and a
// product is long enough to hide both: the indices of non-zero e + 2 and the operands of non-zero e + 1 are requested
// before the product of non-zero e starts.  It stays rolled -- eight copies of the product would not fit the
// instruction cache -- so what is in flight lives in named registers, not in an array indexed by e.
template <class Fr>
MSMZ_HD void mat_run(MatRun& r, uint32_t* out, const MatView& m, const uint32_t* x, uint64_t first, uint32_t count,
                     uint64_t tile_first, uint64_t tile_end) {
  uint32_t acc[8], head[8];   // (head is selected into, never written through a pointer: the arrays stay in registers)
  uint32_t t1[8], v1[8];      // the operands of the next non-zero
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0, head[j] = 0, v1[j] = 0;
  const uint64_t end = first + count;
  uint32_t k1 = m.seg[first];
  uint32_t k2 = count > 1 ? m.seg[first + 1] : 0u, g2 = count > 1 ? m.gidx[first + 1] : 0u;
  mat_load(t1, x, m.gidx[first]);
  if (m.val) mat_load(v1, m.val, first);
  const bool open_left = first > tile_first && m.seg[first - 1] == k1;
  const uint32_t after = end < tile_end ? m.seg[end] : 0u;
  uint32_t key = k1;
  bool in_head = true, bad = false;
  r.hkey = key;
#pragma unroll 1
  for (uint32_t e = 0; e < count; e++) {
    const uint64_t i = first + e;
    const uint32_t k = k1;
    uint32_t t[8], v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) t[j] = t1[j], v[j] = v1[j];
    k1 = k2;
    if (e + 1 < count) {
      mat_load(t1, x, g2);
      if (m.val) mat_load(v1, m.val, i + 1);
    }
    if (e + 2 < count) k2 = m.seg[i + 2], g2 = m.gidx[i + 2];
    if (k != key) {
      if (!in_head) mat_store(out, key, acc);
#pragma unroll
      for (int j = 0; j < 8; j++) head[j] = in_head ? acc[j] : head[j], acc[j] = 0;
      in_head = false;
      key = k;
    }
    const bool geq = words_geq<8>(t, Fr::Q);
    bad |= geq;
    if (m.val) fr_mont_mul<Fr>(t, v, t);   // (v < q: the product is below q whatever t is)
    if (!geq) fr_add<Fr>(acc, acc, t);     // (a flagged entry stays out of the sum, as in k_scalars_dot)
  }
  r.lkey = key;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    r.last[j] = acc[j];
    r.head[j] = in_head ? acc[j] : head[j];
  }
  r.flags = (in_head ? 0u : (uint32_t)MAT_HAS_TAIL) | (bad ? (uint32_t)MAT_BAD : 0u) | (open_left ? (uint32_t)MAT_OPEN_LEFT : 0u) |
            (end < tile_end ? (after == key ? (uint32_t)MAT_OPEN_RIGHT : 0u) : (uint32_t)MAT_ENDS_TILE);
}

// the run's element of the tile's segmented scan: the sum it hands to its right neighbour
MSMZ_HD void mat_run_part(MatPart& a, const MatRun& r) {
  a.reset = (r.flags & MAT_HAS_TAIL) || !(r.flags & MAT_OPEN_LEFT) ? 1u : 0u;
#pragma unroll
  for (int j = 0; j < 8; j++) a.v[j] = r.last[j];
}

MSMZ_HD void mat_part_identity(MatPart& a) {
  a.reset = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) a.v[j] = 0;
}

// r = l followed by r: l's sum joins r's unless r starts a segment of its own.  The operator of the segmented scan; it
// is associative, and the identity (mat_part_identity) may stand on either side.
template <class Fr>
MSMZ_HD void mat_combine(MatPart& r, const MatPart& l) {
  uint32_t s[8];
  fr_add<Fr>(s, r.v, l.v);
#pragma unroll
  for (int j = 0; j < 8; j++) r.v[j] = r.reset ? r.v[j] : s[j];
  r.reset |= l.reset;
}

// What a thread does once it knows `excl`, the combination of every run of the tile before its own: the head, with
// what came from the left, is stored if it ends in this run; the tail is stored if it ends here too, stays with the
// scan if it goes on, and becomes the tile's carry -- closed or not -- if the run is the tile's last.  So a tile stores
// every segment that ends inside it except its last one, the first one possibly as a partial sum, and leaves ONE carry.
template <class Fr>
MSMZ_HD void mat_finish(uint32_t* out, uint32_t* carry, const MatRun& r, const MatPart& excl) {
  uint32_t total[8];
  fr_add<Fr>(total, r.head, excl.v);
  const bool left = (r.flags & MAT_OPEN_LEFT) != 0;
#pragma unroll
  for (int j = 0; j < 8; j++) total[j] = left ? total[j] : r.head[j];
  if (r.flags & MAT_HAS_TAIL) {
    mat_store(out, r.hkey, total);
#pragma unroll
    for (int j = 0; j < 8; j++) total[j] = r.last[j];
  }
  if (r.flags & MAT_ENDS_TILE) {
    carry[0] = r.lkey;
    mat_store(carry, 1, total);
  } else if (!(r.flags & MAT_OPEN_RIGHT)) {
    mat_store(out, r.lkey, total);
  }
}

// The fold of the tile carries, in tile order (so sorted by segment): carry c starts a sum of its own unless carry
// c - 1 has its segment, and the last carry of a segment adds the sum into the output, which holds what the tile in
// which the segment ends stored, or the 0 of the clear if it ends with a tile.
MSMZ_HD void mat_fold_part(MatPart& a, const uint32_t* carries, uint32_t c) {
  const uint32_t* p = carries + (size_t)c * MAT_CARRY_WORDS;
  a.reset = c == 0 || p[0] != p[-MAT_CARRY_WORDS] ? 1u : 0u;
  mat_load(a.v, p, 1);
}
MSMZ_HD bool mat_fold_ends(const uint32_t* carries, uint32_t c, uint32_t count) {
  const uint32_t* p = carries + (size_t)c * MAT_CARRY_WORDS;
  return c + 1 == count || p[0] != p[MAT_CARRY_WORDS];
}
template <class Fr>
MSMZ_HD void mat_fold_apply(uint32_t* out, uint32_t key, const uint32_t* total) {
  uint32_t o[8];
  mat_load(o, out, key);
  fr_add<Fr>(o, o, total);
  mat_store(out, key, o);
}

}  // namespace msmz

#if defined(__HIPCC__)
namespace msmz {

// val[p] = set[perm[p]] 2^256 mod q: the values of a form, gathered out of the caller's scalar set in sorted order.
// perm is a permutation of [0, nnz), so every value of the range is read; one >= q raises bit 2 of *err.
template <class Fr>
__global__ void __launch_bounds__(256) k_matrix_pack(uint32_t* val, const uint32_t* set, const uint32_t* perm,
                                                     uint32_t nnz, uint32_t* err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  uint32_t v[8];
  if (fr_load<Fr>(v, set, perm[i])) atomicOr(err, 4u);
  fr_to_mont<Fr>(v, v);
  fr_store(val, i, v);
}

// a -> the combination of the parts of all threads up to and including this one, excl -> up to but excluding it.
// Within a wave by shuffles (as fr_wave_sum, with `reset` as the key), the four waves through LDS.  Every thread of the
// workgroup must be here; it may be called again in a loop.
template <class Fr>
__device__ __forceinline__ void mat_block_scan(MatPart& a, MatPart& excl) {
  __shared__ MatPart sh[MAT_THREADS / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    MatPart o;
    o.reset = (uint32_t)__shfl_up((int)a.reset, d, 64);
#pragma unroll
    for (int j = 0; j < 8; j++) o.v[j] = (uint32_t)__shfl_up((int)a.v[j], d, 64);
    if (lane < (uint32_t)d) mat_part_identity(o);
    mat_combine<Fr>(a, o);
  }
  excl.reset = (uint32_t)__shfl_up((int)a.reset, 1, 64);
#pragma unroll
  for (int j = 0; j < 8; j++) excl.v[j] = (uint32_t)__shfl_up((int)a.v[j], 1, 64);
  if (lane == 0) mat_part_identity(excl);
  __syncthreads();   // (a second call: everyone has read sh of the first)
  if (lane == 63u) sh[wave] = a;
  __syncthreads();
  MatPart prefix;
  mat_part_identity(prefix);
#pragma unroll
  for (uint32_t u = 0; u + 1 < MAT_THREADS / 64; u++) {
    if (u < wave) {   // (the same in every lane of a wave)
      MatPart w = sh[u];
      mat_combine<Fr>(w, prefix);
      prefix = w;
    }
  }
  mat_combine<Fr>(a, prefix);
  mat_combine<Fr>(excl, prefix);
}

// One tile of the product: thread t walks non-zeros [tile + t MAT_RUN, + MAT_RUN), the workgroup's segmented scan
// tells it what the runs to its left leave for its head, and it stores what ends in its run (mat_finish).  `out` was
// cleared before this launch; carry record blockIdx.x receives the tile's carry.  An entry of x >= q that a non-zero
// reads raises bit 2 of *err; entries no non-zero reads are not loaded.
template <class Fr>
__global__ void __launch_bounds__(MAT_THREADS) k_matrix_mul(uint32_t* out, MatView m, const uint32_t* x, uint32_t nnz,
                                                            uint32_t* carry, uint32_t* err) {
  const uint64_t tile_first = (uint64_t)blockIdx.x * MAT_TILE;
  const uint64_t tile_end = tile_first + MAT_TILE < nnz ? tile_first + MAT_TILE : (uint64_t)nnz;
  const uint64_t first = tile_first + (uint64_t)threadIdx.x * MAT_RUN;
  const bool active = first < tile_end;
  MatRun r;
  MatPart a, excl;
  mat_part_identity(a);
  if (active) {
    const uint64_t left = tile_end - first;
    mat_run<Fr>(r, out, m, x, first, left < MAT_RUN ? (uint32_t)left : (uint32_t)MAT_RUN, tile_first, tile_end);
    mat_run_part(a, r);
  }
  mat_block_scan<Fr>(a, excl);
  if (active) {
    if (r.flags & MAT_BAD) atomicOr(err, 4u);
    mat_finish<Fr>(out, carry + (size_t)blockIdx.x * MAT_CARRY_WORDS, r, excl);
  }
}

// out[segment] += the sum of the carries of that segment, for all `count` tile carries.  ONE workgroup; a pass of its
// loop scans MAT_FOLD_PASS carries, and the sum a pass ends with goes into the next one through LDS.
template <class Fr>
__global__ void __launch_bounds__(MAT_THREADS) k_matrix_fold(uint32_t* out, const uint32_t* carries, uint32_t count) {
  __shared__ MatPart pass_carry;
  if (threadIdx.x == 0) mat_part_identity(pass_carry);
#pragma unroll 1
  for (uint32_t base = 0; base < count; base += MAT_FOLD_PASS) {
    const uint32_t c = base + threadIdx.x;
    const bool active = c < count;
    MatPart a, excl;
    mat_part_identity(a);
    if (active) mat_fold_part(a, carries, c);
    mat_block_scan<Fr>(a, excl);   // (its barriers also order the pass_carry of the pass before)
    const MatPart before = pass_carry;
    mat_combine<Fr>(a, before);
    if (active && mat_fold_ends(carries, c, count)) mat_fold_apply<Fr>(out, carries[(size_t)c * MAT_CARRY_WORDS], a.v);
    __syncthreads();
    if (threadIdx.x == MAT_THREADS - 1) pass_carry = a;
  }
}

}  // namespace msmz
#endif

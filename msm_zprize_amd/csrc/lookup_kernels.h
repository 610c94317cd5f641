// Multiplicities of a column in a table (msmz_scalars_lookup, include/msmz.h): for a table t of
// table_n resident scalars and a column f of col_n,
//     m_j = #{ i : f_i = t_j }  if j is the LOWEST index among the table entries that hold the value t_j,  else 0,
// the vector a logUp argument commits to.  A join on 256-bit keys, not arithmetic mod q: values are compared as the
// canonical integers the records hold.
//
// The data structure is an open-addressing hash index in engine scratch: S = lk_slots(table_n) slots, the power of two
// with 2 table_n <= S < 4 table_n, each a uint32_t that holds a table index or LK_EMPTY.  The load is at most 1/2, so a
// probe always ends at an empty slot.  The first slot of a key is lk_hash of its eight words, masked; probing is linear
// with wrap-around.  Beside the index sits one uint32_t count per table entry.  Three kernels:
//     k_lookup_insert  one thread per table entry: its index into the slot of its value (lk_insert),
//     k_lookup_count   one thread per column entry: probe, count[k] += 1 (lk_count); for a table of at most
//                      LK_SMALL_TABLE entries k_lookup_count_small, the same body in a loop with the counts in LDS,
//     k_lookup_emit    one thread per table entry: count[j] widened to a 32-byte scalar (lk_emit).
//
// Why the index is the same whatever the interleaving of the threads of k_lookup_insert.  Call the table entries that
// hold one value a class.  (1) A slot goes from LK_EMPTY to an index by ONE successful compare-and-swap and is never
// emptied; afterwards only atomicMin(slot, j) with t_j equal to the occupant's value touches it, so the CLASS of an
// occupied slot never changes.  (2) All threads of a class walk the same slot sequence.  Suppose two of them settled in
// different slots a before b of that sequence.  The one in b passed a and saw it occupied by another class; the one in a
// found a empty or occupied by its own class: with (1) the two cannot both be true.  So a class settles in exactly one
// slot, exactly one of its threads -- the one whose compare-and-swap filled that slot -- counts a distinct value, and every
// other thread of the class applies atomicMin to the same slot: it ends holding the lowest index of the class.  (3) Which
// slot a class takes can depend on the interleaving (two classes that collide may end in either order), but nothing that
// leaves the call does: between the first slot of a value and its class's slot every slot is occupied (the thread that
// filled the class's slot walked them), by other classes, so a probe for the value passes them and ends at its class's
// slot with the lowest index of the class; a value in no class ends at an empty slot.  Counts, positions and result
// words are functions of the classes alone.
//
// The first part of this file is host/device code: the hash, the probe, the comparison and the bodies of the kernels,
// with the atomic operations behind a policy (the device policies below; tests/native/lookup_test.cpp has a sequential
// one and runs the bodies on the CPU in any thread order).  The kernels follow, for the device compiler only.
#pragma once
#include <cstddef>
#include <cstdint>

#include "fr.h"

namespace msmz {

constexpr int LK_THREADS = 256;               // threads per workgroup of all three kernels
constexpr uint32_t LK_EMPTY = 0xffffffffu;    // an empty slot; a position without a match; first_missing without one
constexpr uint64_t LK_MAX_TABLE = 1ull << 30;  // table_n <= this: S <= 2^31 and every index is below LK_EMPTY
constexpr uint32_t LK_SMALL_TABLE = 4096;     // table_n <= this: k_lookup_count_small keeps the counts of a workgroup in LDS
constexpr uint32_t LK_SMALL_PASSES = 16;      // ... a workgroup of it takes at least this many passes of LK_THREADS entries
constexpr uint32_t LK_SMALL_GROUPS = 1024;    // ... unless that needs more workgroups than this

// the result words as the kernels leave them, at the head of the result buffer; the positions follow from LK_RES_WORDS
enum { LK_RES_ERR = 0, LK_RES_MISSING = 1, LK_RES_FIRST = 2, LK_RES_DISTINCT = 3, LK_RES_WORDS = 4 };

// S: the power of two with 2 table_n <= S < 4 table_n (table_n >= 1)
MSMZ_HD uint32_t lk_slots(uint64_t table_n) {
  uint32_t s = 2;
  while ((uint64_t)s < 2 * table_n) s <<= 1;
  return s;
}

// the workgroups of k_lookup_count_small for a column of col_n entries: LK_SMALL_PASSES passes each, LK_SMALL_GROUPS at
// the most (every workgroup ends with up to table_n adds to the same few cache lines)
MSMZ_HD uint32_t lk_small_groups(uint64_t col_n) {
  const uint64_t per = (uint64_t)LK_THREADS * LK_SMALL_PASSES, g = (col_n + per - 1) / per;
  return (uint32_t)(g < LK_SMALL_GROUPS ? g : LK_SMALL_GROUPS);
}

// The 32-bit MurmurHash3 of the 32 bytes of a canonical value (Appleby, public domain): every word goes through two
// multiplications and a rotation before it meets the state, the state is rotated and re-multiplied per word, and the
// final avalanche lets every input bit reach every output bit.  So consecutive integers (only word 0 differs) and values
// that differ only in word 7 both spread over the low bits that the mask keeps.
MSMZ_HD uint32_t lk_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
MSMZ_HD uint32_t lk_hash(const uint32_t* w) {
  uint32_t h = 0x9e3779b9u;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    uint32_t k = w[j] * 0xcc9e2d51u;
    k = lk_rotl(k, 15) * 0x1b873593u;
    h = lk_rotl(h ^ k, 13) * 5u + 0xe6546b64u;
  }
  h ^= 32u;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
// the first slot probed for a key, and the one after slot s
MSMZ_HD uint32_t lk_first_slot(const uint32_t* w, uint32_t mask) { return lk_hash(w) & mask; }
MSMZ_HD uint32_t lk_next_slot(uint32_t s, uint32_t mask) { return (s + 1) & mask; }

MSMZ_HD void lk_load(uint32_t* s, const uint32_t* set, uint64_t i) {
  const uint32_t* p = static_cast<const uint32_t*>(__builtin_assume_aligned(set + (size_t)i * 8, 16));
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = p[j];
}
MSMZ_HD bool lk_equal(const uint32_t* a, const uint32_t* b) {
  uint32_t d = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) d |= a[j] ^ b[j];
  return d == 0;
}

// the index as a probe sees it
struct LkIndex {
  uint32_t* slots;
  uint32_t mask;           // S - 1
  const uint32_t* table;   // record 0 of the table range
};

// What a policy provides (every operation on 32-bit words, device scope):
//   uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v)   compare-and-swap, returns what *p held
//   void     amin(uint32_t* p, uint32_t v)                   *p = min(*p, v)
//   void     raise(uint32_t* err)                            sets the error word
//   void     tally(uint32_t* counter, bool on)               *counter += the number of threads that pass on == true
//   void     tally_at(uint32_t* base, uint32_t k, bool on)   base[k] += the same, per distinct k
//   void     tally_min(uint32_t* counter, uint32_t* lowest, uint32_t i, bool on)   ... and *lowest = min(*lowest, i)
// The three tally calls are reached by EVERY thread of a wave, whatever `on` says: the device policy aggregates over the
// wave before anything reaches memory.

// k_lookup_insert, one thread: table entry j into the index.  live == false: a thread beyond the table.
template <class Fr, class Ops>
MSMZ_HD void lk_insert(Ops& ops, const LkIndex& ix, uint32_t* res, uint64_t j, bool live) {
  bool fresh = false;
  if (live) {
    uint32_t key[8];
    lk_load(key, ix.table, j);
    if (words_geq<8>(key, Fr::Q)) {
      ops.raise(res + LK_RES_ERR);
    } else {
      uint32_t s = lk_first_slot(key, ix.mask);
      for (;;) {
        const uint32_t k = ops.cas(ix.slots + s, LK_EMPTY, (uint32_t)j);
        if (k == LK_EMPTY) {
          fresh = true;
          break;
        }
        uint32_t other[8];
        lk_load(other, ix.table, k);
        if (lk_equal(key, other)) {
          ops.amin(ix.slots + s, (uint32_t)j);
          break;
        }
        s = lk_next_slot(s, ix.mask);
      }
    }
  }
  ops.tally(res + LK_RES_DISTINCT, fresh);
}

// the table index in the slot of `key`'s class, or LK_EMPTY.  For a finished index only (after k_lookup_insert).
MSMZ_HD uint32_t lk_find(const LkIndex& ix, const uint32_t* key) {
  uint32_t s = lk_first_slot(key, ix.mask);
  for (;;) {
    const uint32_t k = ix.slots[s];
    if (k == LK_EMPTY) return LK_EMPTY;
    uint32_t other[8];
    lk_load(other, ix.table, k);
    if (lk_equal(key, other)) return k;
    s = lk_next_slot(s, ix.mask);
  }
}

// k_lookup_count, one thread: column entry i.  pos: nullptr, or where position i goes.
template <class Fr, class Ops>
MSMZ_HD void lk_count(Ops& ops, const LkIndex& ix, uint32_t* count, uint32_t* res, uint32_t* pos, const uint32_t* col,
                      uint64_t i, bool live) {
  uint32_t k = LK_EMPTY;
  bool found = false, missing = false;
  if (live) {
    uint32_t key[8];
    lk_load(key, col, i);
    if (words_geq<8>(key, Fr::Q)) {
      ops.raise(res + LK_RES_ERR);
    } else {
      k = lk_find(ix, key);
      found = k != LK_EMPTY;
      missing = !found;
    }
    if (pos) pos[i] = k;
  }
  ops.tally_at(count, k, found);
  ops.tally_min(res + LK_RES_MISSING, res + LK_RES_FIRST, (uint32_t)i, missing);
}

// k_lookup_emit, one thread: out record j = count[j] as a canonical scalar (a count is below 2^32 < q)
MSMZ_HD void lk_emit(uint32_t* out, const uint32_t* count, uint64_t j) {
  uint32_t* o = static_cast<uint32_t*>(__builtin_assume_aligned(out + (size_t)j * 8, 16));
  o[0] = count[j];
#pragma unroll
  for (int w = 1; w < 8; w++) o[w] = 0;
}

}  // namespace msmz

#if defined(__HIPCC__)
namespace msmz {

// The device policies.  Slots, counts and result words see only 32-bit device-scope atomics, and as few of them as the
// kernel can arrange: atomics on one cache line serialise in the L2, about 10 ns each on an MI355X, so a column that is
// mostly padding, or any column over a table of a few hundred entries, is bound by them and by nothing else.
//
// LkDeviceOps: the wave level.  A __ballot collects the lanes that add, ONE lane adds their population count.  For
// tally_at the lanes are grouped by k in a loop that peels one distinct k per iteration (the k of the lowest lane not yet
// served, read with readlane; a second ballot finds its lanes): a wave whose lanes all hit one table entry sends one add
// instead of 64, a wave of 64 distinct entries runs 64 short iterations of scalar work beside probes that wait on memory.
struct LkDeviceOps {
  __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
  __device__ __forceinline__ void amin(uint32_t* p, uint32_t v) { atomicMin(p, v); }
  __device__ __forceinline__ void raise(uint32_t* err) { atomicOr(err, 1u); }
  __device__ __forceinline__ uint32_t lane() const { return __lane_id(); }
  __device__ __forceinline__ void tally(uint32_t* counter, bool on) {
    const unsigned long long who = __ballot(on);
    if (who && lane() == (uint32_t)(__ffsll(who) - 1)) atomicAdd(counter, (uint32_t)__popcll(who));
  }
  __device__ __forceinline__ void tally_min(uint32_t* counter, uint32_t* lowest, uint32_t i, bool on) {
    const unsigned long long who = __ballot(on);
    if (who && lane() == (uint32_t)(__ffsll(who) - 1)) {   // (the lowest lane holds the lowest i of the wave)
      atomicAdd(counter, (uint32_t)__popcll(who));
      atomicMin(lowest, i);
    }
  }
};

// k_lookup_insert: the distinct values of a workgroup are summed in LDS first (a table of all distinct values would
// otherwise send one add per wave to one address).  `sum` is one zeroed word of LDS; flush() after the body.
struct LkInsertOps : LkDeviceOps {
  uint32_t* sum;
  __device__ __forceinline__ void tally(uint32_t*, bool on) {
    const unsigned long long who = __ballot(on);
    if (who && lane() == (uint32_t)(__ffsll(who) - 1)) atomicAdd(sum, (uint32_t)__popcll(who));
  }
  __device__ __forceinline__ void flush(uint32_t* counter) {
    __syncthreads();
    if (threadIdx.x == 0 && *sum) atomicAdd(counter, *sum);
  }
};

// k_lookup_count, a table beyond LK_SMALL_TABLE: the wave loop above, but the FIRST group a wave peels -- for a column
// of padding, the padding -- goes to LDS, and the first LK_THREADS / 64 threads merge the heads of the workgroup's waves
// that hit the same entry into one add.  Later groups of a wave add directly.  head_k / head_c: one word per wave each.
struct LkBlockOps : LkDeviceOps {
  uint32_t* head_k;
  uint32_t* head_c;
  __device__ __forceinline__ void tally_at(uint32_t* base, uint32_t k, bool on) {
    constexpr uint32_t WAVES = LK_THREADS / 64;
    const uint32_t wave = threadIdx.x >> 6;
    unsigned long long todo = __ballot(on);
    if (!todo && lane() == 0) head_k[wave] = LK_EMPTY, head_c[wave] = 0;
    bool head = true;
    while (todo) {   // (todo is wave-uniform: every lane runs the same iterations)
      const uint32_t leader = (uint32_t)(__ffsll(todo) - 1);
      const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)k, (int)leader);
      const unsigned long long same = __ballot(on && k == k0);
      if (lane() == leader) {
        if (head) head_k[wave] = k0, head_c[wave] = (uint32_t)__popcll(same);
        else atomicAdd(base + k0, (uint32_t)__popcll(same));
      }
      head = false;
      todo &= ~same;
    }
    __syncthreads();
    if (threadIdx.x < WAVES) {
      const uint32_t mine = head_k[threadIdx.x];
      uint32_t c = head_c[threadIdx.x];
      bool first = true;   // the lowest wave with this entry adds for all of them
#pragma unroll
      for (uint32_t w = 0; w < WAVES; w++) {
        if (w < threadIdx.x && head_k[w] == mine) first = false;
        if (w > threadIdx.x && head_k[w] == mine) c += head_c[w];
      }
      if (first && c) atomicAdd(base + mine, c);   // (c == 0: a wave without a match, mine is LK_EMPTY)
    }
  }
};

// k_lookup_count_small, a table of at most LK_SMALL_TABLE entries: the counts of a workgroup live in LDS (`hist`, one
// word per table entry, zeroed before the body) over all the passes of its loop, and only the non-zero ones reach
// memory, once, in flush().
struct LkHistOps : LkDeviceOps {
  uint32_t* hist;
  __device__ __forceinline__ void tally_at(uint32_t*, uint32_t k, bool on) {
    if (on) atomicAdd(hist + k, 1u);
  }
  __device__ __forceinline__ void flush(uint32_t* count, uint32_t table_n) {
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < table_n; j += LK_THREADS) {
      const uint32_t c = hist[j];
      if (c) atomicAdd(count + j, c);
    }
  }
};

// No thread leaves early in the kernels below: the tallies need whole waves, the merges whole workgroups.

template <class Fr>
__global__ void __launch_bounds__(LK_THREADS) k_lookup_insert(uint32_t* slots, uint32_t mask, const uint32_t* table,
                                                              uint32_t table_n, uint32_t* res) {
  __shared__ uint32_t sum;
  if (threadIdx.x == 0) sum = 0;
  __syncthreads();
  const uint64_t j = (uint64_t)blockIdx.x * LK_THREADS + threadIdx.x;
  LkInsertOps ops;
  ops.sum = &sum;
  const LkIndex ix = {slots, mask, table};
  lk_insert<Fr>(ops, ix, res, j, j < table_n);
  ops.flush(res + LK_RES_DISTINCT);
}

template <class Fr>
__global__ void __launch_bounds__(LK_THREADS) k_lookup_count(uint32_t* count, uint32_t* res, uint32_t* pos,
                                                             uint32_t* slots, uint32_t mask, const uint32_t* table,
                                                             const uint32_t* col, uint32_t col_n) {
  __shared__ uint32_t head_k[LK_THREADS / 64], head_c[LK_THREADS / 64];
  const uint64_t i = (uint64_t)blockIdx.x * LK_THREADS + threadIdx.x;
  LkBlockOps ops;
  ops.head_k = head_k, ops.head_c = head_c;
  const LkIndex ix = {slots, mask, table};
  lk_count<Fr>(ops, ix, count, res, pos, col, i, i < col_n);
}

template <class Fr>
__global__ void __launch_bounds__(LK_THREADS) k_lookup_count_small(uint32_t* count, uint32_t* res, uint32_t* pos,
                                                                   uint32_t* slots, uint32_t mask, const uint32_t* table,
                                                                   uint32_t table_n, const uint32_t* col, uint32_t col_n) {
  __shared__ uint32_t hist[LK_SMALL_TABLE];
  for (uint32_t j = threadIdx.x; j < table_n; j += LK_THREADS) hist[j] = 0;
  __syncthreads();
  LkHistOps ops;
  ops.hist = hist;
  const LkIndex ix = {slots, mask, table};
  const uint64_t stride = (uint64_t)gridDim.x * LK_THREADS;
  for (uint64_t first = (uint64_t)blockIdx.x * LK_THREADS; first < col_n; first += stride) {   // (uniform in the workgroup)
    const uint64_t i = first + threadIdx.x;
    lk_count<Fr>(ops, ix, count, res, pos, col, i, i < col_n);
  }
  ops.flush(count, table_n);
}

template <class Fr>
__global__ void __launch_bounds__(LK_THREADS) k_lookup_emit(uint32_t* out, const uint32_t* count, uint32_t table_n) {
  const uint64_t j = (uint64_t)blockIdx.x * LK_THREADS + threadIdx.x;
  if (j < table_n) lk_emit(out, count, j);
}

}  // namespace msmz
#endif

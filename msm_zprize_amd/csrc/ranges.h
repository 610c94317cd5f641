// The range predicates every entry point that takes `first` and `n` asks.  Host only; no sum of two caller-given
// 64-bit values is ever formed.
#pragma once
#include <cstdint>

namespace msmz {

// is [first, first + n) inside a set of `len` records?  (no first + n: it can wrap)
static inline bool in_range(uint64_t first, uint64_t n, uint64_t len) { return first <= len && n <= len - first; }

// do the ranges [a, a + n) and [b, b + n) of one set overlap in part?  Equal starts are an in-place operation and
// allowed; a distance of n or more is disjoint.
static inline bool partial_overlap(uint64_t a, uint64_t b, uint64_t n) { return a != b && (a > b ? a - b : b - a) < n; }

// the same question for ranges of different lengths, [a, a + na) and [b, b + nb): do they meet without being one range?
static inline bool ranges_clash(uint64_t a, uint64_t na, uint64_t b, uint64_t nb) {
  if (a == b && na == nb) return false;
  return a < b ? b - a < na : a - b < nb;
}

// do [a, a + na) and [b, b + nb) meet at all?  For an operation that gathers: no entry may be both read and written.
static inline bool ranges_meet(uint64_t a, uint64_t na, uint64_t b, uint64_t nb) { return a < b ? b - a < na : a - b < nb; }

}  // namespace msmz

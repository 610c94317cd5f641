// What one engine keeps on its device and hands out by id: owning device and pinned host buffers, the handle of a
// resident set, and the table of handles.  Everything here frees itself, on whatever device is selected at the time:
// the engine's destructor selects its own first (SetsCore::~SetsCore, sets_core.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <utility>

#include "../../include/msmz.h"
#include "ranges.h"

namespace msmz {

#define MSMZ_HIP(x)                                                                        \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      fprintf(stderr, "msmz: HIP error '%s' from `%s` at %s:%d\n", hipGetErrorString(e_), #x, __FILE__, __LINE__); \
      return MSMZ_ERR_HIP;                                                                 \
    }                                                                                      \
  } while (0)

// msmz_test_poison (include/msmz_test.h): the byte an armed engine fills every device buffer with that ensure newly
// allocates (-1: not armed), on the engine's stream.  One per engine; a DevBuf bound to it points here (`poison`).
struct Poison {
  int pattern = -1;
  hipStream_t stream = nullptr;
};

// Memory owned by one object, grow-only: freed when it goes out of scope, so every error path releases it.  DEVICE:
// device memory, grown with headroom.  Otherwise pinned host memory: where a device-to-host copy lands, or a
// host-to-device copy starts, without a second host wait.  What a new allocation holds is undefined ("Scratch
// is undefined at the start of every call"): a device buffer bound to an armed Poison is filled to show it.
template <bool DEVICE>
struct PoisonRef {                  // (only a device buffer carries one)
  const Poison* poison = nullptr;   // the owning engine's, or null: never filled
};
template <>
struct PoisonRef<false> {};

template <bool DEVICE>
struct OwnedBuf : PoisonRef<DEVICE> {
  void* p = nullptr;
  size_t bytes = 0;
  OwnedBuf() = default;
  OwnedBuf(OwnedBuf&& o) noexcept : PoisonRef<DEVICE>(o), p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) {
      release();
      PoisonRef<DEVICE>::operator=(o);
      p = o.p, bytes = o.bytes;
      o.p = nullptr, o.bytes = 0;
    }
    return *this;
  }
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  ~OwnedBuf() { release(); }
  int ensure(size_t need) {
    if (need <= bytes) return MSMZ_OK;
    release();
    size_t sz = need;
    if constexpr (DEVICE) {
      sz = need + need / 8;
      if (hipMalloc(&p, sz) != hipSuccess) {
        if (hipMalloc(&p, need) != hipSuccess) return MSMZ_ERR_HIP;
        sz = need;
      }
    } else {
      MSMZ_HIP(hipHostMalloc(&p, need));
    }
    bytes = sz;
    if constexpr (DEVICE) MSMZ_HIP(fill_if_armed());
    return MSMZ_OK;
  }
  // exactly `need` bytes for an empty buffer: the records of a new handle, which never grow
  int alloc_exact(size_t need) {
    static_assert(DEVICE, "handles live on the device");
    MSMZ_HIP(hipMalloc(&p, need));
    bytes = need;
    MSMZ_HIP(fill_if_armed());
    return MSMZ_OK;
  }
  // msmz_test_poison: what was just allocated, filled with the armed engine's byte before anything else touches it
  hipError_t fill_if_armed() {
    const Poison* a = this->poison;
    return a && a->pattern >= 0 ? hipMemsetAsync(p, a->pattern, bytes, a->stream) : hipSuccess;
  }
  void release() {
    if (p) (void)(DEVICE ? hipFree(p) : hipHostFree(p));
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};
using DevBuf = OwnedBuf<true>;
using PinnedBuf = OwnedBuf<false>;

// a PinnedBuf that holds one T, read in place (h_meta_->error)
template <class T>
struct PinnedOne : PinnedBuf {
  T* operator->() const { return as<T>(); }
};

struct Handle {
  int kind = 0;             // 0 = points, 1 = scalars, 2 = a sparse matrix
  uint64_t n = 0;
  bool has_endo = false;    // points: records [n, 2n) hold the endomorphism images
  DevBuf mem;
  // precomputed point set (msmz_precompute_points): `factor` copies, copy j = records [j R, (j + 1) R) holds 2^(c j) P_i
  // (R = copy_stride = n, or 2 n with the endomorphism images); built for window size c and GLV choice glv.  0 = plain.
  uint32_t factor = 0;
  int c = 0, glv = 0;
  uint64_t copy_stride = 0;
  int sbits = 0;   // scalar bit bound the copies were built for (Planner::bound: 0 = none)
  // sparse matrix (msmz_matrix_create): n = its non-zeros; form[0] sorted by row (MSMZ_MAT_ROWS), form[1] by column
  // (MSMZ_MAT_COLS), each n gathered indices, n segment indices and, with has_vals, n values of 8 words from byte
  // offset mat_val_offset(n) (matrix_kernels.h); an orientation the matrix was not built for has an empty buffer
  uint32_t n_rows = 0, n_cols = 0, mat_flags = 0;
  bool has_vals = false;
  DevBuf form[2];
};

// The handles of one engine by id.  Ids start at 1 and are never reused.
class HandleTable {
 public:
  // the handle `h` if it is of `kind`, or null
  Handle* get(uint64_t h, int kind) {
    auto it = map_.find(h);
    return it == map_.end() || it->second.kind != kind ? nullptr : &it->second;
  }
  // -> record `first` of handle `h` of `kind`, its records `stride` words apart (8: scalars, PW_WORDS: points), if
  // [first, first + n) lies inside the set's n records; or null
  uint32_t* range(uint64_t h, int kind, uint64_t first, uint64_t n, size_t stride) {
    Handle* hd = get(h, kind);
    return hd && in_range(first, n, hd->n) ? hd->mem.as<uint32_t>() + first * stride : nullptr;
  }
  uint64_t add(Handle&& hd) {
    map_.emplace(next_, std::move(hd));
    return next_++;
  }
  bool known(uint64_t h) const { return map_.count(h) != 0; }
  void erase(uint64_t h) { map_.erase(h); }

 private:
  std::map<uint64_t, Handle> map_;
  uint64_t next_ = 1;
};

}  // namespace msmz

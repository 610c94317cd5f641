// What every family of operations on the resident sets of one engine needs, and nothing a single family owns: the device
// and its ONE HIP stream, the handle table, the staging buffer, the meta block, and the one way a result comes home.
// ResidentSets<Cfg> (resident.h) derives from this and keeps the sets themselves; the family stages (point_ops.h,
// scalar_ops.h, ntt_ops.h, matrix_ops.h, lookup_ops.h, expr_ops.h) are built with a reference to it.
//
// The result-record contract.  Every entry point returns with the stream drained, and reaches its ONE host wait through
// one of three helpers: drained() (nothing comes back), checked() (the 4-byte error word of the meta block) or recorded()
// (a record at the head of a family buffer, and what lies behind it, into h_res_).  Each of them, and every other helper
// here that queues work, waits for the stream before it returns a failure that came after something was queued.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/msmz.h"
#include "kernels.h"
#include "scalar_kernels.h"
#include "iengine.h"
#include "store.h"

namespace msmz {

template <class Cfg> class PointOps;
template <class Cfg> class ScalarOps;
template <class Cfg> class NttOps;
template <class Cfg> class MatrixOps;
template <class Cfg> class LookupOps;
template <class Cfg> class ExprOps;

template <class Cfg>
class SetsCore : public IEngine {
  friend class PointOps<Cfg>;
  friend class ScalarOps<Cfg>;
  friend class NttOps<Cfg>;
  friend class MatrixOps<Cfg>;
  friend class LookupOps<Cfg>;
  friend class ExprOps<Cfg>;

 protected:
  using F = typename Cfg::F;
  using Fr = typename Cfg::Fr;
  static constexpr int NW = F::NW;
  static constexpr int RW = 2 * NW;      // affine record words
  static constexpr int FE_BYTES = NW * 4;
  using P = typename Cfg::P;             // the group policy: formulas and record formats (kernels.h)
  static constexpr bool TE = Cfg::TE;
  static constexpr int PW_WORDS = P::IN_WORDS;   // words between the records of a resident point set

  explicit SetsCore(int device) : device_(device) {}

  // the device, the stream, and the pinned landing of the meta block (ResidentSets::init_sets goes on from here)
  int init_core() {
    MSMZ_HIP(hipSetDevice(device_));
    MSMZ_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    poison_.stream = stream_;
    return h_meta_.ensure(sizeof(MsmMeta));
  }

  // f(buffer) for the scratch every family shares: undefined at the start of every call
  template <class Fn>
  void each_scratch(Fn f) {
    f(stage_), f(meta_);
  }

 public:
  ~SetsCore() override {   // (the device buffers and handles free themselves after this, on this device)
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamDestroy(stream_);
  }

 protected:
  // ------------------------------------------------------------------------------------------ launch geometry
  // the one-thread-per-record kernels: blocks_of(n) workgroups of kBlock threads
  static constexpr uint32_t kBlock = 256;
  static dim3 blocks_of(uint64_t n) { return dim3((uint32_t)((n + kBlock - 1) / kBlock)); }

  // ------------------------------------------------------------------------------------------ the way home
  // the host wait behind what has been queued: `queued` if that failed, else what the wait itself reports
  int wait_after(hipError_t queued) {
    const hipError_t waited = hipStreamSynchronize(stream_);
    MSMZ_HIP(queued);
    MSMZ_HIP(waited);
    return MSMZ_OK;
  }

  // the ONE host wait of an operation that reads nothing back and has no error word (generators, powers, tables)
  int drained() { return wait_after(hipGetLastError()); }

  // *word = the meta error word as the launches queued so far leave it (one host round trip).  What a bit means is the
  // caller's to say: it differs between the kernels that raise them.
  int fetch_error(uint32_t* word) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&h_meta_->error, &meta_.as<MsmMeta>()->error, 4, hipMemcpyDeviceToHost, stream_);
    if (int st = wait_after(e)) return st;
    *word = h_meta_->error;
    return MSMZ_OK;
  }

  // zeroes the error word, runs launch(its device address), fetches it: MSMZ_ERR_RANGE if a kernel raised a bit; bit 3
  // alone (k_import_points_compressed: a record that is no point) is MSMZ_ERR_POINT, so RANGE wins when both occur
  template <class Launch>
  int checked(Launch launch) {
    uint32_t* d_err = &meta_.as<MsmMeta>()->error;
    const hipError_t e = hipMemsetAsync(d_err, 0, 4, stream_);
    if (e != hipSuccess) return wait_after(e);   // (the caller may have queued copies)
    launch(d_err);
    uint32_t err = 0;
    if (int st = fetch_error(&err)) return st;
    return (err & ~8u) ? MSMZ_ERR_RANGE : err ? MSMZ_ERR_POINT : MSMZ_OK;
  }

  // The result record at the head of a family buffer, and how it comes home.
  struct Record {
    size_t head = 64;       // bytes at the head of the buffer: zeroed before the launches, written by them
    int err_word = 8;       // the word of the head that is the error word (set: MSMZ_ERR_RANGE), or -1: there is none
    int preset_word = -1;   // a word of the head that starts as 0xffffffff, the "none yet" of an atomicMin, or -1
    size_t tail = 0;        // bytes behind the head that come home with it (verdicts, positions)
  };
  // `buf` is grown to `bytes` (the record and the family's scratch behind it); its head is zeroed in stream order (one
  // word preset), launch(its device address) queues the kernels, and head + tail land in h_res_ (pinned, grown as
  // needed) in ONE copy behind ONE wait.  The caller reads its words and its tail out of h_res_ afterwards.
  template <class Launch>
  int recorded(DevBuf& buf, size_t bytes, Launch launch, Record r = {}) {
    if (int st = buf.ensure(bytes)) return st;
    if (int st = h_res_.ensure(r.head + r.tail)) return st;
    uint32_t* d_res = buf.as<uint32_t>();
    hipError_t e = hipMemsetAsync(d_res, 0, r.head, stream_);
    if (e == hipSuccess && r.preset_word >= 0) e = hipMemsetAsync(d_res + r.preset_word, 0xff, 4, stream_);
    if (e == hipSuccess) {
      launch(d_res);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_res_.p, d_res, r.head + r.tail, hipMemcpyDeviceToHost, stream_);
    if (int st = wait_after(e)) return st;
    return r.err_word >= 0 && h_res_.template as<const uint32_t>()[r.err_word] ? MSMZ_ERR_RANGE : MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ copies
  // Host -> device copy of this engine's `n` local records of `rec` bytes.  split == nullptr: one contiguous copy.
  // Otherwise the engine is shard `split->shard` of `split->nshards` inside a multi-device context (multi.h): its local
  // block b is global block b * nshards + shard of the caller's buffer, so every block is copied straight from where
  // the caller has it -- no gathered host copy in between.  (A failure drains the stream: earlier blocks may be queued.)
  int copy_h2d(void* dst, const uint8_t* src, size_t rec, uint64_t n, const GenMap* split) {
    if (!split || split->nshards <= 1) {
      const hipError_t e = hipMemcpyAsync(dst, src, n * rec, hipMemcpyHostToDevice, stream_);
      return e == hipSuccess ? (int)MSMZ_OK : wait_after(e);
    }
    const uint64_t blk = 1ull << split->blk_shift;
    for (uint64_t li = 0; li < n; li += blk) {
      const uint64_t len = n - li < blk ? n - li : blk;
      const uint64_t gi = ((li >> split->blk_shift) * split->nshards + split->shard) << split->blk_shift;
      const hipError_t e = hipMemcpyAsync((uint8_t*)dst + li * rec, src + gi * rec, len * rec, hipMemcpyHostToDevice, stream_);
      if (e != hipSuccess) return wait_after(e);
    }
    return MSMZ_OK;
  }

  // `count` resident point records from `recs` as canonical x || y in the caller's host memory (k_points_from_resident
  // through stage_): one launch, one copy, ONE wait
  int fetch_points(const uint32_t* recs, uint64_t count, uint8_t* xy) {
    MSMZ_HIP(hipSetDevice(device_));
    if (int st = stage_.ensure(count * RW * 4)) return st;
    hipLaunchKernelGGL((k_points_from_resident<P>), blocks_of(count), dim3(kBlock), 0, stream_, stage_.as<uint32_t>(), recs,
                       (uint32_t)count);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(xy, stage_.p, count * RW * 4, hipMemcpyDeviceToHost, stream_);
    return wait_after(e);
  }

  // ------------------------------------------------------------------------------------------ handles and ranges
  // record indices of a point set (incl. the endomorphism images) fit 30 bits
  static bool points_fit(uint64_t n) { return n != 0 && n < (1ull << (Cfg::HAS_ENDO ? 29 : 30)); }

  // a new handle and its device memory (owned by it: an error before add_handle frees it)
  int new_handle(Handle* hd, int kind, uint64_t n, bool endo, size_t bytes) {
    *hd = Handle{kind, n, endo};
    hd->mem.poison = hd->form[0].poison = hd->form[1].poison = &poison_;
    return hd->mem.alloc_exact(bytes);
  }
  int new_points(uint64_t n, Handle* hd) {
    if (!points_fit(n)) return MSMZ_ERR_ARG;
    return new_handle(hd, 0, n, Cfg::HAS_ENDO, (size_t)n * PW_WORDS * 4 * (Cfg::HAS_ENDO ? 2 : 1));
  }
  int new_scalars(uint64_t n, Handle* hd) { return new_handle(hd, 1, n, false, n * 32); }
  // the memory of a fresh destination (resolve left *out null): hd owns it until add_handle
  int fresh_out(uint64_t n, Handle* hd, uint32_t** out) {
    if (*out) return MSMZ_OK;
    if (int st = new_scalars(n, hd)) return st;
    *out = hd->mem.template as<uint32_t>();
    return MSMZ_OK;
  }
  int add_handle(Handle&& hd, uint64_t* h) {
    *h = handles_.add(std::move(hd));
    return MSMZ_OK;
  }

  // *recs -> record `first` of point set `h` if a download or an export may read [first, first + n): the endomorphism
  // images stay readable; a precomputed set: all its copies
  int point_records(uint64_t h, uint64_t first, uint64_t n, const uint32_t** recs) {
    const Handle* pts = handles_.get(h, 0);
    if (!pts) return MSMZ_ERR_ARG;
    const uint64_t have = pts->factor ? pts->copy_stride * pts->factor : pts->n * (pts->has_endo ? 2 : 1);
    if (!in_range(first, n, have)) return MSMZ_ERR_ARG;
    *recs = pts->mem.template as<const uint32_t>() + first * PW_WORDS;
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ scalar arguments
  // a broadcast scalar of the caller's (32 bytes, canonical): out = its words, or its Montgomery form; >= q is refused
  static int read_fr(const uint8_t* src, uint32_t out[8], bool to_mont) {
    uint32_t c[8];
    memcpy(c, src, 32);
    if (words_geq<8>(c, Fr::Q)) return MSMZ_ERR_RANGE;
    if (to_mont) fr_to_mont<Fr>(out, c);
    else memcpy(out, c, 32);
    return MSMZ_OK;
  }

  // The operands of combine, recurrence, inverse and ntt.  Every source is a range of n records of a scalar set that does
  // not overlap the destination in part (entry i is read, then written: equal starts are in place).  The destination:
  // records [first_out, first_out + n) of `out_handle`, or, for out_handle == 0, a fresh set -- first_out must be 0 and
  // *out stays null, for the caller to allocate once every check has passed.
  struct Source {
    uint64_t handle, first;
    const uint32_t** p;
    uint64_t n = 0;   // records, where they differ from the destination's (a transform of zero-padded vectors); 0 = n
  };
  int resolve(const std::vector<Source>& srcs, uint64_t n, uint64_t first_out, uint64_t out_handle, uint32_t** out) {
    if (out_handle == 0 && first_out != 0) return MSMZ_ERR_ARG;
    for (const Source& s : srcs) {
      const uint64_t len = s.n ? s.n : n;
      if (s.handle == out_handle && ranges_clash(s.first, len, first_out, n)) return MSMZ_ERR_ARG;
      if (!(*s.p = handles_.range(s.handle, 1, s.first, len, 8))) return MSMZ_ERR_ARG;
    }
    if (out_handle && !(*out = handles_.range(out_handle, 1, first_out, n, 8))) return MSMZ_ERR_ARG;
    return MSMZ_OK;
  }

  int device_;
  hipStream_t stream_ = nullptr;
  HandleTable handles_;
  Poison poison_;                      // msmz_test_poison: armed or not; every device buffer of the engine points here
  DevBuf stage_;                       // host data on its way to a kernel, results on their way back
  DevBuf meta_;                        // MsmMeta: the error word every kernel here reports through; the pipeline's totals
  PinnedOne<MsmMeta> h_meta_;          // ... and its pinned landing
  PinnedBuf h_res_;                    // pinned landing of a result record here, of the window results of an MSM
};

}  // namespace msmz

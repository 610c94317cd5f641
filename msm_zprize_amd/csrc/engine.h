// Host-side MSM engine: the pipeline of one GPU (sort, plan, tree rounds, bucket reduction) over the resident sets of
// ResidentSets (resident.h), from which it derives; it owns the buffers its stages share, sequences the stages (sort.h,
// reduce.h) and its own kernels on the one HIP stream and finishes the K window sums on the host.  This replaces the
// reference's SPMD worker runtime (src/threads/threads.ts:132-359, src/parallel.ts:291-320) and the JS orchestration inside
// `msm` (src/msm-batched-affine.ts:74-328): barriers between phases become stream order, the
// per-thread bucket split (msm-common.ts:88-188) becomes grid sizing.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/msmz.h"
#include "kernels.h"
#include "host64.h"
#include "multi.h"
#include "plan.h"
#include "reduce.h"
#include "resident.h"
#include "run.h"
#include "sort.h"

namespace msmz {

// What an MSM attempt asks of its caller besides its status: nothing, the same MSM again with windows for the proven
// GLV bound (a GLV half was longer than assumed), or this sub-batch's problems one by one (its plan does not batch).
enum class Redo { NONE, PROVEN_BITS, PER_PROBLEM };

// Host-side group addition of two canonical affine points (msmz_point_add; fold_partial, multi.h, folds partial MSM
// results with it).
template <class G>
static int host_point_add(const uint8_t* a, int ai, const uint8_t* b, int bi, uint8_t* out, int* oi) {
  using F = typename G::F;
  constexpr int NW = F::NW;
  if (G::TE && (!a || !b)) return MSMZ_ERR_ARG;   // twisted Edwards has no infinity flag: the identity is (0, 1)
  auto load = [](typename G::Acc& p, const uint8_t* xy, bool inf) {
    if (inf) {
      G::set_identity(p);
      return;
    }
    uint32_t w[2 * NW];
    memcpy(w, xy, sizeof(w));
    Fe<F> x, y, xm, ym;
    fe_unpack<F>(x, w);
    fe_unpack<F>(y, w + NW);
    fe_to_mont(xm, x);
    fe_to_mont(ym, y);
    G::from_affine(p, xm, ym);
  };
  typename G::Acc p, q, r;
  load(p, a, !G::TE && ai);
  load(q, b, !G::TE && bi);
  G::add(r, p, q);
  uint32_t w[2 * NW];
  *oi = G::to_affine_canon(w, r) ? 1 : 0;
  memcpy(out, w, sizeof(w));
  return MSMZ_OK;
}

template <class Cfg>
class TestHooks;   // test_hooks.h

template <class Cfg>
class Engine : public ResidentSets<Cfg> {
  friend class TestHooks<Cfg>;
  using Base = ResidentSets<Cfg>;
  // what the pipeline uses of the resident sets' core (SetsCore, sets_core.h): the curve's types and record sizes, the
  // device and its stream, the handle table, the staging buffer, the meta block with its pinned landing, and the pinned
  // results
  using typename Base::F;
  using typename Base::Fr;
  using Base::NW, Base::RW, Base::FE_BYTES, Base::TE, Base::PW_WORDS;
  using Base::device_, Base::stream_, Base::handles_, Base::stage_, Base::meta_, Base::h_meta_, Base::h_res_;
  using Base::poison_;
  using Base::copy_h2d, Base::fetch_error, Base::new_handle, Base::add_handle;
  static constexpr int XW = 4 * NW;      // XYZZ / extended record words
 public:
  Engine(int curve_id, int device) : Base(device), curve_id_(curve_id) {}

  int init() {
    int st;
    if ((st = Base::init_sets())) return st;
    each_scratch([&](DevBuf& b) { b.poison = &poison_; });
    for (hipEvent_t* e : ev_.all()) MSMZ_HIP(hipEventCreate(e));
    if ((st = h_res_.ensure((size_t)2 * kMaxWindows * XW * 4))) return st;   // the results of one problem
    if ((st = sort_.init(device_))) return st;   // (the sort kernels' LDS limits, once)
    return meta_.ensure(sizeof(MsmMeta) + kTraceBytes * 65536);
  }

 public:
  ~Engine() override {   // (the pipeline's buffers free themselves after this, on this device; then the base's turn)
    (void)hipSetDevice(device_);
    for (hipEvent_t* e : ev_.all())
      if (*e) (void)hipEventDestroy(*e);
  }

  // ------------------------------------------------------------------------------------------ precomputed point sets
  int precompute_params(uint64_t n, const msmz_opts* o, uint32_t factor, int* c_out, int* glv_out,
                        uint32_t* f_out, int* k_out, int* sbits_out) const override {
    if (TE) return MSMZ_ERR_UNSUPPORTED;   // twisted Edwards runs msmBasic: no batched-affine buckets to share
    return planner_.precompute_params(n, o, factor, c_out, glv_out, f_out, k_out, sbits_out);
  }

  // new handle: `F` copies of the first n points of `ph`, copy j = 2^(c j) P_i (+ the endomorphism images with glv)
  int precompute_points(uint64_t ph, uint64_t n, int c, int glv, uint32_t copies, int sbits, uint64_t* h) override {
    if (TE) return MSMZ_ERR_UNSUPPORTED;
    const Handle* plain = handles_.get(ph, 0);
    if (!h || !plain || plain->factor != 0 || n == 0 || plain->n < n || copies < 2 || c < 2 || c > 24) return MSMZ_ERR_ARG;
    const Handle& src = *plain;
    if (glv && !src.has_endo) return MSMZ_ERR_UNSUPPORTED;
    MSMZ_HIP(hipSetDevice(device_));
    const uint64_t R = n * (glv ? 2 : 1);
    const size_t rec = (size_t)PW_WORDS * 4;
    Handle hd;
    if (int st = new_handle(&hd, 0, n, glv != 0, (size_t)copies * R * rec)) return st;
    uint8_t* dev = hd.mem.as<uint8_t>();
    // copy 0: the source's first n points (and their images, which follow the source's whole set)
    MSMZ_HIP(hipMemcpyAsync(dev, src.mem.p, n * rec, hipMemcpyDeviceToDevice, stream_));
    if (glv)
      MSMZ_HIP(hipMemcpyAsync(dev + n * rec, src.mem.template as<const uint8_t>() + src.n * rec, n * rec,
                              hipMemcpyDeviceToDevice, stream_));
    for (uint32_t j = 1; j < copies; j++) {
      if constexpr (!TE)
        hipLaunchKernelGGL((k_precompute_copy<F>), dim3((n + 255) / 256), dim3(256), 0, stream_,
                           (uint32_t*)(dev + j * R * rec), (const uint32_t*)(dev + (j - 1) * R * rec), (uint32_t)n, c, glv);
      MSMZ_HIP(hipGetLastError());
    }
    MSMZ_HIP(hipStreamSynchronize(stream_));
    hd.factor = copies;
    hd.c = c;
    hd.glv = glv;
    hd.copy_stride = R;
    hd.sbits = planner_.bound(sbits);
    return add_handle(std::move(hd), h);
  }

  int precomputed_info(uint64_t hd, int32_t* c, int32_t* glv, uint32_t* factor, uint32_t* K, uint64_t* records,
                       int32_t* sbits) override {
    const Handle* pre = handles_.get(hd, 0);
    if (!pre || pre->factor == 0) return MSMZ_ERR_ARG;
    const Handle& h = *pre;
    const int b = planner_.scalar_bits(h.glv != 0, 0, h.sbits);
    if (sbits) *sbits = h.sbits;
    if (c) *c = h.c;
    if (glv) *glv = h.glv;
    if (factor) *factor = h.factor;
    if (K) *K = (uint32_t)((b + 1 + h.c - 1) / h.c);
    if (records) *records = h.copy_stride * h.factor;
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ msm
  // `batch` MSMs over the first n points: problem k's scalars are entries [k n, (k + 1) n) of the resident set `sh`, or
  // vector k of the host buffer (at host_scalars + k host_stride 32; host_stride = n unless a multi-device context hands
  // this engine its share `split` of longer vectors).  batch = 1 is msmz_msm.  Sub-batches run one after another
  // (run_problems decides how each runs), their logs summed.
  int msm_batch(uint64_t ph, const uint8_t* host_scalars, uint64_t sh, uint64_t n, uint32_t batch, const msmz_opts* o,
                uint8_t* out, int* out_inf, msmz_log* log, const GenMap* split = nullptr,
                uint64_t host_stride = 0) override {
    auto t_begin = std::chrono::steady_clock::now();
    if (!out || !out_inf || n == 0 || batch == 0) return MSMZ_ERR_ARG;
    const Handle* pp = handles_.get(ph, 0);
    if (!pp || !in_range(0, n, pp->n)) return MSMZ_ERR_ARG;
    const Handle& pts = *pp;
    msmz_opts opt;
    if (int st = resolve_opts(pts, o, &opt)) return st;
    if (opt.glv < 0) opt.glv = pts.has_endo && planner_.default_glv(n, opt.reserved[1]) ? 1 : 0;   // (per problem: batch = 1 is msm())
    if (host_stride == 0) host_stride = n;
    if (host_scalars && host_stride < n) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(device_));
    const uint64_t total = (uint64_t)batch * n;
    const uint32_t* d_scalars = nullptr;
    if (host_scalars) {
      // range (< group order) is checked on the device while the scalars are sliced
      int st = stage_.ensure(total * 32);
      if (st) return st;
      if (!split && host_stride == n) {
        if ((st = copy_h2d(stage_.p, host_scalars, 32, total, nullptr))) return st;
      } else {
        for (uint32_t k = 0; k < batch; k++)
          if ((st = copy_h2d(stage_.template as<uint8_t>() + (size_t)k * n * 32, host_scalars + (size_t)k * host_stride * 32, 32, n,
                             split)))
            return st;
      }
      d_scalars = stage_.template as<uint32_t>();
    } else if (!(d_scalars = handles_.range(sh, 1, 0, total, 8))) {
      return MSMZ_ERR_ARG;
    }
    if (log) memset(log, 0, sizeof(*log));
    int st = MSMZ_OK;
    for (uint32_t done = 0; done < batch && st == MSMZ_OK;) {
      msmz_log plog;
      memset(&plog, 0, sizeof(plog));
      uint32_t ran = 0;
      st = run_problems(pts, d_scalars + (size_t)done * n * 8, n, batch - done, opt, out + (size_t)done * RW * 4,
                        out_inf + done, log ? &plog : nullptr, &ran);
      if (st) break;
      if (log) merge_log(log, plog, done == 0, LogMerge::SEQUENTIAL);
      done += ran;
    }
    stamp_total(log, t_begin);
    return st;
  }

  // msmz_msm_segments: problem k = scalars [first_s, first_s + n) of `sh` times base points [first_p, first_p + n) of `ph`.
  // The segments are dealt into length classes (segment_classes, multi.h); run_segments decides how each class runs, for
  // its longest segment; results go back through the permutation, logs are summed as msm_batch sums them.
  int msm_segments(uint64_t ph, uint64_t sh, const msmz_segment* segs, uint32_t n_segs, const msmz_opts* o, uint8_t* out,
                   int* out_inf, msmz_log* log) override {
    auto t_begin = std::chrono::steady_clock::now();
    if (!segs || !out || !out_inf || n_segs == 0) return MSMZ_ERR_ARG;
    const Handle *pp = handles_.get(ph, 0), *sp = handles_.get(sh, 1);
    if (!pp || !sp) return MSMZ_ERR_ARG;
    const Handle& pts = *pp;
    const Handle& sc = *sp;
    std::vector<uint64_t> lens(n_segs);
    for (uint32_t k = 0; k < n_segs; k++) {
      const msmz_segment& s = segs[k];
      if (s.n == 0 || !in_range(s.first_p, s.n, pts.n) || !in_range(s.first_s, s.n, sc.n)) return MSMZ_ERR_ARG;
      lens[k] = s.n;
    }
    msmz_opts opt;
    if (int st = resolve_opts(pts, o, &opt)) return st;
    MSMZ_HIP(hipSetDevice(device_));
    if (log) memset(log, 0, sizeof(*log));
    std::vector<uint32_t> order, starts;
    segment_classes(lens.data(), n_segs, &order, &starts);
    const bool fits32 = !(sc.n >> 32);   // the descriptors of the batched pipeline hold 32-bit offsets
    int st = MSMZ_OK;
    bool first = true;
    for (size_t ci = 0; ci + 1 < starts.size() && st == MSMZ_OK; ci++) {
      const uint32_t lo = starts[ci], hi = starts[ci + 1];
      uint64_t n_max = 0;
      for (uint32_t j = lo; j < hi; j++) n_max = lens[order[j]] > n_max ? lens[order[j]] : n_max;
      msmz_opts copt = opt;
      if (copt.glv < 0) copt.glv = pts.has_endo && planner_.default_glv(n_max, copt.reserved[1]) ? 1 : 0;   // (as msm_batch, per class)
      for (uint32_t done = lo; done < hi && st == MSMZ_OK;) {
        msmz_log plog;
        memset(&plog, 0, sizeof(plog));
        uint32_t ran = 0;
        st = run_segments(pts, sc.mem.template as<const uint32_t>(), segs, order.data() + done, hi - done, n_max, fits32, copt,
                          out, out_inf, log ? &plog : nullptr, &ran);
        if (st) break;
        if (log) merge_log(log, plog, first, LogMerge::SEQUENTIAL);
        first = false;
        done += ran;
      }
    }
    stamp_total(log, t_begin);
    return st;
  }

  // ------------------------------------------------------------------ tests (msmz_test.h; the stage hooks: test_hooks.h)
  int test_set_glv_bits(int bits) override {
    if (!Fr::HAS_GLV) return MSMZ_ERR_UNSUPPORTED;
    if (bits != 0 && (bits < 8 || bits > Fr::GLV_BITS - 1)) return MSMZ_ERR_ARG;
    planner_.k.glv_bits_assumed = bits;
    return MSMZ_OK;
  }
  int test_retries() override { return retries_; }
  int test_set_limits(uint64_t pass_entries, uint64_t batch_entries) override {
    if (pass_entries != 0 && (pass_entries < 2 || pass_entries > kMaxEntriesPerPass)) return MSMZ_ERR_ARG;
    if (batch_entries > kMaxBatchEntries) return MSMZ_ERR_ARG;
    pass_entries_ = pass_entries ? pass_entries : kMaxEntriesPerPass;
    planner_.k.batch_entries = batch_entries;
    return MSMZ_OK;
  }
  void test_passes(uint64_t* range_passes, uint64_t* sub_batches) override {
    if (range_passes) *range_passes = range_passes_;
    if (sub_batches) *sub_batches = sub_batches_;
  }
  ITestHooks* test_hooks() override { return &hooks_; }
  // msmz_test_poison: arm (or disarm) the allocations to come, and fill what every stage holds now, headroom included
  int test_poison(int pattern, uint64_t* buffers, uint64_t* bytes) override {   // (pattern: checked by msmz_test_poison)
    uint64_t nbuf = 0, nbytes = 0;
    poison_.pattern = pattern;
    if (pattern >= 0) {
      MSMZ_HIP(hipSetDevice(device_));
      hipError_t e = hipSuccess;
      each_scratch([&](DevBuf& b) {
        if (b.bytes == 0 || e != hipSuccess) return;
        e = hipMemsetAsync(b.p, pattern, b.bytes, stream_);
        nbuf++;
        nbytes += b.bytes;
      });
      MSMZ_HIP(e);
      MSMZ_HIP(hipStreamSynchronize(stream_));
    }
    if (buffers) *buffers = nbuf;
    if (bytes) *bytes = nbytes;
    return MSMZ_OK;
  }
  // msmz_test_scratch: the scratch buffers that hold memory now and their capacities (what a fill would write)
  int test_scratch(int engine, uint64_t* buffers, uint64_t* bytes) override {
    if (engine != 0) return MSMZ_ERR_ARG;
    uint64_t nbuf = 0, nbytes = 0;
    each_scratch([&](DevBuf& b) {
      if (b.bytes) nbuf++, nbytes += b.bytes;
    });
    if (buffers) *buffers = nbuf;
    if (bytes) *bytes = nbytes;
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ what only the engine calls
 private:
  // The options of an MSM over handle `h`: a precomputed set fixes c and the GLV choice (opts->c must be 0 or its c,
  // opts->glv -1 or its choice; a null opts means both defaults) and takes batched-affine buckets with the 2-D reduction.
  // reserved[1], the scalar bit bound, leaves here as the planner's (Planner::bound); a precomputed set fixes it too.
  int resolve_opts(const Handle& h, const msmz_opts* o, msmz_opts* opt) const {
    memset(opt, 0, sizeof(*opt));
    if (o) *opt = *o;
    if (opt->reserved[1] < 0 || opt->reserved[1] > 256) return MSMZ_ERR_ARG;
    opt->reserved[1] = planner_.bound(opt->reserved[1]);
    if (!h.factor) return MSMZ_OK;
    if (!o) opt->glv = -1;
    if (opt->buckets == MSMZ_BUCKETS_PROJECTIVE || opt->reserved[0] == 1) return MSMZ_ERR_UNSUPPORTED;
    if ((opt->c != 0 && opt->c != h.c) || (opt->glv >= 0 && (opt->glv != 0) != (h.glv != 0))) return MSMZ_ERR_ARG;
    if (opt->reserved[1] != 0 && opt->reserved[1] != h.sbits) return MSMZ_ERR_ARG;
    opt->c = h.c;
    opt->glv = h.glv;
    opt->reserved[1] = h.sbits;
    return MSMZ_OK;
  }

  static void stamp_total(msmz_log* log, std::chrono::steady_clock::time_point t0) {
    if (!log) return;
    log->stage_ms[MSMZ_ST_TOTAL] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }

  // What run_problems and run_segments decide from: msmBasic or batched-affine buckets, the (half-)scalars of one index
  // range pass, and how many of `candidates` problems of n entries run as ONE batched pipeline (1: the first alone).
  struct Shape {
    bool basic;
    uint64_t per_pass;
    uint32_t bs;
  };
  Shape shape(uint64_t n, uint32_t candidates, const msmz_opts& opt, const Handle& pts) const {
    const bool basic = TE || opt.buckets == MSMZ_BUCKETS_PROJECTIVE;
    const uint64_t per_pass = (opt.glv != 0 && !TE) ? pass_entries_ / 2 : pass_entries_;
    const uint32_t bs = !basic && opt.reserved[0] != 1 && n <= per_pass && candidates > 1
                            ? planner_.batch_size(n, opt, (uint32_t)pts.n, pts.factor, candidates)
                            : 1;
    return {basic, per_pass, bs};
  }

  // How a shape runs is decided here.  Up to `remaining` problems over device scalars; *ran = how many it ran.
  //  - one batched pipeline over a sub-batch of them (planner_.batch_size): Weierstrass batched-affine buckets with the
  //    2-D reduction, n within one sort pass, and a sub-batch plan the two-level sort takes -- a plan that falls off it
  //    (also only after the GLV retry) runs the first problem alone and the rest is decided again;
  //  - else the first problem alone over consecutive index ranges of at most one sort pass (2^24 entries; 2^23 points
  //    with GLV) whose partial sums are folded on the host -- the same additivity the multi-GPU split uses -- each range
  //    with batched-affine buckets (Weierstrass) or msmBasic (projective buckets, twisted Edwards).
  // first_p (a segment run alone, remaining = 1): the problem's points start at record first_p of the set.
  int run_problems(const Handle& pts, const uint32_t* d_scalars, uint64_t n, uint32_t remaining, const msmz_opts& opt,
                   uint8_t* out, int* out_inf, msmz_log* log, uint32_t* ran, uint64_t first_p = 0) {
    const Shape sh = shape(n, remaining, opt, pts);
    *ran = 1;
    if (sh.bs > 1) {
      Redo redo = Redo::NONE;   // (a GLV half longer than assumed: the whole sub-batch again)
      const int st = glv_retry(&redo, [&](int extra_bits, Redo* r) {
        return msm_weierstrass_affine(pts, pts.mem.template as<const uint32_t>(), d_scalars, n, opt, out, out_inf, log,
                                      extra_bits, sh.bs, r);
      });
      if (st || redo != Redo::PER_PROBLEM) {
        if (!st) sub_batches_++;
        *ran = sh.bs;
        return st;
      }
    }
    uint8_t part[RW * 4];
    int st = MSMZ_OK;
    for (uint64_t done = 0; done < n && st == MSMZ_OK; done += sh.per_pass) {
      const uint64_t cnt = n - done < sh.per_pass ? n - done : sh.per_pass;
      range_passes_++;
      const uint32_t* d_points = pts.mem.template as<const uint32_t>() + (first_p + done) * PW_WORDS;
      const uint32_t* d_sc = d_scalars + done * 8;
      int pinf = 0;
      msmz_log plog;
      msmz_log* lp = log ? &plog : nullptr;
      if (lp) memset(lp, 0, sizeof(*lp));
      uint8_t* o = done == 0 ? out : part;
      int* oi = done == 0 ? out_inf : &pinf;
      if (sh.basic) {
        st = msm_basic(pts, d_points, d_sc, cnt, opt, o, oi, lp);
      } else {
        Redo redo = Redo::NONE;
        st = glv_retry(&redo, [&](int extra_bits, Redo* r) {
          return msm_weierstrass_affine(pts, d_points, d_sc, cnt, opt, o, oi, lp, extra_bits, 1, r);
        });
      }
      if (st) break;
      if (done > 0) st = fold_partial(curve_id_, RW * 4, out, out_inf, part, pinf);
      if (log) merge_log(log, plog, done == 0, LogMerge::SEQUENTIAL);
    }
    return st;
  }

  // The next segments of one length class (order[0 .. remaining): indices into segs; n_max: the class's longest): the
  // decision of run_problems, taken for n_max.  Either a sub-batch of them in ONE batched pipeline planned for n_max, the
  // kernels reading each problem's offsets and length from a descriptor table (SegDesc; filled from pinned memory in
  // stream order, no host wait) -- or the first segment alone through the range loop of run_problems, the base pointers
  // advanced to it.  Results go to out / out_inf at the segments' own indices.  batchable: the offsets fit the table.
  int run_segments(const Handle& pts, const uint32_t* d_scalars, const msmz_segment* segs, const uint32_t* order,
                   uint32_t remaining, uint64_t n_max, bool batchable, const msmz_opts& opt, uint8_t* out, int* out_inf,
                   msmz_log* log, uint32_t* ran) {
    const uint32_t most = remaining < kMaxSegProblems ? remaining : kMaxSegProblems;
    const uint32_t bs = shape(n_max, batchable ? most : 1, opt, pts).bs;
    *ran = 1;
    if (bs > 1) {
      int st;
      if ((st = h_segs_.ensure((size_t)bs * sizeof(SegDesc))) || (st = segs_.ensure((size_t)bs * sizeof(SegDesc)))) return st;
      for (uint32_t p = 0; p < bs; p++) {
        const msmz_segment& s = segs[order[p]];
        h_segs_.template as<SegDesc>()[p] = SegDesc{(uint32_t)s.first_s, (uint32_t)s.first_p, (uint32_t)s.n};
      }
      MSMZ_HIP(hipMemcpyAsync(segs_.p, h_segs_.p, (size_t)bs * sizeof(SegDesc), hipMemcpyHostToDevice, stream_));
      std::vector<uint8_t> res((size_t)bs * RW * 4);
      std::vector<int> inf(bs, 0);
      Redo redo = Redo::NONE;
      st = glv_retry(&redo, [&](int extra_bits, Redo* r) {
        return msm_weierstrass_affine(pts, pts.mem.template as<const uint32_t>(), d_scalars, n_max, opt, res.data(),
                                      inf.data(), log, extra_bits, bs, r, segs_.as<const SegDesc>());
      });
      if (st || redo != Redo::PER_PROBLEM) {
        if (!st) {
          sub_batches_++;
          for (uint32_t p = 0; p < bs; p++) {
            memcpy(out + (size_t)order[p] * RW * 4, res.data() + (size_t)p * RW * 4, RW * 4);
            out_inf[order[p]] = inf[p];
          }
        }
        *ran = bs;
        return st;
      }
    }
    const msmz_segment& s = segs[order[0]];
    uint32_t one = 0;
    return run_problems(pts, d_scalars + s.first_s * 8, s.n, 1, opt, out + (size_t)order[0] * RW * 4, out_inf + order[0], log,
                        &one, s.first_p);
  }
  static constexpr uint32_t kMaxSegProblems = 32768;   // problems of one pipeline = gridDim.y of the sort kernels

  // attempt(extra_bits, &redo): a GLV half longer than the assumed 127 bits (k_hist flags it) redoes the MSM with
  // windows for the PROVEN bound (Fr::GLV_PROVEN_BITS, tools/gen_constants.py), which no half can exceed -- a second
  // flag is an internal error.  *redo: what the last attempt asks beyond that (Redo::PER_PROBLEM).
  template <class Attempt>
  int glv_retry(Redo* redo, Attempt attempt) {
    int st = attempt(0, redo);
    if (*redo != Redo::PROVEN_BITS) return st;
    retries_++;
    *redo = Redo::NONE;
    st = attempt(1, redo);
    return *redo == Redo::PROVEN_BITS ? MSMZ_ERR_ARG : st;
  }

  // f(buffer) for every scratch buffer of the engine: the resident-set operations', the stages' and the pipeline's own
  template <class Fn>
  void each_scratch(Fn f) {
    Base::each_scratch(f);
    sort_.each_scratch(f);
    reduce_.each_scratch(f);
    f(desc_), f(bfin_), f(rscan_), f(partials_), f(slots_), f(segs_);
  }

  // ------------------------------------------------------------------------------------------ shared phases
  Run new_run(const msmz_opts& opt) const {
    Run run;
    run.timing = opt.timing != 0;
    run.ev = ev_;
    return run;
  }
  void mark(const Run& run, hipEvent_t e) { run.mark(e, stream_); }
  static float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
  }

  // read the device-side totals (one host round trip)
  int fetch_meta(Run& run) {
    MSMZ_HIP(hipMemcpyAsync(h_meta_.p, meta_.p, sizeof(MsmMeta), hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    run.max_bucket = h_meta_->max_bucket;
    run.n_entries = h_meta_->n_entries;
    run.rounds = h_meta_->rounds;
    memcpy(run.round_pairs, h_meta_->round_pairs, sizeof(run.round_pairs));
    memcpy(run.round_base, h_meta_->round_base, sizeof(run.round_base));
    return MSMZ_OK;
  }

  // copy the window results of all pl.nprob problems (the C entries of the last level; its rows are multiples of the
  // weight unit and not needed) to h_res_, and the meta block to the host
  int fetch_window_sums(const Plan& pl, size_t per_problem) {
    const size_t words = pl.nprob * per_problem * XW;
    if (int st = h_res_.ensure(words * 4)) return st;
    MSMZ_HIP(hipGetLastError());
    MSMZ_HIP(hipMemcpyAsync(h_res_.p, reduce_.final(), words * 4, hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipMemcpyAsync(h_meta_.p, meta_.p, sizeof(MsmMeta), hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    return MSMZ_OK;
  }

  // twisted Edwards as a host group of host_horner (fp.h limbs)
  struct HostTe {
    using Pt = TeExt<F>;
    void set_inf(Pt& p) const { te_set_zero(p); }
    void dbl(Pt& r, const Pt& p) const { te_add(r, p, p); }
    void add_pt(Pt& r, const Pt& a, const Pt& b) const { te_add(r, a, b); }
    void load_pt(Pt& p, const uint32_t* w) const {
      fe_unpack<F>(p.X, w);
      fe_unpack<F>(p.Y, w + NW);
      fe_unpack<F>(p.Z, w + 2 * NW);
      fe_unpack<F>(p.T, w + 3 * NW);
    }
  };

  // The end of every MSM, after its bucket reduction: fetch the window results (two_d: two per bucket set, else one),
  // combine each problem's on the host (msm-batched-affine.ts:300-322) and fill the log.
  int finish_msm(const Plan& pl, Run& run, bool two_d, uint8_t* out, int* out_inf, msmz_log* log) {
    mark(run, run.ev.red_end);
    const size_t per_problem = (size_t)(two_d ? 2 : 1) * pl.Keff;
    // (the terms are listed while the device still reduces)
    const std::vector<WindowTerm> terms =
        window_terms(pl.c, pl.K, pl.Keff, (int)pl.F, two_d ? planner_.split_2d(pl).b : -1, pl.fold_shift != 0);
    int st = fetch_window_sums(pl, per_problem);
    if (st) return st;
    const auto t_host = std::chrono::steady_clock::now();
    if (h_meta_->error & 1u) return MSMZ_ERR_DEGENERATE;
    for (uint32_t p = 0; p < pl.nprob; p++) {
      const uint32_t* rp = h_res_.template as<const uint32_t>() + p * per_problem * XW;
      uint32_t w[RW];
      if constexpr (TE) {
        te_to_affine_canon<F>(w, host_horner(HostTe{}, terms, rp, XW));
        out_inf[p] = 0;
      } else {
        // ~K*c dependent doublings: on 64-bit limbs (host64.h), ~4x faster on a CPU core than the kernels' limb code
        Xyzz<F> fin;
        host64_.to_xyzz(fin, host_horner(host64_, terms, rp, XW));
        out_inf[p] = xyzz_to_affine_canon<F>(w, fin) ? 1 : 0;
      }
      memcpy(out + (size_t)p * RW * 4, w, sizeof(w));
    }
    const float host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_host).count();
    fill_log(log, pl, run, host_ms);
    return MSMZ_OK;
  }

  // the log of one MSM (or sub-batch): its plan, its run's totals and (timed) its stage events.  scatter_kernel_ms: the
  // scatter kernel alone (k_coarse / k_scatter), without k_fine.
  static void fill_log(msmz_log* log, const Plan& pl, const Run& run, float host_ms) {
    if (!log) return;
    log->c = pl.c;
    log->K = pl.K;
    log->rounds = (int)run.rounds;
    log->glv = pl.glv ? 1 : 0;
    log->n_entries = run.n_entries;
    log->n_pairs = run.n_pairs;
    log->max_bucket = run.max_bucket;
    log->stage_ms[MSMZ_ST_FINAL] = host_ms;
    if (!run.timing) return;
    const StageEvents& ev = run.ev;
    log->stage_ms[MSMZ_ST_DIGITS] = elapsed(ev.sort0, ev.hist_end);
    log->stage_ms[MSMZ_ST_SCAN] = elapsed(ev.hist_end, ev.scan_end);
    log->stage_ms[MSMZ_ST_SCATTER] = elapsed(ev.scan_end, ev.sort_end);
    log->scatter_kernel_ms = elapsed(ev.scan_end, ev.coarse_end);
    log->scatter_launches = 1;
    log->stage_ms[MSMZ_ST_PLAN] = elapsed(ev.plan0, ev.plan_end);
    log->stage_ms[MSMZ_ST_ACCUMULATE] = elapsed(ev.plan_end, ev.acc_end);
    log->stage_ms[MSMZ_ST_REDUCE] = elapsed(ev.acc_end, ev.red_end);
    hipEvent_t prev = ev.plan_end;
    for (uint32_t r = 0; r < run.rounds && r < 32; r++) {
      if (run.round_pairs[r] == 0) continue;
      log->batch_add_ms[r] = elapsed(prev, ev.round_end[r]);
      prev = ev.round_end[r];
    }
  }

  // The schedule of the tree rounds (plan_kernels.h) for the sorted buckets d_off / d_refs (nb of them, all problems'),
  // cut into workgroups as pc says: desc_ <- one descriptor per addition of every round (room for desc_records), bfin_ <-
  // what the rounds leave of each bucket, meta <- rounds, entries, round sizes and bases.  Reads meta->max_bucket, which
  // the sort left.  No host round trip.
  int plan_phase(const PlanChunks& pc, const uint32_t* d_off, const uint32_t* d_refs, uint32_t nb, int tail_skip,
                 size_t desc_records, Run& run) {
    int st;
    MsmMeta* d_meta = meta_.template as<MsmMeta>();
    mark(run, run.ev.plan0);
    const uint32_t n_chunks = pc.n_main + (nb - pc.nb_main + pc.chunk_top - 1) / pc.chunk_top;
    // chunk totals per round, then the per-workgroup scratch of the rounds beyond PLAN_RL
    const size_t pair_words = (size_t)n_chunks * (PLAN_RMAX - PLAN_RL) * PLAN_T;
    if ((st = rscan_.ensure(((size_t)PLAN_RMAX * n_chunks + pair_words) * 4 + kTraceBytes * n_chunks))) return st;
    if ((st = desc_.ensure(desc_records * 8))) return st;
    if ((st = bfin_.ensure((size_t)nb * 16))) return st;
    hipLaunchKernelGGL(k_plan_count, dim3(n_chunks), dim3(PLAN_T), 0, stream_, rscan_.as<uint32_t>(), d_off, nb,
                       n_chunks, d_meta, tail_skip, pc);
    hipLaunchKernelGGL(k_plan_emit, dim3(n_chunks), dim3(PLAN_T), 0, stream_, desc_.as<uint2>(), bfin_.as<uint4>(),
                       d_meta, rscan_.as<uint32_t>(), d_off, d_refs, nb, n_chunks, tail_skip, rscan_.as<uint32_t>() + (size_t)PLAN_RMAX * n_chunks, pc);
    MSMZ_HIP(hipGetLastError());
#ifdef MSMZ_TRACE
    if ((st = trace_dump(stream_, "k_plan_emit", rscan_.as<uint32_t>() + (size_t)PLAN_RMAX * n_chunks + pair_words, n_chunks, false))) return st;
#endif
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ Weierstrass, affine buckets
  // nprob > 1: a batched MSM of nprob problems over the same points (scalars of problem p at d_scalars + p n 8, results
  // at out + p 2 FE_BYTES / out_inf[p]): one sort, one plan, one train of tree rounds and one two-dimensional reduction
  // over nprob * Keff bucket sets.  *redo: Redo::PER_PROBLEM when this plan does not batch (the two-level sort only),
  // Redo::PROVEN_BITS when a GLV half is longer than the windows were sized for (glv_retry).
  // d_segs (run_segments): the nprob problems are segments of the scalar and point sets; n64 is the longest, d_points and
  // d_scalars the sets' starts.  Only the sort reads the table: what follows sees one dense sort, as for a batch.
  int msm_weierstrass_affine(const Handle& pts, const uint32_t* d_points, const uint32_t* d_scalars, uint64_t n64,
                             const msmz_opts& opt, uint8_t* out, int* out_inf, msmz_log* log, int extra_bits,
                             uint32_t nprob, Redo* redo, const SegDesc* d_segs = nullptr) {
    const bool glv = opt.glv != 0;
    if (glv && (!Fr::HAS_GLV || !pts.has_endo)) return MSMZ_ERR_UNSUPPORTED;
    Plan pl;
    const bool want_2d = opt.reserved[0] != 1;   // else reduceAffine: the batched-affine first level (reduce_affine.h)
    // precomputed point set: its copies carry windows [j F, (j + 1) F) into one bucket set (two-level sort, 2-D reduction)
    const uint32_t fac = pts.factor > 1 ? pts.factor : 1;
    if (fac > 1 && (!want_2d || glv != (pts.glv != 0))) return MSMZ_ERR_UNSUPPORTED;
    int st = planner_.make_plan(pl, n64, glv, opt, (uint32_t)pts.n, true, extra_bits, want_2d, nprob, fac);
    if (st) return st;
    const SortLayout sl = planner_.sort_layout(pl);
    if (fac > 1 && !sl.two_level) return MSMZ_ERR_ARG;   // (msmz_precompute_points refuses such sets)
    if (nprob > 1 && (!want_2d || !sl.two_level)) {
      *redo = Redo::PER_PROBLEM;
      return MSMZ_OK;
    }
    // location words hold a record index in 30 bits
    if ((uint64_t)nprob * pl.K * pl.M >= (1ull << 30)) return MSMZ_ERR_ARG;
    // whole groups of 64 records; + the records of the batched-affine first reduction level when it is selected
    const size_t f2_records = opt.reserved[0] == 1 ? (size_t)13 * pl.Keff * ((pl.L + 1) / 2) + 256 : 0;
    if ((st = slots_.ensure(((size_t)nprob * pl.K * pl.M + 64 + f2_records) * SlotFmt<F>::WORDS * 4))) return st;
    Run run = new_run(opt);
    MsmMeta* d_meta = meta_.template as<MsmMeta>();
    if ((st = sort_.run(pl, sl, d_scalars, run, stream_, d_meta, (uint32_t)pts.copy_stride, d_segs))) return st;
    const uint32_t nb = pl.nb * nprob;   // buckets of all problems

    // ---- plan: descriptors of every pair of every round + what is left of each bucket (plan_kernels.h)
    // the batched-affine first reduction level (opt.reserved[0] = 1) wants ONE sum per bucket: no rounds skipped
    const int tail_skip = want_2d ? tail_skip_2d_ : 0;
    if ((st = plan_phase(planner_.plan_chunks(pl), sort_.off(), sort_.refs(), nb, tail_skip, (size_t)nprob * pl.K * pl.M, run))) return st;
    if ((st = fetch_meta(run))) return st;      // the ONE host round trip before the final fetch
    if (h_meta_->error & 4u) return MSMZ_ERR_RANGE;
    if (h_meta_->error & 2u) {
      *redo = Redo::PROVEN_BITS;
      return MSMZ_OK;
    }
    // (a plain set's bucket holds <= M <= 2^24 entries; a precomputed set's up to W M < 2^PLAN_RMAX, which pre_fits checked)
    if (run.max_bucket > (pl.F > 1 ? (1u << PLAN_RMAX) - 1u : (1u << 24))) return MSMZ_ERR_ARG;
    mark(run, run.ev.plan_end);
    const uint32_t R = run.rounds;
    for (uint32_t r = 0; r < R; r++) run.n_pairs += run.round_pairs[r];
    const BatchAdder<Cfg> adder = batch_adder();   // (slots_ has its final size: nothing below grows it)
    for (uint32_t r = 0; r < R; r++) {
      const uint32_t pairs = run.round_pairs[r];
      if (pairs == 0) continue;
      adder.launch(pairs, opt.safe != 0, d_points, desc_.as<uint2>() + run.round_base[r], run.round_base[r], d_meta);
#ifdef MSMZ_TRACE
      {
        char nm[32];
        snprintf(nm, sizeof nm, "k_batch_add round %d", r);
        const int B = adder.batch_b(pairs);
        const uint32_t wgs = (pairs + MSMZ_BATCH_T * B - 1) / (MSMZ_BATCH_T * B);
        if ((st = trace_dump(stream_, nm, d_meta + 1, wgs < 65536 ? wgs : 65536, false))) return st;
      }
#endif
      mark(run, run.ev.round_end[r]);
    }
    mark(run, run.ev.acc_end);

    // ---- bucket reduction (reduce.h)
    const BucketSource buckets = BucketSource::locations(slots_.as<uint32_t>(), d_points, bfin_.as<uint4>());
    if (want_2d) {
      // two-dimensional: row / column sums of the buckets, then two half-length weighted sums per bucket set
      if ((st = reduce_.run_2d(planner_.r2_geom(pl), reduce_knobs_, buckets, stream_))) return st;
    } else {
      // level 1 from affine bucket sums, then XYZZ levels down to one entry per window.  The weight-L bucket is folded
      // into element L/2, which must be the FIRST element of its group
      uint32_t S1 = planner_.first_group_size(pl);
      if (S1 > 8) S1 = 8;
      while (S1 > 1 && S1 * 2 > pl.L) S1 >>= 1;
      const uint32_t groups = (pl.L + S1 - 1) / S1;   // elements are weights 0..L-1 (weight L folded into L/2)
      if ((st = reduce_.first_affine(pl, S1, groups, run.n_pairs, adder, slots_.bytes, buckets, d_meta))) return st;
      if ((st = reduce_.levels(reduce_knobs_, groups, (uint32_t)pl.Keff, stream_))) return st;
    }
    return finish_msm(pl, run, want_2d, out, out_inf, log);
  }

  // ------------------------------------------------------------------------------------------ msmBasic: projective / extended buckets
  // (msm-basic.ts:45-176; Weierstrass "projective fallback" parallel.ts:69-87 and the twisted-Edwards MSM)
  int msm_basic(const Handle& pts, const uint32_t* d_points, const uint32_t* d_scalars, uint64_t n64, const msmz_opts& opt,
                uint8_t* out, int* out_inf, msmz_log* log) {
    using P = typename Cfg::P;
    // neither msmProjective (parallel.ts:69-87) nor the twisted-Edwards path (msm-basic.ts:4) uses the endomorphism
    if (opt.glv) return MSMZ_ERR_UNSUPPORTED;
    Plan pl;
    int st = planner_.make_plan(pl, n64, false, opt, (uint32_t)pts.n, false);
    if (st) return st;
    Run run = new_run(opt);
    MsmMeta* d_meta = meta_.template as<MsmMeta>();
    if ((st = sort_.run(pl, planner_.sort_layout(pl), d_scalars, run, stream_, d_meta, 0)) || (st = fetch_meta(run))) return st;
    if (h_meta_->error & 4u) return MSMZ_ERR_RANGE;
    run.n_pairs = run.n_entries;   // (no tree rounds: every entry is added into its chunk's accumulator)
    constexpr int AW = P::ACC_WORDS;
    const uint32_t nb = pl.nb;
    mark(run, run.ev.plan0);
    // chunk offsets: cscan[g] = sum_{g' < g} ceil(size / 2^chunk_shift); chunks of 64 entries unless some bucket is
    // very long (then ~sqrt of it: bounds both the chunk and the number of partial sums one reduction thread adds)
    int chunk_shift = chunk_shift_override_ > 0 ? chunk_shift_override_ : ACC_CHUNK_SHIFT;
    while ((1ull << (2 * chunk_shift)) < run.max_bucket) chunk_shift++;
    if ((st = rscan_.ensure(((size_t)nb + 1) * 4))) return st;
    if ((st = scan_exclusive(stream_, partials_, rscan_.as<uint32_t>(), sort_.off(), nb, chunk_shift, d_meta->round_pairs,
                             nullptr)))
      return st;
    MSMZ_HIP(hipMemcpyAsync(h_meta_.p, d_meta, sizeof(MsmMeta), hipMemcpyDeviceToHost, stream_));
    MSMZ_HIP(hipStreamSynchronize(stream_));
    const uint32_t n_chunks = h_meta_->round_pairs[0];
    mark(run, run.ev.plan_end);
    if ((st = slots_.ensure((size_t)(n_chunks + 1) * AW * 4))) return st;
    if (n_chunks > 0) {
      hipLaunchKernelGGL((k_bucket_accumulate<P>), dim3((n_chunks + 127) / 128), dim3(128), 0, stream_,
                         slots_.as<uint32_t>(), d_points, sort_.refs(), sort_.off(), rscan_.as<uint32_t>(), nb,
                         n_chunks, chunk_shift);
    }
    mark(run, run.ev.acc_end);
    // every bucket is visited twice: buckets of several chunk accumulators (large inputs: Pallas 2^22 has 4,
    // ed-on-bls12-377 2^24 has 8) are first summed into one accumulator each, in bucket order
    const bool summed = (uint64_t)n_chunks * 2 > (uint64_t)nb * 3 && !no_bucket_sums_;
    BucketSource buckets = BucketSource::chunks(slots_.as<uint32_t>(), rscan_.as<uint32_t>());
    if (summed && (st = reduce_.bucket_sums(buckets, nb, stream_, &buckets))) return st;
    if ((st = reduce_.run_2d(planner_.r2_geom(pl), reduce_knobs_, buckets, stream_))) return st;
    return finish_msm(pl, run, true, out, out_inf, log);
  }
  // the launcher of batched-affine additions into slots_ as it is now (batch_add.h)
  BatchAdder<Cfg> batch_adder() const { return {stream_, slots_.template as<uint32_t>(), batch_min_wgs_, batch_b_override_}; }

  // shared state -------------------------------------------------------------------------------
  int curve_id_;
  StageEvents ev_{};
  // Tuning knobs (the planning ones: PlanKnobs, plan.h; which kernel a reduction level runs: ReduceKnobs, reduce.h), each
  // through env_int (plan.h).  None of them changes a result.
  uint32_t batch_min_wgs_ = (uint32_t)env_int("MSMZ_BATCH_WGS", 512);
  int chunk_shift_override_ = env_int("MSMZ_CHUNK_SHIFT", 0);
  const ReduceKnobs reduce_knobs_{};
  Host64<F> host64_;
  bool no_bucket_sums_ = env_int("MSMZ_NO_BUCKET_SUMS", 0) != 0;
  // rounds left to the 2-D reduction's loader: at most 2 (a bucket's final-location record holds 4 partial sums)
  int tail_skip_2d_ = env_int("MSMZ_TAIL_SKIP_2D", 1) > 2 ? 2 : env_int("MSMZ_TAIL_SKIP_2D", 1);
  int batch_b_override_ = env_int("MSMZ_BATCH_B", 0);
  int retries_ = 0;            // MSMs redone with the proven GLV bound (test hook reads it)
  // (half-)scalars one index-range pass of run_problems takes: kMaxEntriesPerPass unless msmz_test_set_limits lowered
  // it (the capacity checks keep the constant); what msmz_test_passes reports
  uint64_t pass_entries_ = kMaxEntriesPerPass;
  uint64_t range_passes_ = 0, sub_batches_ = 0;
  // window sizes, geometry, sort layout (plan.h), PlanKnobs in declaration order
  Planner<Fr> planner_{{env_int("MSMZ_NO_SPREAD", 0) != 0, env_int("MSMZ_NO_FOLD", 0) != 0,
                        env_int("MSMZ_NO_WINDOW_MODEL", 0) != 0, env_int("MSMZ_ATOMIC_SORT", 0) != 0,
                        env_int("MSMZ_NO_FBT", 0) != 0, env_int("MSMZ_NO_PLAN_TOP", 0) != 0,
                        env_int("MSMZ_NO_SORT_SPECIAL", 0) != 0, env_int("MSMZ_FB", 0), (uint32_t)env_int("MSMZ_S1", 0),
                        (uint32_t)env_int("MSMZ_R2_NC", 0)}};
  BucketSort<Fr, TE> sort_;   // the sort stage: its buffers, the sorted references and bucket offsets included
  BucketReduce<Cfg> reduce_;  // the bucket reduction: its level buffers and the window results included
  // what the stages share: the tree rounds' descriptors and final locations, the plan's / msmBasic's chunk scan (and its
  // scratch partials_), the slot records (msmBasic: chunk accumulators)
  DevBuf desc_, bfin_, rscan_, partials_, slots_;
  DevBuf segs_;         // run_segments: the descriptor table of a sub-batch ...
  PinnedBuf h_segs_;    // ... and its pinned host copy (rewritten only after the sub-batch's final fetch)
  TestHooks<Cfg> hooks_{*this};
};

}  // namespace msmz

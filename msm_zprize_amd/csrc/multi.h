// Multi-GPU context: one engine + one HIP stream + one host thread per device, inputs split over the
// devices, partial sums folded on the host.  This is what replaces the reference's worker pool
// (src/threads/threads.ts:132-359: startThreads(n) spawns n-1 workers that run the same msm body on
// their share of the work, src/parallel.ts:291-315) -- here startThreads(n) -> msmz_create(..., n_devices = n).
//
// Input split (MSM is additive over disjoint index sets): contiguous blocks of
// 2^MULTI_BLOCK_SHIFT entries are dealt round-robin, entry i lives on device (i >> shift) % G at local index
// ((i >> shift) / G << shift) | (i & mask).  Unlike one contiguous range per device this does not depend on the
// size of the set, so (1) a point set and a scalar set of different lengths are split consistently and (2) the
// first n entries of a set are a PREFIX of every device's local array -- msm(scalars, points, n) with
// n <= allocated (msm-batched-affine.ts:74-97; the warm-up of scripts/msm-weierstrass.ts:24) needs no data
// movement.  No inter-GPU traffic during an MSM; the G affine partial sums are added with msmz_point_add.
#pragma once
#include <condition_variable>
#include <cstring>
#include <map>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/msmz.h"
#include "constants_gen.h"
#include "fr.h"
#include "iengine.h"
#include "ranges.h"

namespace msmz {

// The checks of msmz_scalars_expr that need no handle, for the multi-device context: what expr_compile (expr_kernels.h)
// refuses, in its order -- that header is device code and cannot be included here, half way through kernels.h.
// named[c] = 0: no factor reads column c, 1: at rotation 0 only, 3: rotated; *rotated: some factor is.
static inline int expr_precheck(const msmz_expr& e, uint8_t named[MSMZ_EXPR_MAX_COLUMNS], bool* rotated) {
  if (!e.columns || !e.terms || e.n_columns < 1 || e.n_columns > (uint32_t)MSMZ_EXPR_MAX_COLUMNS || e.n_terms < 1 ||
      e.n_terms > (uint32_t)MSMZ_EXPR_MAX_TERMS || e.n == 0 || e.n >> 32 || e.flags)
    return MSMZ_ERR_ARG;
  memset(named, 0, MSMZ_EXPR_MAX_COLUMNS);
  std::vector<uint64_t> operands;   // (column << 32 | rot mod n), distinct
  for (uint32_t k = 0; k < e.n_terms; k++) {
    const msmz_expr_term& t = e.terms[k];
    if (t.reserved || t.n_factors > (uint32_t)MSMZ_EXPR_MAX_DEGREE || (t.n_factors && !t.factors)) return MSMZ_ERR_ARG;
    for (uint32_t f = 0; f < t.n_factors; f++) {
      const uint32_t col = t.factors[f].column;
      if (col >= e.n_columns) return MSMZ_ERR_ARG;
      int64_t r = (int64_t)t.factors[f].rot % (int64_t)e.n;
      if (r < 0) r += (int64_t)e.n;
      named[col] |= r ? 3 : 1;
      if (r) *rotated = true;
      const uint64_t key = (uint64_t)col << 32 | (uint64_t)r;
      bool seen = false;
      for (uint64_t o : operands) seen = seen || o == key;
      if (!seen) operands.push_back(key);
      if (operands.size() > (size_t)MSMZ_EXPR_MAX_OPERANDS) return MSMZ_ERR_ARG;
    }
  }
  return MSMZ_OK;
}

// Problems per sub-batch of a batched MSM: at most `cap` entries (problems x entries_per_problem) per sub-batch, and the
// `remaining` problems dealt into equally large sub-batches (64 problems with room for 40 -> 2 x 32, not 40 + 24).
static inline uint32_t batch_split(uint32_t remaining, uint64_t entries_per_problem, uint64_t cap) {
  if (remaining == 0) return 0;
  uint64_t fit = entries_per_problem ? cap / entries_per_problem : remaining;
  if (fit < 1) fit = 1;
  if (fit >= remaining) return remaining;
  const uint64_t parts = (remaining + fit - 1) / fit;
  return (uint32_t)((remaining + parts - 1) / parts);
}

// Length classes of a segmented MSM (msmz_msm_segments): segments whose lengths have the same floor(log2 n) -- within 2x
// of each other, which bounds what sizing one pipeline for the longest wastes on the shortest.  order: the segment indices
// class after class (shortest class first), caller order kept inside a class; starts: class i = order[starts[i] ..
// starts[i + 1]).  Lengths are >= 1.
static inline void segment_classes(const uint64_t* n, uint32_t count, std::vector<uint32_t>* order,
                                   std::vector<uint32_t>* starts) {
  auto bits = [](uint64_t x) {
    int b = 0;
    while (x >>= 1) b++;
    return b;
  };
  uint32_t per[65] = {};
  for (uint32_t k = 0; k < count; k++) per[bits(n[k]) + 1]++;
  starts->clear();
  for (int b = 0; b < 64; b++) {
    if (per[b + 1]) starts->push_back(per[b]);
    per[b + 1] += per[b];   // -> first position of class b + 1; per[b] is class b's
  }
  starts->push_back(count);
  order->assign(count, 0);
  for (uint32_t k = 0; k < count; k++) (*order)[per[bits(n[k])]++] = k;
}

// acc = acc + part mod the group order of curve `curve_id` (8 words each, below q): the per-device sums of a dot product
static inline int fold_scalar(int curve_id, uint32_t* acc, const uint32_t* part) {
  switch (curve_id) {
    case MSMZ_BLS12_377_G1: fr_add<Bls377Fr>(acc, acc, part); return MSMZ_OK;
    case MSMZ_PALLAS: fr_add<PallasFr>(acc, acc, part); return MSMZ_OK;
    case MSMZ_BLS12_381_G1: fr_add<Bls381Fr>(acc, acc, part); return MSMZ_OK;
    case MSMZ_ED_ON_BLS12_377: fr_add<Ed377Fr>(acc, acc, part); return MSMZ_OK;
    default: return MSMZ_ERR_UNSUPPORTED;
  }
}

// entries of the first n that live on shard g of G
static inline uint64_t shard_count(uint64_t n, uint32_t g, uint32_t G, int shift = MULTI_BLOCK_SHIFT) {
  const uint64_t blk = 1ull << shift, cycle = blk * G;
  const uint64_t full = n / cycle, rem = n % cycle;
  uint64_t extra = rem > (uint64_t)g * blk ? rem - (uint64_t)g * blk : 0;
  if (extra > blk) extra = blk;
  return full * blk + extra;
}

// acc += part for partial MSM results of `rec` bytes (canonical affine x | y) and their infinity flags: the reference's
// "partition sum" on the main thread (msm-batched-affine.ts:300-307).  Index ranges of one engine, devices of a context.
static inline int fold_partial(int curve_id, size_t rec, uint8_t* acc, int* acc_inf, const uint8_t* part, int part_inf) {
  uint8_t a[2 * 48];
  memcpy(a, acc, rec);
  return msmz_point_add(curve_id, *acc_inf ? nullptr : a, *acc_inf, part_inf ? nullptr : part, part_inf, acc, acc_inf);
}

// total += part for the logs of parts of one call.  SEQUENTIAL: the parts ran one after another (index ranges,
// sub-batches), their times add; PARALLEL: side by side (devices), the slowest part's times count.  Counts add in both,
// max_bucket and rounds take the maximum.  first: total = part.  c, K and GLV: the first sequential part's, the last
// parallel one's.
enum class LogMerge { SEQUENTIAL, PARALLEL };
static inline void merge_log(msmz_log* total, const msmz_log& part, bool first, LogMerge mode) {
  if (first) {
    *total = part;
    return;
  }
  auto time = [mode](float& t, float p) { t = mode == LogMerge::SEQUENTIAL ? t + p : (p > t ? p : t); };
  for (int i = 0; i < MSMZ_N_STAGES; i++) time(total->stage_ms[i], part.stage_ms[i]);
  for (int i = 0; i < 32; i++) time(total->batch_add_ms[i], part.batch_add_ms[i]);
  time(total->scatter_kernel_ms, part.scatter_kernel_ms);
  total->n_entries += part.n_entries;
  total->n_pairs += part.n_pairs;
  total->scatter_launches += part.scatter_launches;
  if (part.max_bucket > total->max_bucket) total->max_bucket = part.max_bucket;
  if (part.rounds > total->rounds) total->rounds = part.rounds;
  if (mode == LogMerge::PARALLEL) {
    total->c = part.c;
    total->K = part.K;
    total->glv = part.glv;
  }
}

class MultiEngine : public IEngine {
 public:
  // takes ownership of the engines (already initialised, one per device id; ids may repeat)
  MultiEngine(int curve_id, int fe_bytes, std::vector<IEngine*> engines)
      : curve_id_(curve_id), fb_(fe_bytes), G_((uint32_t)engines.size()) {
    for (IEngine* e : engines) workers_.push_back(new Worker(e));
  }
  ~MultiEngine() override {
    for (Worker* w : workers_) delete w;
  }

  int upload_points(const uint8_t* xy, const uint8_t* inf, uint64_t n, uint64_t* h, const GenMap* = nullptr) override {
    if (!xy || !h || n == 0) return MSMZ_ERR_ARG;
    return make_set(0, n, h, [&](uint32_t g, IEngine* e, uint64_t cnt, uint64_t* sub) {
      // every device copies its own blocks straight out of the caller's buffer (no gathered host copy)
      const GenMap split{G_, g, MULTI_BLOCK_SHIFT};
      return e->upload_points(xy, inf, cnt, sub, &split);
    });
  }

  int upload_scalars(const uint8_t* s, uint64_t n, uint64_t* h, const GenMap* = nullptr) override {
    if (!s || !h || n == 0) return MSMZ_ERR_ARG;
    return make_set(1, n, h, [&](uint32_t g, IEngine* e, uint64_t cnt, uint64_t* sub) {
      const GenMap split{G_, g, MULTI_BLOCK_SHIFT};
      return e->upload_scalars(s, cnt, sub, &split);
    });
  }

  // Correctness first: the source, wherever it is, becomes a packed host copy (made by the first engine), and every
  // device imports its own blocks of it like an upload.  A device source gains nothing here.
  int import_scalars(const msmz_src& s, uint64_t n, uint64_t* h, const GenMap* = nullptr) override {
    return import_any(s, 0, n, h);
  }
  int import_points(const msmz_src& s, uint64_t n, uint64_t* h, const GenMap* = nullptr) override {
    return import_any(s, fb_, n, h);
  }
  int import_scalars_into(uint64_t, uint64_t, const msmz_src&, uint64_t) override {
    return MSMZ_ERR_UNSUPPORTED;   // a vector start is not a block boundary of the devices' shares
  }
  int gather_src(const msmz_src& s, int point_fe_bytes, uint64_t n, std::vector<uint8_t>* recs,
                 std::vector<uint8_t>* flags) override {
    return workers_[0]->eng->gather_src(s, point_fe_bytes, n, recs, flags);
  }

  int random_points(uint64_t n, uint64_t seed, const GenMap&, uint64_t* h) override {
    if (!h || n == 0) return MSMZ_ERR_ARG;
    return make_set(0, n, h, [&](uint32_t g, IEngine* e, uint64_t cnt, uint64_t* sub) {
      return e->random_points(cnt, seed, GenMap{G_, g, MULTI_BLOCK_SHIFT}, sub);
    });
  }

  int random_scalars(uint64_t n, uint64_t seed, const GenMap&, uint64_t* h) override {
    if (!h || n == 0) return MSMZ_ERR_ARG;
    return make_set(1, n, h, [&](uint32_t g, IEngine* e, uint64_t cnt, uint64_t* sub) {
      return e->random_scalars(cnt, seed, GenMap{G_, g, MULTI_BLOCK_SHIFT}, sub);
    });
  }

  int download_points(uint64_t hd, uint64_t first, uint64_t count, uint8_t* xy, uint8_t* inf) override {
    const MHandle* pts = range(hd, 0, first, count);
    if (!pts || !xy) return MSMZ_ERR_ARG;
    const size_t rec = 2 * (size_t)fb_;
    return for_range(*pts, first, count, [&](IEngine* e, uint64_t sub, uint64_t li, uint64_t gi, uint64_t len) {
      return e->download_points(sub, li, len, xy + (gi - first) * rec, inf ? inf + (gi - first) : nullptr);
    });
  }

  int download_points_compressed(uint64_t hd, uint64_t first, uint64_t count, uint8_t* out, uint8_t* inf,
                                 uint32_t flags) override {
    const MHandle* pts = range(hd, 0, first, count);
    if (!pts || !out || (flags & ~(uint32_t)MSMZ_SRC_SIGN_PARITY)) return MSMZ_ERR_ARG;
    return for_range(*pts, first, count, [&](IEngine* e, uint64_t sub, uint64_t li, uint64_t gi, uint64_t len) {
      return e->download_points_compressed(sub, li, len, out + (gi - first) * (size_t)fb_,
                                           inf ? inf + (gi - first) : nullptr, flags);
    });
  }

  int download_scalars(uint64_t hd, uint64_t first, uint64_t count, uint8_t* s) override {
    const MHandle* sc = range(hd, 1, first, count);
    if (!sc || !s) return MSMZ_ERR_ARG;
    return for_range(*sc, first, count, [&](IEngine* e, uint64_t sub, uint64_t li, uint64_t gi, uint64_t len) {
      return e->download_scalars(sub, li, len, s + (gi - first) * 32);
    });
  }

  // msmz_export_scalars / _points to a host destination: every engine exports its own blocks to
  // ptr + (global index - first) * stride, as the downloads do.  A device destination is refused.
  int export_scalars(uint64_t hd, uint64_t first, uint64_t n, const msmz_dst& d) override {
    return export_any(hd, 1, 0, first, n, d);
  }
  int export_points(uint64_t hd, uint64_t first, uint64_t n, const msmz_dst& d) override {
    return export_any(hd, 0, fb_, first, n, d);
  }

  int free_handle(uint64_t hd) override {
    auto it = handles_.find(hd);
    if (it == handles_.end()) return MSMZ_ERR_ARG;
    free_shares(it->second);
    handles_.erase(it);
    return MSMZ_OK;
  }

  // Every engine computes the partial sums of the `batch` problems over its share of the points; the host adds them per
  // problem.  Resident scalars of a batch are gathered to the host first: vector k starts at entry k n of the set, which
  // is not a block boundary of the devices' shares unless n is a multiple of the block cycle.  (batch = 1: vector 0
  // starts at a block boundary, each device reads its own share of the set.)
  int msm_batch(uint64_t ph, const uint8_t* host_scalars, uint64_t sh, uint64_t n, uint32_t batch, const msmz_opts* o,
                uint8_t* out, int* out_inf, msmz_log* log, const GenMap* = nullptr, uint64_t = 0) override {
    if (!out || !out_inf || n == 0 || batch == 0) return MSMZ_ERR_ARG;
    const MHandle* pp = range(ph, 0, 0, n);
    if (!pp) return MSMZ_ERR_ARG;
    const MHandle* sc = nullptr;
    std::vector<uint8_t> gathered;
    if (!host_scalars) {
      const MHandle* all = get(sh, 1);
      if (!all || all->n / batch < n) return MSMZ_ERR_ARG;
      if (batch == 1) {
        sc = all;
      } else {
        gathered.resize((size_t)batch * n * 32);
        if (int st = download_scalars(sh, 0, (uint64_t)batch * n, gathered.data())) return st;
        host_scalars = gathered.data();
      }
    }
    const size_t rec = 2 * (size_t)fb_;
    std::vector<std::vector<uint8_t>> part(G_, std::vector<uint8_t>(rec * batch));
    std::vector<std::vector<int>> pinf(G_, std::vector<int>(batch, 1));
    std::vector<int> used(G_, 0);
    std::vector<msmz_log> logs(G_);
    const MHandle& pts = *pp;
    int st = for_shares(n, [&](uint32_t g, IEngine* e, uint64_t cnt) {
      used[g] = 1;
      if (sc) return e->msm_batch(pts.sub[g], nullptr, sc->sub[g], cnt, 1, o, part[g].data(), pinf[g].data(), &logs[g]);
      const GenMap split{G_, g, MULTI_BLOCK_SHIFT};   // the device copies its own blocks of every vector
      return e->msm_batch(pts.sub[g], host_scalars, 0, cnt, batch, o, part[g].data(), pinf[g].data(), &logs[g], &split, n);
    });
    if (st) return st;
    bool first = true;
    for (uint32_t g = 0; g < G_; g++) {
      if (!used[g]) continue;
      for (uint32_t k = 0; k < batch && st == MSMZ_OK; k++) {
        const uint8_t* pk = part[g].data() + (size_t)k * rec;
        if (first) {
          memcpy(out + (size_t)k * rec, pk, rec);
          out_inf[k] = pinf[g][k];
        } else {
          st = fold_partial(curve_id_, rec, out + (size_t)k * rec, &out_inf[k], pk, pinf[g][k]);
        }
      }
      if (st) return st;
      if (log) merge_log(log, logs[g], first, LogMerge::PARALLEL);
      first = false;
    }
    return MSMZ_OK;
  }

  int msm_segments(uint64_t, uint64_t, const msmz_segment*, uint32_t, const msmz_opts*, uint8_t*, int*, msmz_log*) override {
    return MSMZ_ERR_UNSUPPORTED;   // a range is not a prefix of a device's share (as import_scalars_into)
  }

  // every engine precomputes its own share of the points (the same c, GLV choice and copies, chosen for the whole set)
  int precompute_params(uint64_t n, const msmz_opts* o, uint32_t factor, int* c, int* glv, uint32_t* copies,
                        int* K, int* sbits) const override {
    return workers_[0]->eng->precompute_params(n, o, factor, c, glv, copies, K, sbits);
  }
  int precompute_points(uint64_t ph, uint64_t n, int c, int glv, uint32_t copies, int sbits, uint64_t* h) override {
    const MHandle* plain = get(ph, 0);
    if (!h || !plain || plain->factor != 0 || n == 0 || plain->n < n) return MSMZ_ERR_ARG;
    const MHandle& src = *plain;
    MHandle mh = new_set(0, n);
    int st = for_shares(n, [&](uint32_t g, IEngine* e, uint64_t cnt) {
      return e->precompute_points(src.sub[g], cnt, c, glv, copies, sbits, &mh.sub[g]);
    });
    mh.factor = copies;
    mh.glv = glv;
    return finish_handle(st, mh, h);
  }
  int precomputed_info(uint64_t hd, int32_t* c, int32_t* glv, uint32_t* factor, uint32_t* K, uint64_t* records,
                       int32_t* sbits) override {
    const MHandle* pre = get(hd, 0);
    if (!pre || pre->factor == 0) return MSMZ_ERR_ARG;
    if (records) *records = (uint64_t)pre->factor * pre->n * (pre->glv ? 2 : 1);
    return workers_[0]->eng->precomputed_info(pre->sub[0], c, glv, factor, K, nullptr, sbits);   // (shard 0 holds block 0)
  }

  // Every engine checks its own share: the set indices [first, first + count) that live on device g are one contiguous
  // range of its local array (the local order is the set order), [shard_count(first), shard_count(first + count)).  Local
  // indices go back to set indices through the block split, as in download_points.
  int check_points(uint64_t hd, uint64_t first, uint64_t count, uint32_t what, msmz_check_result* out,
                   uint8_t* verdicts) override {
    if (!out || count == 0 || what == 0 || (what & ~(uint32_t)(MSMZ_CHECK_CURVE | MSMZ_CHECK_SUBGROUP))) return MSMZ_ERR_ARG;
    const MHandle* pts = get(hd, 0);
    if (!pts) return MSMZ_ERR_ARG;
    if (pts->factor) return MSMZ_ERR_UNSUPPORTED;
    if (!in_range(first, count, pts->n)) return MSMZ_ERR_ARG;
    const MHandle& mh = *pts;
    std::vector<msmz_check_result> res(G_, msmz_check_result{0, 0, UINT64_MAX});
    std::vector<std::vector<uint8_t>> local(G_);
    std::vector<uint64_t> lo(G_), cnt(G_);
    for (uint32_t g = 0; g < G_; g++) {
      lo[g] = shard_count(first, g, G_);
      cnt[g] = shard_count(first + count, g, G_) - lo[g];
      if (verdicts) local[g].resize(cnt[g]);
    }
    int st = for_all([&](uint32_t g, IEngine* e) {
      if (cnt[g] == 0) return (int)MSMZ_OK;
      return e->check_points(mh.sub[g], lo[g], cnt[g], what, &res[g], verdicts ? local[g].data() : nullptr);
    });
    if (st) return st;
    *out = msmz_check_result{0, 0, UINT64_MAX};
    const uint64_t mask = (1ull << MULTI_BLOCK_SHIFT) - 1;
    for (uint32_t g = 0; g < G_; g++) {
      out->off_curve += res[g].off_curve;
      out->off_subgroup += res[g].off_subgroup;
      if (res[g].first_bad == UINT64_MAX) continue;
      const uint64_t li = res[g].first_bad;
      const uint64_t gi = ((((li >> MULTI_BLOCK_SHIFT) * G_ + g) << MULTI_BLOCK_SHIFT)) | (li & mask);
      if (gi < out->first_bad) out->first_bad = gi;
    }
    if (!verdicts) return MSMZ_OK;
    return for_range(mh, first, count, [&](IEngine*, uint64_t, uint64_t li, uint64_t gi, uint64_t len) {
      const uint32_t g = (uint32_t)((gi >> MULTI_BLOCK_SHIFT) % G_);
      memcpy(verdicts + (gi - first), local[g].data() + (li - lo[g]), len);
      return (int)MSMZ_OK;
    });
  }

  // Every engine multiplies its own share of the points, under the call's options; the result is dealt like an upload.
  // Index i of P, s and Q lives on one device only when all three ranges start at a block-cycle boundary; only first = 0
  // is taken.
  int points_mul(const msmz_mul& m, const msmz_mul_opts& o, uint64_t n, uint64_t* h) override {
    if (!h || n == 0) return MSMZ_ERR_ARG;
    const MHandle* P = get(m.points_handle, 0);
    const MHandle* Q = m.addend_handle ? get(m.addend_handle, 0) : nullptr;
    const MHandle* S = m.scalars_handle ? get(m.scalars_handle, 1) : nullptr;
    if (!P || (m.addend_handle && !Q) || (m.scalars_handle ? !S : !m.scalar)) return MSMZ_ERR_ARG;
    if (P->factor || (Q && Q->factor)) return MSMZ_ERR_UNSUPPORTED;
    if (!in_range(m.first_p, n, P->n) || (Q && !in_range(m.first_q, n, Q->n)) || (S && !in_range(m.first_s, n, S->n)))
      return MSMZ_ERR_ARG;
    if (m.first_p || (m.scalars_handle && m.first_s) || (m.addend_handle && m.first_q)) return MSMZ_ERR_UNSUPPORTED;
    return make_set(0, n, h, [&](uint32_t g, IEngine* e, uint64_t cnt, uint64_t* sub) {
      msmz_mul mine = m;
      mine.points_handle = P->sub[g];
      mine.scalars_handle = S ? S->sub[g] : 0;
      mine.addend_handle = Q ? Q->sub[g] : 0;
      return e->points_mul(mine, o, cnt, sub);
    });
  }

  // msmz_points_fixed_base: the base becomes bytes once (a resident one: the one record is downloaded from the engine
  // that holds it; a record at infinity comes back all zero, which is how the engines read it), then every engine
  // multiplies its own share of the scalars from its own table, and the result is dealt like an upload.
  int points_fixed_base(const msmz_fixed_base& f, uint64_t n, uint64_t* h) override {
    if (!h || n == 0) return MSMZ_ERR_ARG;
    if (f.base_handle ? f.base_xy_le != nullptr : f.base_index != 0) return MSMZ_ERR_ARG;
    const MHandle* S = get(f.scalars_handle, 1);
    if (!S || !in_range(f.first_s, n, S->n)) return MSMZ_ERR_ARG;
    std::vector<uint8_t> xy;
    if (f.base_handle) {
      const MHandle* B = get(f.base_handle, 0);
      if (!B) return MSMZ_ERR_ARG;
      if (B->factor) return MSMZ_ERR_UNSUPPORTED;
      if (!in_range(f.base_index, 1, B->n)) return MSMZ_ERR_ARG;
    }
    if (f.first_s) return MSMZ_ERR_UNSUPPORTED;
    if (f.base_handle) {
      xy.resize(2 * (size_t)fb_);
      if (int st = download_points(f.base_handle, f.base_index, 1, xy.data(), nullptr)) return st;
    }
    return make_set(0, n, h, [&](uint32_t g, IEngine* e, uint64_t cnt, uint64_t* sub) {
      msmz_fixed_base mine = f;
      mine.base_handle = 0;
      mine.base_index = 0;
      if (!xy.empty()) mine.base_xy_le = xy.data();
      mine.scalars_handle = S->sub[g];
      return e->points_fixed_base(mine, cnt, sub);
    });
  }

  // Every engine combines its own share.  Entry i of every operand and of the destination lives on one device only when
  // all ranges start at 0 (as points_mul), and an existing destination is then written whole: n is its length.
  int scalars_combine(const msmz_scalar_term& x, const msmz_scalar_term* y, uint64_t n, uint64_t first_out,
                      uint64_t* out_handle) override {
    if (!out_handle || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    const bool fresh = *out_handle == 0;
    if (fresh && first_out != 0) return MSMZ_ERR_ARG;
    const msmz_scalar_term* in[2] = {&x, y};
    const MHandle* v[2] = {nullptr, nullptr};
    const MHandle* c[2] = {nullptr, nullptr};
    bool shifted = first_out != 0;
    for (int k = 0; k < 2; k++) {
      if (!in[k]) continue;
      if (!(v[k] = range(in[k]->handle, 1, in[k]->first, n))) return MSMZ_ERR_ARG;
      if (in[k]->coeff_handle && !(c[k] = range(in[k]->coeff_handle, 1, in[k]->coeff_first, n))) return MSMZ_ERR_ARG;
      shifted = shifted || in[k]->first || (in[k]->coeff_handle && in[k]->coeff_first);
    }
    const MHandle* dst = nullptr;
    if (!fresh && !(dst = range(*out_handle, 1, first_out, n))) return MSMZ_ERR_ARG;
    if (shifted || (dst && dst->n != n)) return MSMZ_ERR_UNSUPPORTED;
    MHandle mh = new_set(1, n);
    int st = for_shares(n, [&](uint32_t g, IEngine* e, uint64_t cnt) {
      msmz_scalar_term sub[2];
      for (int k = 0; k < 2; k++) {
        if (!in[k]) continue;
        sub[k] = *in[k];
        sub[k].handle = v[k]->sub[g];
        sub[k].coeff_handle = c[k] ? c[k]->sub[g] : 0;
      }
      if (dst) mh.sub[g] = dst->sub[g];
      return e->scalars_combine(sub[0], y ? &sub[1] : nullptr, cnt, 0, &mh.sub[g]);
    });
    if (dst) return st;   // (written in place: the handle stays the caller's)
    return finish_handle(st, mh, out_handle);
  }

  // every engine sums over its own share (both ranges from 0: a prefix of every share); the host adds the sums mod q
  int scalars_dot(uint64_t xh, uint64_t first_x, uint64_t yh, uint64_t first_y, uint64_t n, uint8_t* out) override {
    if (!out || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    if (!yh && first_y) return MSMZ_ERR_ARG;
    const MHandle* X = range(xh, 1, first_x, n);
    const MHandle* Y = yh ? range(yh, 1, first_y, n) : nullptr;
    if (!X || (yh && !Y)) return MSMZ_ERR_ARG;
    if (first_x || first_y) return MSMZ_ERR_UNSUPPORTED;
    std::vector<uint32_t> part((size_t)G_ * 8, 0);
    int st = for_shares(n, [&](uint32_t g, IEngine* e, uint64_t cnt) {
      return e->scalars_dot(X->sub[g], 0, Y ? Y->sub[g] : 0, 0, cnt,
                            reinterpret_cast<uint8_t*>(part.data() + (size_t)g * 8));
    });
    if (st) return st;
    uint32_t acc[8] = {};
    for (uint32_t g = 0; g < G_; g++)
      if ((st = fold_scalar(curve_id_, acc, part.data() + (size_t)g * 8))) return st;
    memcpy(out, acc, 32);
    return MSMZ_OK;
  }

  int scalars_powers(const uint8_t* base, const uint8_t* ratio, uint64_t n, const GenMap&, uint64_t* h) override {
    if (!h || !ratio || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    return make_set(1, n, h, [&](uint32_t g, IEngine* e, uint64_t cnt, uint64_t* sub) {
      return e->scalars_powers(base, ratio, cnt, GenMap{G_, g, MULTI_BLOCK_SHIFT}, sub);
    });
  }

  // A recurrence is sequential in the set index, and consecutive blocks of a set live on different engines: the
  // dependency would cross every block boundary.  Refused (after the checks that need no handle).
  int scalars_recurrence(const msmz_scalar_rec& r, uint64_t n, uint64_t, uint64_t* out_handle, uint8_t*) override {
    if (!out_handle || n == 0 || n >> 32 || (r.flags & ~(uint32_t)(MSMZ_REC_REVERSE | MSMZ_REC_EXCLUSIVE)) ||
        (!r.a_handle && !r.a && !r.b_handle))
      return MSMZ_ERR_ARG;
    return MSMZ_ERR_UNSUPPORTED;
  }

  // element-wise: every engine inverts its own share, as scalars_combine (all ranges from 0, an existing destination
  // written whole); the zero counts add up
  int scalars_inverse(uint64_t h, uint64_t first, uint64_t n, uint64_t first_out, uint64_t* out_handle,
                      uint64_t* n_zero) override {
    if (!out_handle || n == 0 || n >> 32) return MSMZ_ERR_ARG;
    const bool fresh = *out_handle == 0;
    if (fresh && first_out != 0) return MSMZ_ERR_ARG;
    const MHandle* src = range(h, 1, first, n);
    if (!src) return MSMZ_ERR_ARG;
    const MHandle* dst = nullptr;
    if (!fresh && !(dst = range(*out_handle, 1, first_out, n))) return MSMZ_ERR_ARG;
    if (dst && *out_handle == h && partial_overlap(first, first_out, n)) return MSMZ_ERR_ARG;
    if (first || first_out || (dst && dst->n != n)) return MSMZ_ERR_UNSUPPORTED;
    MHandle mh = new_set(1, n);
    std::vector<uint64_t> zeros(G_, 0);
    int st = for_shares(n, [&](uint32_t g, IEngine* e, uint64_t cnt) {
      if (dst) mh.sub[g] = dst->sub[g];
      return e->scalars_inverse(src->sub[g], 0, cnt, 0, &mh.sub[g], &zeros[g]);
    });
    if (!st && n_zero) {
      *n_zero = 0;
      for (uint64_t z : zeros) *n_zero += z;
    }
    if (dst) return st;   // (written in place: the handle stays the caller's)
    return finish_handle(st, mh, out_handle);
  }

  // A gate expression without a rotated operand is element-wise: every engine evaluates its own share, as
  // scalars_combine (every range from 0, an existing destination written whole).  A rotation reads across the
  // boundaries between blocks of 2^16 entries, which live on different engines: refused, after every check that needs
  // no engine.  The engines get the factors with rotation 0: a multiple of n is no multiple of a share's length.
  int scalars_expr(const msmz_expr& e, uint64_t first_out, uint64_t* out_handle) override {
    if (!out_handle) return MSMZ_ERR_ARG;
    uint8_t named[MSMZ_EXPR_MAX_COLUMNS];
    bool rotated = false;
    if (int st = expr_precheck(e, named, &rotated)) return st;
    const bool fresh = *out_handle == 0;
    if (fresh && first_out != 0) return MSMZ_ERR_ARG;
    const MHandle* col[MSMZ_EXPR_MAX_COLUMNS];
    bool shifted = first_out != 0;
    for (uint32_t c = 0; c < e.n_columns; c++) {
      if (!(col[c] = range(e.columns[c].handle, 1, e.columns[c].first, e.n))) return MSMZ_ERR_ARG;
      const uint64_t first = e.columns[c].first;   // (named[c] == 1: read at rotation 0 only; 3: read rotated)
      if (e.columns[c].handle == *out_handle && named[c] &&
          (named[c] & 2 ? ranges_meet(first, e.n, first_out, e.n) : partial_overlap(first, first_out, e.n)))
        return MSMZ_ERR_ARG;
      shifted = shifted || e.columns[c].first;
    }
    const MHandle* dst = nullptr;
    if (!fresh && !(dst = range(*out_handle, 1, first_out, e.n))) return MSMZ_ERR_ARG;
    if (rotated || shifted || (dst && dst->n != e.n)) return MSMZ_ERR_UNSUPPORTED;
    std::vector<msmz_expr_factor> factors;
    std::vector<msmz_expr_term> terms(e.terms, e.terms + e.n_terms);
    for (const msmz_expr_term& t : terms)
      for (uint32_t f = 0; f < t.n_factors; f++) factors.push_back({t.factors[f].column, 0});
    size_t at = 0;
    for (msmz_expr_term& t : terms) {
      t.factors = t.n_factors ? factors.data() + at : nullptr;
      at += t.n_factors;
    }
    MHandle mh = new_set(1, e.n);
    int st = for_shares(e.n, [&](uint32_t g, IEngine* eng, uint64_t cnt) {
      msmz_expr_column sub[MSMZ_EXPR_MAX_COLUMNS];
      for (uint32_t c = 0; c < e.n_columns; c++) sub[c] = {col[c]->sub[g], 0};
      msmz_expr mine = e;
      mine.columns = sub;
      mine.terms = terms.data();
      mine.n = cnt;
      if (dst) mh.sub[g] = dst->sub[g];
      return eng->scalars_expr(mine, 0, &mh.sub[g]);
    });
    if (dst) return st;   // (written in place: the handle stays the caller's)
    return finish_handle(st, mh, out_handle);
  }

  // The butterflies of a transform cross every boundary between blocks of 2^16 entries, and consecutive blocks live on
  // different engines: refused, as a recurrence is (after the checks that need no handle).
  int scalars_ntt(const msmz_ntt& t, uint64_t, uint64_t* out_handle) override {
    if (!out_handle || t.count == 0 || (t.flags & ~(uint32_t)(MSMZ_NTT_INVERSE | MSMZ_NTT_COSET)) ||
        ((t.flags & MSMZ_NTT_COSET) != 0) != (t.shift != nullptr))
      return MSMZ_ERR_ARG;
    return MSMZ_ERR_UNSUPPORTED;
  }

  int test_set_glv_bits(int bits) override {
    return on_every([&](IEngine* e) { return e->test_set_glv_bits(bits); });
  }
  int test_retries() override {
    int r = 0;
    for (Worker* w : workers_) r += w->eng->test_retries();
    return r;
  }
  int test_set_limits(uint64_t pass_entries, uint64_t batch_entries) override {
    return on_every([&](IEngine* e) { return e->test_set_limits(pass_entries, batch_entries); });
  }
  int test_set_fixed_base_window(int c) override {
    return on_every([&](IEngine* e) { return e->test_set_fixed_base_window(c); });
  }
  uint64_t test_fixed_base_tables() override {
    uint64_t built = 0;
    for (Worker* w : workers_) built += w->eng->test_fixed_base_tables();
    return built;
  }
  uint64_t test_ntt_tables() override {
    uint64_t built = 0;
    for (Worker* w : workers_) built += w->eng->test_ntt_tables();
    return built;
  }
  void test_passes(uint64_t* range_passes, uint64_t* sub_batches) override {
    uint64_t rp = 0, sb = 0;
    for (Worker* w : workers_) {
      uint64_t r = 0, s = 0;
      w->eng->test_passes(&r, &s);
      rp += r;
      sb += s;
    }
    if (range_passes) *range_passes = rp;
    if (sub_batches) *sub_batches = sb;
  }
  int test_poison(int pattern, uint64_t* buffers, uint64_t* bytes) override {   // every engine's; the sums
    uint64_t tb = 0, ty = 0;
    const int st = on_every([&](IEngine* e) {
      uint64_t nb = 0, by = 0;
      const int s = e->test_poison(pattern, &nb, &by);
      tb += nb, ty += by;
      return s;
    });
    if (st) return st;
    if (buffers) *buffers = tb;
    if (bytes) *bytes = ty;
    return MSMZ_OK;
  }
  int test_scratch(int engine, uint64_t* buffers, uint64_t* bytes) override {   // one engine's own
    if (engine < 0 || (uint32_t)engine >= G_) return MSMZ_ERR_ARG;
    return workers_[engine]->eng->test_scratch(0, buffers, bytes);
  }
  ITestHooks* test_hooks() override { return workers_[0]->eng->test_hooks(); }

 private:
  int import_any(const msmz_src& s, int point_fe_bytes, uint64_t n, uint64_t* h) {
    if (!h || n == 0) return MSMZ_ERR_ARG;
    std::vector<uint8_t> recs, flags;
    if (int st = gather_src(s, point_fe_bytes, n, &recs, &flags)) return st;
    msmz_src hs{};
    hs.ptr = recs.data();
    hs.width = (uint32_t)(recs.size() / n);
    hs.flags = s.flags & (MSMZ_SRC_MONTGOMERY | MSMZ_SRC_COMPRESSED | MSMZ_SRC_SIGN_PARITY);   // (the form of the records)
    hs.is_inf = flags.empty() ? nullptr : flags.data();
    return make_set(point_fe_bytes ? 0 : 1, n, h, [&](uint32_t g, IEngine* e, uint64_t cnt, uint64_t* sub) {
      const GenMap split{G_, g, MULTI_BLOCK_SHIFT};
      return point_fe_bytes ? e->import_points(hs, cnt, sub, &split) : e->import_scalars(hs, cnt, sub, &split);
    });
  }

  int export_any(uint64_t hd, int kind, int point_fe_bytes, uint64_t first, uint64_t n, const msmz_dst& d) {
    uint32_t width = 0;
    uint64_t stride = 0;
    if (int st = dst_check(&d, point_fe_bytes, &width, &stride)) return st;
    const MHandle* set = range(hd, kind, first, n);
    if (!set || n == 0) return MSMZ_ERR_ARG;
    if (d.flags & MSMZ_SRC_DEVICE) return MSMZ_ERR_UNSUPPORTED;
    return for_range(*set, first, n, [&](IEngine* e, uint64_t sub, uint64_t li, uint64_t gi, uint64_t len) {
      msmz_dst piece = d;
      piece.ptr = (uint8_t*)d.ptr + (gi - first) * stride;
      piece.stride = stride;
      piece.is_inf = d.is_inf ? d.is_inf + (gi - first) : nullptr;
      return kind ? e->export_scalars(sub, li, len, piece) : e->export_points(sub, li, len, piece);
    });
  }

  struct MHandle {
    int kind;
    uint64_t n;
    std::vector<uint64_t> sub;   // per-device handle (0 = that device holds nothing)
    uint32_t factor = 0;         // precomputed point set: copies (0 = plain) and GLV choice
    int glv = 0;
  };

  // one persistent host thread per device: runs the tasks posted for its engine
  struct Worker {
    IEngine* eng;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> task;
    bool has_task = false, done = false, stop = false;
    int status = 0;
    explicit Worker(IEngine* e) : eng(e) {
      th = std::thread([this] {
        std::unique_lock<std::mutex> lk(mu);
        while (true) {
          cv.wait(lk, [this] { return has_task || stop; });
          if (stop) return;
          std::function<int()> f = std::move(task);
          has_task = false;
          lk.unlock();
          const int st = f();
          lk.lock();
          status = st;
          done = true;
          cv.notify_all();
        }
      });
    }
    ~Worker() {
      {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
      }
      cv.notify_all();
      th.join();
      delete eng;
    }
    void post(std::function<int()> f) {
      std::lock_guard<std::mutex> lk(mu);
      task = std::move(f);
      has_task = true;
      done = false;
      cv.notify_all();
    }
    int wait() {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [this] { return done; });
      return status;
    }
  };

  // a set of n records of `kind` that no engine holds a share of yet
  MHandle new_set(int kind, uint64_t n) const { return MHandle{kind, n, std::vector<uint64_t>(G_, 0)}; }
  // a new set whose shares the engines make: fn(g, engine, entries of its share, where its handle goes)
  int make_set(int kind, uint64_t n, uint64_t* h, const std::function<int(uint32_t, IEngine*, uint64_t, uint64_t*)>& fn) {
    MHandle mh = new_set(kind, n);
    const int st = for_shares(n, [&](uint32_t g, IEngine* e, uint64_t cnt) { return fn(g, e, cnt, &mh.sub[g]); });
    return finish_handle(st, mh, h);
  }
  // the set `h` if it is of `kind`, or null; `range`: and if [first, first + n) lies inside it
  const MHandle* get(uint64_t h, int kind) const {
    auto it = handles_.find(h);
    return it == handles_.end() || it->second.kind != kind ? nullptr : &it->second;
  }
  const MHandle* range(uint64_t h, int kind, uint64_t first, uint64_t n) const {
    const MHandle* mh = get(h, kind);
    return mh && in_range(first, n, mh->n) ? mh : nullptr;
  }
  void free_shares(const MHandle& mh) {
    for (uint32_t g = 0; g < G_; g++)
      if (mh.sub[g]) (void)workers_[g]->eng->free_handle(mh.sub[g]);
  }

  // fn(engine) on every engine, one after another; the first non-zero status wins
  int on_every(const std::function<int(IEngine*)>& fn) {
    int st = MSMZ_OK;
    for (Worker* w : workers_) {
      const int s = fn(w->eng);
      if (s && !st) st = s;
    }
    return st;
  }

  // for_all over the engines that hold a share of the first n entries of a set: fn(g, engine, entries of its share)
  int for_shares(uint64_t n, const std::function<int(uint32_t, IEngine*, uint64_t)>& fn) {
    return for_all([&](uint32_t g, IEngine* e) {
      const uint64_t cnt = shard_count(n, g, G_);
      return cnt ? fn(g, e, cnt) : (int)MSMZ_OK;
    });
  }

  // run fn(g, engine) on every device's thread concurrently; first non-zero status wins (but MSMZ_ERR_RANGE on any
  // device beats MSMZ_ERR_POINT, as it does inside one engine's compressed import)
  int for_all(const std::function<int(uint32_t, IEngine*)>& fn) {
    for (uint32_t g = 0; g < G_; g++) {
      Worker* w = workers_[g];
      w->post([&fn, g, w] { return fn(g, w->eng); });
    }
    int st = MSMZ_OK;
    for (uint32_t g = 0; g < G_; g++) {
      const int s = workers_[g]->wait();
      if (s && (!st || (st == MSMZ_ERR_POINT && s == MSMZ_ERR_RANGE))) st = s;
    }
    return st;
  }

  // pieces of the global range [first, first + count): fn(engine, sub handle, local index, global index, length)
  int for_range(const MHandle& mh, uint64_t first, uint64_t count,
                const std::function<int(IEngine*, uint64_t, uint64_t, uint64_t, uint64_t)>& fn) {
    const uint64_t blk = 1ull << MULTI_BLOCK_SHIFT;
    uint64_t gi = first;
    const uint64_t end = first + count;
    while (gi < end) {
      const uint64_t b = gi >> MULTI_BLOCK_SHIFT;
      const uint32_t g = (uint32_t)(b % G_);
      uint64_t len = ((b + 1) << MULTI_BLOCK_SHIFT) - gi;
      if (len > end - gi) len = end - gi;
      const uint64_t li = ((b / G_) << MULTI_BLOCK_SHIFT) | (gi & (blk - 1));
      const int st = fn(workers_[g]->eng, mh.sub[g], li, gi, len);
      if (st) return st;
      gi += len;
    }
    return MSMZ_OK;
  }

  int finish_handle(int st, MHandle& mh, uint64_t* h) {
    if (st) return free_shares(mh), st;
    *h = next_handle_++;
    handles_[*h] = std::move(mh);
    return MSMZ_OK;
  }

  int curve_id_, fb_;
  uint32_t G_;
  std::vector<Worker*> workers_;
  std::map<uint64_t, MHandle> handles_;
  uint64_t next_handle_ = 1;
};

}  // namespace msmz

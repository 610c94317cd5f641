// The operations on resident point sets that are neither data movement nor an MSM, as one stage: the point checks,
// per-point multiplication and fixed-base multiplication with its cache of window tables.  PointOps owns what only these
// touch (check_, the cache) and reaches the engine through the SetsCore it is built with (sets_core.h); ResidentSets
// (resident.h) forwards the IEngine methods here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <deque>
#include <vector>

#include "../../include/msmz.h"
#include "check_kernels.h"
#include "fixed_kernels.h"
#include "mul_kernels.h"
#include "sets_core.h"

namespace msmz {

template <class Cfg>
class PointOps {
  using Core = SetsCore<Cfg>;
  using F = typename Cfg::F;
  using Fr = typename Cfg::Fr;
  using P = typename Cfg::P;
  static constexpr int NW = Core::NW, RW = Core::RW, PW_WORDS = Core::PW_WORDS;
  static constexpr bool TE = Cfg::TE;
  static constexpr uint32_t kBlock = Core::kBlock;

 public:
  explicit PointOps(Core& core) : core_(core) {}

  // f(buffer) for every scratch buffer of the stage: undefined at the start of every call.  (Not the cached tables: they
  // stay valid across calls, and are bound to the engine's Poison when they are built.)
  template <class Fn>
  void each_scratch(Fn f) {
    f(check_);
  }

  // ------------------------------------------------------------------------------------------ validation
  // msmz_check_points: the curve equation, then (if asked, and unless the curve has cofactor 1) [q]P = O, over base
  // points [first, first + count) of a plain point handle.  A query: bad points are reported, not refused.  Two launches,
  // then the result record and the verdict bytes behind it come back in ONE copy behind ONE host wait (into pinned
  // memory: a copy into the caller's pageable buffer would block the host a second time).
  int check_points(uint64_t hd, uint64_t first, uint64_t count, uint32_t what, msmz_check_result* out, uint8_t* verdicts) {
    if (!out || count == 0 || what == 0 || (what & ~(uint32_t)(MSMZ_CHECK_CURVE | MSMZ_CHECK_SUBGROUP))) return MSMZ_ERR_ARG;
    const Handle* pts = core_.handles_.get(hd, 0);
    if (!pts) return MSMZ_ERR_ARG;
    if (pts->factor) return MSMZ_ERR_UNSUPPORTED;   // derived data: the source set is what a caller checks
    const uint32_t* recs = core_.handles_.range(hd, 0, first, count, PW_WORDS);   // (base points only)
    if (!recs) return MSMZ_ERR_ARG;
    MSMZ_HIP(hipSetDevice(core_.device_));
    const bool chain = (what & MSMZ_CHECK_SUBGROUP) && !Fr::PRIME_ORDER;   // cofactor 1: the curve is the subgroup
    typename Core::Record rec;   // no error word; first_bad starts as "none"; the verdicts ride behind the record
    rec.head = sizeof(CheckResult), rec.err_word = -1, rec.preset_word = offsetof(CheckResult, first_bad) / 4;
    rec.tail = verdicts ? count : 0;
    const int st = core_.recorded(check_, sizeof(CheckResult) + count, [&](uint32_t* d) {
      CheckResult* d_res = reinterpret_cast<CheckResult*>(d);
      uint8_t* d_verdicts = reinterpret_cast<uint8_t*>(d) + sizeof(CheckResult);
      const dim3 grid = Core::blocks_of(count), block(kBlock);
      hipLaunchKernelGGL((k_check_curve<P>), grid, block, 0, core_.stream_, d_verdicts, d_res, recs, (uint32_t)count, (uint32_t)first);
      if (chain)
        hipLaunchKernelGGL((k_check_subgroup<P, Fr>), grid, block, 0, core_.stream_, d_verdicts, d_res, recs, (uint32_t)count, (uint32_t)first);
    }, rec);
    if (st) return st;
    const CheckResult* res = core_.h_res_.template as<const CheckResult>();
    if (verdicts) memcpy(verdicts, core_.h_res_.template as<const uint8_t>() + sizeof(CheckResult), count);
    out->off_curve = res->off_curve;
    out->off_subgroup = res->off_subgroup;
    out->first_bad = res->first_bad == 0xffffffffu ? UINT64_MAX : res->first_bad;
    return MSMZ_OK;
  }

  // ------------------------------------------------------------------------------------------ per-point multiplication
  // msmz_points_mul(_opts): a new plain point handle, record i = [s_i] P_i (+ Q_i).  One launch of the chain that
  // points_mul_chain picks from the options (mul_kernels.h); the error word (a resident scalar >= q or >= the caller's
  // bound) comes back behind the ONE host wait, like that of an upload.  (msmz.hip has checked the options' ranges.)
  int points_mul(const msmz_mul& m, const msmz_mul_opts& o, uint64_t n, uint64_t* h) {
    HandleTable& handles = core_.handles_;
    if (!h || !Core::points_fit(n)) return MSMZ_ERR_ARG;
    const Handle* pts = handles.get(m.points_handle, 0);
    const Handle* add = m.addend_handle ? handles.get(m.addend_handle, 0) : nullptr;
    if (!pts || (m.addend_handle && !add)) return MSMZ_ERR_ARG;
    if (m.scalars_handle ? !handles.get(m.scalars_handle, 1) : !m.scalar) return MSMZ_ERR_ARG;
    if (pts->factor || (add && add->factor)) return MSMZ_ERR_UNSUPPORTED;   // derived data
    const uint32_t* d_p = handles.range(m.points_handle, 0, m.first_p, n, PW_WORDS);
    const uint32_t* d_q = add ? handles.range(m.addend_handle, 0, m.first_q, n, PW_WORDS) : nullptr;
    const uint32_t* S = m.scalars_handle ? handles.range(m.scalars_handle, 1, m.first_s, n, 8) : nullptr;
    if (!d_p || (add && !d_q) || (m.scalars_handle && !S)) return MSMZ_ERR_ARG;
    const MulChain chain = points_mul_chain<Fr>((o.flags & MSMZ_MUL_SUBGROUP) != 0, o.scalar_bits);
    const int bound = o.scalar_bits == 0 || o.scalar_bits >= Fr::BITS ? Fr::BITS : o.scalar_bits;
    MulScalar bc{};
    if (!S) {
      if (int st = Core::read_fr(m.scalar, bc.w, false)) return st;
      if (words_geq_pow2(bc.w, bound)) return MSMZ_ERR_RANGE;
    }
    MSMZ_HIP(hipSetDevice(core_.device_));
    Handle hd;
    if (int st = core_.new_points(n, &hd)) return st;
    hipStream_t stream = core_.stream_;
    const dim3 grid = Core::blocks_of(n), block(kBlock);   // whole blocks: every wave reaches the inversion entire
    const int st = core_.checked([&](uint32_t* d_err) {   // a resident scalar >= group order, or >= 2^bound
      if constexpr (Fr::HAS_GLV) {
        if (chain.kind == MUL_CHAIN_GLV) {
          MulGlvScalar g{};
          if (!S) glv_decompose<Fr>(g.k0, g.k1, g.neg0, g.neg1, bc.w);
          hipLaunchKernelGGL((k_points_mul_glv<P, Fr>), grid, block, 0, stream, hd.mem.as<uint32_t>(), d_p, S, g, d_q,
                             (uint32_t)n, hd.has_endo ? 1 : 0, bound, d_err);
          return;
        }
      }
      if (chain.steps == Fr::BITS)   // no bound: the instance with compile-time loop bounds
        hipLaunchKernelGGL((k_points_mul<P, Fr, false>), grid, block, 0, stream, hd.mem.as<uint32_t>(), d_p, S, bc, d_q,
                           (uint32_t)n, hd.has_endo ? 1 : 0, chain.steps, d_err);
      else
        hipLaunchKernelGGL((k_points_mul<P, Fr, true>), grid, block, 0, stream, hd.mem.as<uint32_t>(), d_p, S, bc, d_q,
                           (uint32_t)n, hd.has_endo ? 1 : 0, chain.steps, d_err);
    });
    return st ? st : core_.add_handle(std::move(hd), h);
  }

  // ------------------------------------------------------------------------------------------ fixed-base multiplication
  // msmz_points_fixed_base: a new plain point handle, record i = [s_(first_s + i)] B.  The base becomes canonical bytes
  // (a resident one: one record fetched), the planner (fixed_base.h) picks the window width for n and the bound, the
  // table comes from the cache or is built now, and ONE launch of k_fixed_mul makes the points; its error word (a
  // resident scalar >= q or >= the caller's bound) comes back behind the ONE host wait, like that of msmz_points_mul.
  int points_fixed_base(const msmz_fixed_base& f, uint64_t n, uint64_t* h) {
    if (!h || !Core::points_fit(n)) return MSMZ_ERR_ARG;
    if (f.base_handle ? f.base_xy_le != nullptr : f.base_index != 0) return MSMZ_ERR_ARG;
    const uint32_t* S = core_.handles_.range(f.scalars_handle, 1, f.first_s, n, 8);
    if (!S) return MSMZ_ERR_ARG;
    FixedKey key{};
    if (f.base_handle) {
      const Handle* b = core_.handles_.get(f.base_handle, 0);
      if (!b) return MSMZ_ERR_ARG;
      if (b->factor) return MSMZ_ERR_UNSUPPORTED;   // derived data
      const uint32_t* rec = core_.handles_.range(f.base_handle, 0, f.base_index, 1, PW_WORDS);   // (base points only)
      if (!rec) return MSMZ_ERR_ARG;
      if (int st = core_.fetch_points(rec, 1, reinterpret_cast<uint8_t*>(key.xy))) return st;
    } else if (f.base_xy_le) {
      memcpy(key.xy, f.base_xy_le, sizeof(key.xy));
      if (words_geq<NW>(key.xy, F::PW) || words_geq<NW>(key.xy + NW, F::PW)) return MSMZ_ERR_RANGE;
    } else {
      Fe<F> g, t;
      fe_set_const<F>(g, F::GX);
      fe_from_mont(t, g);
      fe_to_canon_words<F>(key.xy, t);
      fe_set_const<F>(g, F::GY);
      fe_from_mont(t, g);
      fe_to_canon_words<F>(key.xy + NW, t);
    }
    const int bits = fixed_base_bits(f.scalar_bits, Fr::BITS);
    const FixedPlan plan = fixed_window_ ? fixed_base_plan_forced(fixed_window_, bits, RW * 4)
                                         : fixed_base_plan(n, bits, TE, RW * 4);
    if (plan.c == 0) return MSMZ_ERR_ARG;   // (a forced width only: the planner always finds one)
    key.c = plan.c;
    key.K = plan.K;
    MSMZ_HIP(hipSetDevice(core_.device_));
    const uint32_t* table = nullptr;
    if (int st = fixed_table(key, plan, &table)) return st;
    Handle hd;
    if (int st = core_.new_points(n, &hd)) return st;
    hipStream_t stream = core_.stream_;
    const dim3 grid = Core::blocks_of(n), block(kBlock);   // whole blocks: every wave reaches the inversion entire
    const int st = core_.checked([&](uint32_t* d_err) {   // a resident scalar >= group order, or >= 2^bits
      if (bits == Fr::BITS)
        hipLaunchKernelGGL((k_fixed_mul<P, Fr, false>), grid, block, 0, stream, hd.mem.as<uint32_t>(), table, S, (uint32_t)n,
                           hd.has_endo ? 1 : 0, plan.c, plan.K, bits, d_err);
      else
        hipLaunchKernelGGL((k_fixed_mul<P, Fr, true>), grid, block, 0, stream, hd.mem.as<uint32_t>(), table, S, (uint32_t)n,
                           hd.has_endo ? 1 : 0, plan.c, plan.K, bits, d_err);
    });
    return st ? st : core_.add_handle(std::move(hd), h);
  }

  int test_set_fixed_base_window(int c) {
    if (c != 0 && fixed_base_plan_forced(c, Fr::BITS, RW * 4).c == 0) return MSMZ_ERR_ARG;
    fixed_window_ = c;
    return MSMZ_OK;
  }
  uint64_t test_fixed_base_tables() const { return fixed_built_; }

  // bases[k] = 2^(ck) B for k < K, as affine Montgomery records of RW words (what k_fixed_table and k_gen_table multiply
  // out on the device): c doublings from one to the next on the host.  A base that has reached infinity (B at infinity
  // or of small order) is the all-zero record.
  static void window_bases(typename P::Acc g, int K, int c, uint32_t* bases) {
    memset(bases, 0, (size_t)K * RW * 4);
    for (int k = 0; k < K; k++) {
      if (TE || !fe_is_zero_mod_p(P::denominator(g))) {
        Fe<F> inv, x, y;
        fe_inverse(inv, P::denominator(g));
        P::affine_from_inverse(x, y, g, inv);
        fe_store<F>(bases + (size_t)k * RW, x);
        fe_store<F>(bases + (size_t)k * RW + NW, y);
      }
      typename P::Acc t;
      for (int j = 0; j < c; j++) {
        P::dbl(t, g);
        g = t;
      }
    }
  }

 private:
  // The window table of a base (k_fixed_table) from the cache or built now.  The key: the base's canonical words (on the
  // Weierstrass curves all zero = the point at infinity), the window width and the number of windows.  At most
  // FIXED_CACHE tables are kept, the one unused longest goes first; all are freed with the engine.
  struct FixedKey {
    uint32_t xy[RW];
    int c, K;
  };
  struct FixedTable {
    FixedKey key;
    DevBuf mem;
  };
  int fixed_table(const FixedKey& key, const FixedPlan& plan, const uint32_t** table) {
    for (auto it = fixed_cache_.begin(); it != fixed_cache_.end(); ++it) {
      if (it->key.c == key.c && it->key.K == key.K && !memcmp(it->key.xy, key.xy, sizeof(key.xy))) {
        FixedTable hit = std::move(*it);   // to the back: the table that leaves is the one unused longest
        fixed_cache_.erase(it);
        fixed_cache_.push_back(std::move(hit));
        *table = fixed_cache_.back().mem.template as<const uint32_t>();
        return MSMZ_OK;
      }
    }
    // the bases on the host, the multiples on the device
    Fe<F> cx, cy, x, y;
    fe_unpack<F>(cx, key.xy);
    fe_unpack<F>(cy, key.xy + NW);
    fe_to_mont(x, cx);
    fe_to_mont(y, cy);
    typename P::Acc g;
    if (!TE && words_point_is_inf<F>(key.xy)) P::set_identity(g);
    else P::from_affine(g, x, y);
    std::vector<uint32_t> bases((size_t)plan.K * RW);
    window_bases(g, plan.K, plan.c, bases.data());
    FixedTable ft;
    ft.mem.poison = &core_.poison_;
    ft.key = key;
    DevBuf& stage = core_.stage_;
    if (int st = ft.mem.ensure((size_t)plan.entries * RW * 4)) return st;
    if (int st = stage.ensure(bases.size() * 4)) return st;
    MSMZ_HIP(hipMemcpyAsync(stage.p, bases.data(), bases.size() * 4, hipMemcpyHostToDevice, core_.stream_));
    hipLaunchKernelGGL((k_fixed_table<P>), Core::blocks_of(plan.entries), dim3(kBlock), 0, core_.stream_,
                       ft.mem.template as<uint32_t>(), stage.template as<const uint32_t>(), (uint32_t)plan.entries, plan.c);
    // (`bases` is pageable: the copy has left it when the call returns; the wait keeps the cache free of a table whose
    // build failed, and frees the entry that leaves with nothing in flight)
    if (int st = core_.drained()) return st;
    fixed_built_++;
    if (fixed_cache_.size() == FIXED_CACHE) fixed_cache_.pop_front();
    fixed_cache_.push_back(std::move(ft));
    *table = fixed_cache_.back().mem.template as<const uint32_t>();
    return MSMZ_OK;
  }

  Core& core_;
  DevBuf check_;                        // check_points: its result record, then one verdict byte per point
  std::deque<FixedTable> fixed_cache_;  // points_fixed_base: the window tables of the last FIXED_CACHE (base, c, K)
  uint64_t fixed_built_ = 0;            // ... the tables built so far, and the forced window width (0 = the planner's)
  int fixed_window_ = 0;
};

}  // namespace msmz

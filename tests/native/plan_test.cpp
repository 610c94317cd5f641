// The planner (msm_zprize_amd/csrc/plan.h) against a frozen copy of the planning code engine.h had before it moved
// there, over a sweep of every input a plan depends on: the four scalar fields, sizes 1 .. 2^25 (powers of two +- 1 and
// odd sizes), window sizes 0 (automatic) and 2..24, GLV on / off with both scalar bit lengths and several assumed GLV
// lengths, batches, precomputed sets of F windows per bucket set, fold allowed or not, tree rounds or not, and the
// default knobs plus each planning knob flipped on its own.  Compared: make_plan's status and Plan, the sort layout
// (SortGeom, bins, k_fine's top bin, specialized window size, two-level or fallback), plan chunks, the 2-D split, the
// first reduction group, batch_size and precompute_params.  Also asserted: a folded plan is two-level; a shape
// precompute_params accepts plans two-level for the assumed and the proven GLV bit length; a sub-batch of batch_size
// fits kMaxBatchEntries; a two-level layout has at most SORT_MAX_BINS bins; the invariants of the 2-D reduction's
// geometry (r2_geom_cases).  Exit code = number of mismatches.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/plan.h"
using namespace msmz;

namespace old {
// the Plan of commit 79707f1: planner output plus the engine's run state (timing, device totals, copy stride, events)
struct Plan {
  uint32_t n, M, L, nb, nblocks;
  int c, K, b;
  int Keff, spread;
  int fold_shift = 0, fold_rows = 0;
  uint32_t top_range = 1;
  bool glv, timing;
  uint32_t max_bucket = 0, n_entries = 0;
  uint32_t endo_delta = 0;
  uint32_t nprob = 1;
  uint32_t F = 1;
  uint32_t copy_stride = 0;
  int ei = 0;
  int ev_coarse = -1, ev_sort_end = -1;
};

// engine.h's planning members as they were at commit 79707f1 (in Engine<Cfg>; knobs were members, TE = twisted Edwards)
template <class Fr, bool TE>
struct Engine {
  bool no_spread_ = false, no_fold_ = false, no_fbt_ = false, no_window_model_ = false, force_atomic_sort_ = false;
  bool no_plan_top_ = false, no_sort_special_ = false;
  int fb_cap_ = 0;
  uint32_t s1_override_ = 0, r2_nc_ = 0;
  int glv_bits_assumed_ = 0;
  static constexpr int kMaxWindows = 128;
  static constexpr uint64_t kMaxBatchEntries = 1ull << 26;
  struct Handle {
    uint64_t n;
    uint32_t factor;
  };

  int scalar_bits(bool glv, int extra_bits) const {
    if (!glv) return Fr::BITS;
    if (extra_bits) return Fr::GLV_PROVEN_BITS > Fr::GLV_BITS - 1 ? Fr::GLV_PROVEN_BITS : Fr::GLV_BITS - 1;
    return glv_bits_assumed_ > 0 ? glv_bits_assumed_ : Fr::GLV_BITS - 1;
  }

  int precompute_params(uint64_t n, const msmz_opts* o, uint32_t factor, int* c_out, int* glv_out,
                        uint32_t* f_out, int* k_out) const {
    if (TE) return MSMZ_ERR_UNSUPPORTED;   // twisted Edwards runs msmBasic: no batched-affine buckets to share
    if (n == 0 || factor == 1) return MSMZ_ERR_ARG;
    msmz_opts opt;
    memset(&opt, 0, sizeof(opt));
    if (o) opt = *o; else opt.glv = -1;
    if (opt.buckets == MSMZ_BUCKETS_PROJECTIVE || opt.reserved[0] == 1) return MSMZ_ERR_UNSUPPORTED;
    if (opt.c < 0 || opt.c > 24) return MSMZ_ERR_ARG;
    int glv = opt.glv;
    if (glv < 0) glv = default_glv(n) ? 1 : 0;   // msm()'s choice for n points
    if (glv && !Fr::HAS_GLV) return MSMZ_ERR_UNSUPPORTED;
    glv = glv ? 1 : 0;
    const uint64_t M64 = glv ? 2 * n : n;
    if (M64 > (1ull << 24)) return MSMZ_ERR_ARG;
    const uint32_t M = (uint32_t)M64;
    const int b0 = scalar_bits(glv != 0, 0), b1 = scalar_bits(glv != 0, 1);
    // window size: the user's, or the model's for F copies (0: all windows in one set)
    int c = opt.c;
    auto windows = [&](int cc, int b) { return (b + 1 + cc - 1) / cc; };
    if (c == 0) c = choose_window_pre(glv != 0, M, b0, 1, factor == 0 ? 1024u : factor);
    if (c < 2) c = 2;
    const int K0 = windows(c, b0), K1 = windows(c, b1);
    const int Kmax = K0 > K1 ? K0 : K1;
    const uint32_t copies = factor == 0 || factor > (uint32_t)Kmax ? (uint32_t)Kmax : factor;
    if (copies < 2) return MSMZ_ERR_ARG;
    if (!pre_fits(c, glv != 0, M, b0, copies) || !pre_fits(c, glv != 0, M, b1, copies)) return MSMZ_ERR_ARG;
    const uint64_t records = (uint64_t)copies * n * (glv ? 2 : 1);
    if (records >= (1ull << 30)) return MSMZ_ERR_ARG;   // location words: 30-bit record index
    *c_out = c;
    *glv_out = glv;
    *f_out = copies;
    if (k_out) *k_out = K0;
    return MSMZ_OK;
  }

  static bool default_glv(uint64_t n) { return !TE && Fr::HAS_GLV && n < (1ull << 15); }

  uint32_t batch_size(const Handle& pts, uint64_t n, const msmz_opts& opt, uint32_t remaining) {
    uint32_t bs = remaining;
    for (int it = 0; it < 4 && bs > 1; it++) {
      Plan pl;
      if (make_plan(pl, n, opt.glv != 0, opt, (uint32_t)pts.n, true, 0, true, bs, pts.factor > 1 ? pts.factor : 1) != MSMZ_OK) {
        bs = (bs + 1) / 2;
        continue;
      }
      const uint32_t fit = batch_split(remaining, (uint64_t)pl.K * pl.M, kMaxBatchEntries);
      if (fit >= bs) break;
      bs = fit;
    }
    return bs;
  }

  // Window geometry for window size c: K windows, L buckets each, significant bits t_top of the top window's
  // digit (from the largest scalar q - 1, or the typical GLV half), and the 2^spread sub-windows the top window
  // is spread over when it is sparse.
  struct Geometry {
    int c, K, t_top, spread, Keff;
    uint32_t L;
    uint32_t top_range = 0;   // number of values the top window's digit can take (<= L + 1)
    int fold_shift = 0, fold_rows = 0;   // thin top window folded into its own bucket set (sort_kernels.h SortGeom)
  };
  Geometry geometry(int c, bool glv, uint32_t M, int b, bool allow_fold = false, uint32_t F = 1) const {
    Geometry g;
    g.c = c;
    g.K = (b + 1 + c - 1) / c;                              // msm-batched-affine.ts:96
    g.L = 1u << (c - 1);
    const int pos = (g.K - 1) * c;
    g.t_top = b + 1 - pos;
    if (!glv) {
      uint64_t top = 0;
      for (int j = 0; j < 64 && pos + j < 256; j++)
        top |= (uint64_t)((Fr::Q[(pos + j) >> 5] >> ((pos + j) & 31)) & 1u) << j;
      top += 1;   // carry from the window below
      g.t_top = ceil_log2_u64(top + 1);
      g.top_range = (uint32_t)(top + 1 > g.L ? g.L : top + 1);
    } else if (Fr::GLV_TYP_BITS + 1 - pos < g.t_top) {
      g.t_top = Fr::GLV_TYP_BITS + 1 - pos;
      if (g.t_top < 1) g.t_top = 1;
    }
    g.spread = 0;
    {
      // a thin top window whose digit fits the COLUMN index of the two-dimensional reduction (l < D = 2^b2) is folded:
      // 2^(c-1-b2) copies of the digit's range fill the set's buckets as evenly as any other window's.  The bound on
      // the digit is the hard one (largest scalar; for GLV halves the bit length the windows were sized for).
      const int b2 = (c - 1) - (c - 1 + 1) / 2;                       // low bits of Split2d
      const int t_bound = glv ? b + 1 - pos : g.t_top;
      // (only where the two-level sort applies: the fallback sort numbers buckets by digit alone)
      const uint32_t ncb0 = g.L >> fine_bits(c, M);
      const bool sort2 = !force_atomic_sort_ && M <= (1u << 24) && ncb0 <= (uint32_t)COARSE_MAX_BINS &&
                         (uint64_t)g.K * ncb0 <= (uint64_t)SORT_MAX_BINS;
      if (F == 1 && allow_fold && !no_fold_ && sort2 && g.K > 1 && g.t_top <= c - 2 && b2 >= 1 && t_bound <= b2) {
        g.fold_shift = b2;
        g.fold_rows = c - 1 - b2;
      }
    }
    // (precomputed sets, F > 1: neither -- the top window shares its bucket set with F - 1 windows; choose_window keeps
    // it from being thin)
    if (F == 1 && g.fold_shift == 0 && !no_spread_ && g.K > 1 && g.t_top <= c - 2) {
      g.spread = c - 1 - g.t_top;
      if (g.spread > 3) g.spread = 3;
      const int ib = ceil_log2_u64(M < 2 ? 2 : M);
      (void)ib;
      const int fbx = fine_bits(c, M);
      while (g.spread > 0 && ((g.L >> fbx) << g.spread) > (uint32_t)COARSE_MAX_BINS) g.spread--;
    }
    if (g.top_range == 0) g.top_range = g.t_top >= c - 1 ? g.L : 1u << g.t_top;
    g.Keff = g.K - 1 + (1 << g.spread);
    return g;
  }

  // Fine bits of the two-level sort = log2(buckets per coarse bin): as many as (1) the packed word leaves beside the
  // index and the sign, (2) k_fine's counters hold, and (3) keep an average bin inside k_fine's LDS staging (a bin of
  // 2^fb buckets holds ~M 2^fb / L entries; beyond FINE_STAGE it falls back to scattered stores: 3x slower).
  // Precomputed sets (W = windows per bucket set > 1): a set receives W M entries and the packed index carries the copy
  // (copy_bits(W) more bits); fb is then raised again, if the index leaves room, until a window has <= COARSE_MAX_BINS
  // bins (k_fine sorts a denser bin unstaged); -1 when even that does not fit.
  int fine_bits(int c, uint32_t M, uint32_t W = 1) const {
    const int idx_bits = ceil_log2_u64(M < 2 ? 2 : M) + copy_bits(W);
    int fb = 31 - idx_bits;
    if (fb > FINE_MAX_BITS) fb = FINE_MAX_BITS;
    if (fb_cap_ > 0 && fb > fb_cap_) fb = fb_cap_;
    if (fb > c - 1) fb = c - 1;
    const int fb_max = fb;
    const uint64_t L = 1ull << (c - 1);
    while (fb > 0 && ((((uint64_t)M * W) << fb) / L) * 10 > (uint64_t)FINE_STAGE * 9) fb--;
    if (W > 1) {
      while (fb < fb_max && (L >> fb) > (uint64_t)COARSE_MAX_BINS) fb++;
      if ((L >> fb) > (uint64_t)COARSE_MAX_BINS || fb < 0) return -1;
    }
    return fb;
  }
  // windows per bucket set of a plan
  static uint32_t set_windows(const Plan& pl) { return pl.F < (uint32_t)pl.K ? pl.F : (uint32_t)pl.K; }

  // Fine bits of the TOP window's bins (SortGeom::fbt): its entries fall on top_range << spread buckets only (the largest
  // scalar bounds the top digit), so they are up to 2x denser than M / L; as many fine bits as keep such a bin inside
  // k_fine's staging, and no fewer than keep the window's bins inside k_coarse's 9-bit bin field.
  int fine_bits_top(const Plan& pl, int fb) const {
    if (pl.fold_shift != 0 || no_fbt_ || pl.F > 1) return fb;
    const uint64_t slots = (uint64_t)pl.top_range << pl.spread;
    int fbt = fb;
    while (fbt > 0 && (((uint64_t)pl.M << fbt) / slots) * 10 > (uint64_t)FINE_STAGE * 9) fbt--;
    while (fbt < fb && ((pl.L >> fbt) << pl.spread) > (uint32_t)COARSE_MAX_BINS) fbt++;
    return fbt;
  }

  // Default window size.  Large inputs (M >= 2^18: profiles/r03_sweep.json) are throughput-bound: c = log2 M - 3 capped at 17, stepped
  // down while the top window would be nearly empty.  Smaller inputs are latency-bound -- every tree round costs
  // ~75 us whatever its size and the number of rounds is log2 of the LONGEST bucket, which usually sits in a
  // partly filled top window -- so they pick the c that minimizes a small cost model fitted to this GPU
  // (ms: rounds * 0.075 + additions / 4.5e6 + reduction levels * 0.065 + buckets * 0.8e-6).
  // A batch of B problems runs the same number of tree rounds and reduction levels as one, with B times the additions
  // and buckets: those two terms of the model are scaled by B.
  // Precomputed point sets (F > 1 windows per bucket set): the same model at every size, over the
  // window sizes whose sets fit one sort pass, with ceil(K / F) bucket sets, buckets W = min(F, K) times longer, and the
  // top window's concentration on its few digits (it shares a set, it is neither spread nor folded).
  int choose_window(bool glv, uint32_t M, int b, bool tree_rounds, uint32_t nprob = 1, uint32_t F = 1) const {
    if (F > 1) return choose_window_pre(glv, M, b, nprob, F);
    int c = default_window(M);
    if (M >= (1u << 18) || no_window_model_) {
      // measured optimum of the batched-affine path from 2^18 entries per window on (profiles/r03_sweep.json): 17 without
      // GLV (2^18: 1.60 ms against 1.83 at c = 15), 16 with it (128-bit halves = 8 windows exactly)
      if (tree_rounds && !no_window_model_) c = glv ? 16 : 17;
      for (int tries = 0; tries < 3 && c > 4; tries++) {
        const int K0 = (b + 1 + c - 1) / c;
        const int top_bits = b + 1 - (K0 - 1) * c;
        if (K0 == 1 || top_bits >= c - 4) break;
        c--;
      }
      return c;
    }
    const int lg = ceil_log2_u64(M < 2 ? 2 : M);
    int best_c = c;
    double best = 1e30;
    for (int cc = (lg - 6 < 3 ? 3 : lg - 6); cc <= (lg + 2 > 17 ? 17 : lg + 2); cc++) {
      const Geometry g = geometry(cc, glv, M, b);
      if (g.Keff > kMaxWindows) continue;
      const double lam = (double)M / g.L;
      const double conc = g.t_top < cc ? (double)(1u << (cc - g.t_top)) / (1 << g.spread) : 1.0;
      double maxb = 1.5 * lam + 12;
      if (g.K > 1 && conc * lam * 1.3 + 12 > maxb) maxb = conc * lam * 1.3 + 12;
      if (maxb > M) maxb = M;
      const int rounds = ceil_log2_u64((uint64_t)(maxb < 2 ? 2 : maxb));
      const double cost = (tree_rounds ? 0.075 * rounds : 0.0) + (double)nprob * g.K * M / 4.5e6 +
                          0.065 * ((cc - 1 + 1) / 2) + 0.8e-6 * nprob * g.Keff * g.L;
      if (cost < best) {
        best = cost;
        best_c = cc;
      }
    }
    return best_c;
  }

  // does a window size fit a precomputed set's sort (F windows per set; the two-level sort only)?
  bool pre_fits(int c, bool glv, uint32_t M, int b, uint32_t F) const {
    const Geometry g = geometry(c, glv, M, b, false, F);
    const uint32_t W = F < (uint32_t)g.K ? F : (uint32_t)g.K;
    const int fb = fine_bits(c, M, W);
    if (fb < 0 || g.K > kMaxWindows || M > (1u << 24)) return false;
    // one bucket collects the entries of all W windows of its set (every digit equal in the worst case): the tree rounds
    // take buckets below 2^PLAN_RMAX entries
    if ((uint64_t)W * M >= (1ull << PLAN_RMAX)) return false;
    const uint32_t ncb = g.L >> fb;
    return ncb <= (uint32_t)COARSE_MAX_BINS && (uint64_t)g.K * ncb <= (uint64_t)SORT_MAX_BINS;
  }
  int choose_window_pre(bool glv, uint32_t M, int b, uint32_t nprob, uint32_t F) const {
    // measured (profiles/r05_precompute_c_sweep.jsonl): with every window in one set and >= 2^16 entries per window, c = 17
    // is the fastest fitting size (2^16: 0.86 ms against 0.94 at c = 16, 16 x 2^16: 3.26 against 3.43, 2^20: 3.62 against
    // 3.99); with fewer windows per set the model below is (16 x 2^16, F = 2: c = 15 5.98 ms, c = 17 7.76)
    if (!glv && M >= (1u << 16) && F >= (uint32_t)geometry(17, false, M, b, false, F).K && pre_fits(17, false, M, b, F))
      return 17;
    int best_c = 0;
    double best = 1e30;
    for (int cc = 3; cc <= 20; cc++) {
      if (!pre_fits(cc, glv, M, b, F)) continue;
      const Geometry g = geometry(cc, glv, M, b, false, F);
      const uint32_t W = F < (uint32_t)g.K ? F : (uint32_t)g.K;
      const int sets = (g.K + (int)W - 1) / (int)W;
      const int w_top = g.K - (sets - 1) * (int)W;   // windows in the top window's set
      const double lam = (double)M * W / g.L;
      double maxb = 1.5 * lam + 12;
      const double top = 1.3 * (double)M / (g.top_range < 1 ? 1 : g.top_range) + (double)(w_top - 1) * M / g.L + 12;
      if (g.K > 1 && top > maxb) maxb = top;
      if (maxb > (double)M * W) maxb = (double)M * W;
      const int rounds = ceil_log2_u64((uint64_t)(maxb < 2 ? 2 : maxb));
      const double cost = 0.075 * rounds + (double)nprob * g.K * M / 4.5e6 + 0.065 * ((cc - 1 + 1) / 2) +
                          0.8e-6 * nprob * sets * g.L;
      if (cost < best) {
        best = cost;
        best_c = cc;
      }
    }
    return best_c > 0 ? best_c : default_window(M);
  }

  int make_plan(Plan& pl, uint64_t n64, bool glv, const msmz_opts& opt, uint32_t pts_n, bool tree_rounds = true,
                int extra_bits = 0, bool allow_fold = false, uint32_t nprob = 1, uint32_t F = 1) {
    pl.n = (uint32_t)n64;
    pl.nprob = nprob;
    pl.glv = glv;
    pl.M = glv ? 2 * pl.n : pl.n;
    // scalar bit length.  GLV halves: first attempt assumes |s_j| < 2^127 (every half seen so far; for BLS12-377 the
    // analytic bound is 2^126); k_hist flags a longer half and the MSM is redone (extra_bits = 1) with the proven bound
    // GLV_PROVEN_BITS <= 128, which also is what the 4-word halves of glv_decompose can hold.
    static_assert(!Fr::HAS_GLV || (Fr::GLV_PROVEN_BITS <= 128 && Fr::GLV_PROVEN_BITS <= Fr::GLV_BITS), "GLV halves must fit 4 words");
    pl.b = scalar_bits(glv, extra_bits);
    pl.c = opt.c > 0 ? opt.c : choose_window(glv, pl.M, pl.b, tree_rounds, nprob, F);
    if (pl.c < 2) pl.c = 2;
    if (pl.c > 24) pl.c = 24;
    pl.F = F < 1 ? 1 : F;
    const Geometry g = geometry(pl.c, glv, pl.M, pl.b, allow_fold, pl.F);
    pl.K = g.K;
    pl.L = g.L;
    pl.spread = g.spread;
    pl.top_range = g.top_range;
    pl.fold_shift = g.fold_shift;
    pl.fold_rows = g.fold_rows;
    pl.Keff = g.Keff;
    if (pl.F > 1) pl.Keff = (pl.K + (int)set_windows(pl) - 1) / (int)set_windows(pl);   // bucket sets
    const uint64_t nb64 = (uint64_t)pl.Keff * pl.L;
    if (nb64 * nprob + 1 >= (1ull << 31) || (uint64_t)nprob * pl.K * pl.M >= (1ull << 32) || pl.Keff > kMaxWindows)
      return MSMZ_ERR_ARG;
    pl.nb = (uint32_t)nb64;
    pl.nblocks = (pl.nb + SCAN_TILE - 1) / SCAN_TILE;
    pl.timing = opt.timing != 0;
    pl.endo_delta = glv ? pts_n - pl.n : 0u;
    return MSMZ_OK;
  }

  // does the two-level LDS-staged sort apply to this plan (else the per-entry atomic fallback)?
  bool sort2_applies(const Plan& pl) const {
    const int fb = fine_bits(pl.c, pl.M, set_windows(pl));
    if (fb < 0) return false;
    const uint32_t ncb = pl.L >> fb;
    const uint32_t ncbt = pl.L >> fine_bits_top(pl, fb);
    const uint32_t nbins = (uint32_t)(pl.K - 1) * ncb + (ncbt << pl.spread);
    return !force_atomic_sort_ && fb >= 0 && pl.M <= (1u << 24) && ncb <= (uint32_t)COARSE_MAX_BINS &&
           (ncbt << pl.spread) <= (uint32_t)COARSE_MAX_BINS && nbins <= (uint32_t)SORT_MAX_BINS;
  }

  uint32_t first_group_size(const Plan& pl) const {
    if (s1_override_ > 0) return s1_override_ < pl.L ? s1_override_ : pl.L;
    uint32_t S1 = 2;
    // L / S1 a power of 4 saves one reduction level; with >= 2^20 buckets groups of 8 still fill the GPU
    // (2 waves per SIMD) and halve the levels above (measured: S1 = 4 -> 1.58 ms, 8 -> 1.45 ms, 16 -> 1.94 ms)
    if (pl.L >= 4 && (ceil_log2_u64(pl.L) & 1) == 0) S1 = 4;
    if ((uint64_t)pl.Keff * pl.L >= (1u << 20) && pl.L >= 8) S1 = 8;
    return S1 < pl.L ? S1 : pl.L;
  }

  struct Split2d {
    int a, b;            // c - 1 = a + b: high / low bits of the bucket weight
    uint32_t H, D, NC;
  };
  Split2d split_2d(const Plan& pl) const {
    Split2d s;
    s.a = (pl.c - 1 + 1) / 2;
    s.b = pl.c - 1 - s.a;
    s.H = 1u << s.a;
    s.D = 1u << s.b;
    // chunks per line: so that the partial sums of all lines are ~256 K threads (measured at 2^20: 16 / 32 / 64 chunks ->
    // reduce stage 0.88 / 0.81 / 0.81 ms), at most 32 per line (5 pair-sum launches), and a chunk holds at least one
    // bucket along either direction
    uint32_t nc = 1;
    while (nc < 32 && nc * 2 <= s.D && (uint64_t)2 * pl.nprob * pl.Keff * s.H * nc < (1u << 18)) nc *= 2;
    if (r2_nc_ > 0) {
      nc = 1;
      while (nc < r2_nc_ && nc * 2 <= s.D) nc *= 2;
    }
    s.NC = nc;
    return s;
  }


  // the layout the sort stage once computed inline (its two-level branch)
  struct Sort {
    bool sort2;
    SortGeom g;
    uint32_t nbins, fbins, fine_top;
    int cspec;
  };
  Sort sort(const Plan& pl) const {
    Sort r;
    memset(&r, 0, sizeof(r));
    const uint32_t M = pl.M, L = pl.L, n = pl.n;
    const int c = pl.c, K = pl.K;
    const uint32_t W = set_windows(pl);
    const int mbits = ceil_log2_u64(M < 2 ? 2 : M);
    const int idx_bits = mbits + copy_bits(W);
    r.sort2 = sort2_applies(pl);
    if (!r.sort2) return r;
    const int fb = r.sort2 ? fine_bits(c, M, W) : fine_bits(c, M);
    const uint32_t ncb = L >> fb;
    const int fbt = fine_bits_top(pl, fb);
    const uint32_t ncbt = L >> fbt;
    const uint32_t top_bin = (uint32_t)(K - 1) * ncb;
    const uint32_t nbins = top_bin + (ncbt << pl.spread);   // tile-local bins (per window)
    const uint32_t sbins = pl.F > 1 ? (uint32_t)pl.Keff * W * ncb : nbins;   // scanned bins per problem
    const uint32_t fbins = pl.F > 1 ? (uint32_t)pl.Keff * ncb : nbins;       // k_fine's bins per problem
    r.g = SortGeom{n, M, c, K, fb, pl.spread, idx_bits, ncb, fbt, ncbt, pl.fold_shift, pl.fold_rows, W, mbits, sbins};
    r.nbins = nbins;
    r.fbins = fbins;
    r.fine_top = pl.F > 1 ? fbins - ncb : top_bin;
    r.cspec = (no_sort_special_ || (c != 16 && c != 17) || (pl.glv && c != 16)) ? 0 : c;
    return r;
  }

  // msm_weierstrass_affine's plan chunks
  PlanChunks chunks(const Plan& pl, uint32_t nprob, uint32_t* n_chunks) const {
    const uint32_t nb = pl.nb * nprob;
    uint32_t chunk = PLAN_CHUNK;
    while (chunk > 64 && (nb + chunk - 1) / chunk < 1024) chunk >>= 1;
    PlanChunks pc;
    pc.chunk = chunk;
    pc.nb_main = nb;
    pc.chunk_top = chunk;
    if (!no_plan_top_ && nprob == 1 && pl.F == 1 && pl.K > 1 && pl.fold_shift == 0 && chunk >= 128 &&
        (uint64_t)pl.L * 10 > ((uint64_t)pl.top_range << pl.spread) * 13) {
      pc.nb_main = (uint32_t)(pl.K - 1) * pl.L;
      pc.chunk_top = chunk / 2;
    }
    pc.n_main = (pc.nb_main + chunk - 1) / chunk;
    *n_chunks = pc.n_main + (nb - pc.nb_main + pc.chunk_top - 1) / pc.chunk_top;
    return pc;
  }
};
}  // namespace old

static int bad = 0;
static long shapes = 0;

static void mismatch(const char* what, const char* fr, uint64_t n, int c, int glv, int e, int knob, uint32_t nprob,
                     uint32_t F) {
  if (bad++ < 20)
    printf("mismatch %s: %s n %llu c %d glv %d extra %d knob %d nprob %u F %u\n", what, fr, (unsigned long long)n, c, glv,
           e, knob, nprob, F);
}

// every field of the planner's Plan (the old one's run state is no longer planner output)
static bool same_plan(const Plan& a, const old::Plan& b) {
  return a.n == b.n && a.M == b.M && a.L == b.L && a.nb == b.nb && a.nblocks == b.nblocks && a.c == b.c && a.K == b.K &&
         a.b == b.b && a.Keff == b.Keff && a.spread == b.spread && a.fold_shift == b.fold_shift &&
         a.fold_rows == b.fold_rows && a.top_range == b.top_range && a.glv == b.glv && a.endo_delta == b.endo_delta &&
         a.nprob == b.nprob && a.F == b.F;
}

static bool same_geom(const SortGeom& a, const SortGeom& b) {
  return a.n == b.n && a.M == b.M && a.c == b.c && a.K == b.K && a.fb == b.fb && a.spread == b.spread &&
         a.idx_bits == b.idx_bits && a.ncb == b.ncb && a.fbt == b.fbt && a.ncbt == b.ncbt && a.fold_shift == b.fold_shift &&
         a.fold_rows == b.fold_rows && a.F == b.F && a.mbits == b.mbits && a.sbins == b.sbins;
}

constexpr int kKnobs = 11;   // 0 = defaults, 1..10 = one planning knob flipped

template <class Fr, bool TE>
static void set_knob(int i, PlanKnobs& k, old::Engine<Fr, TE>& o) {
  switch (i) {
    case 1: k.no_spread = o.no_spread_ = true; break;
    case 2: k.no_fold = o.no_fold_ = true; break;
    case 3: k.no_fbt = o.no_fbt_ = true; break;
    case 4: k.no_window_model = o.no_window_model_ = true; break;
    case 5: k.force_atomic_sort = o.force_atomic_sort_ = true; break;
    case 6: k.no_plan_top = o.no_plan_top_ = true; break;
    case 7: k.no_sort_special = o.no_sort_special_ = true; break;
    case 8: k.fb_cap = o.fb_cap_ = 7; break;
    case 9: k.s1_override = o.s1_override_ = 16; break;
    case 10: k.r2_nc = o.r2_nc_ = 4; break;
    default: break;
  }
}

template <class Fr, bool TE>
static void replay(const char* name) {
  std::vector<uint64_t> sizes = {3, 5, 7, 11, 1000, 12345, 100003, 1234567, 3000001, 20000001};
  for (int k = 0; k <= 25; k++)
    for (int64_t d = -1; d <= 1; d++)
      if ((1ull << k) + d >= 1) sizes.push_back((1ull << k) + d);
  struct GlvCase {
    int glv, extra, assumed;
  };
  std::vector<GlvCase> glvs = {{0, 0, 0}, {0, 1, 0}};
  if (Fr::HAS_GLV)
    for (GlvCase g : {GlvCase{1, 1, 0}, GlvCase{1, 0, 0}, GlvCase{1, 0, 8}, GlvCase{1, 0, 64}, GlvCase{1, 0, Fr::GLV_BITS - 1}})
      glvs.push_back(g);
  for (int knob = 0; knob < kKnobs; knob++)
    for (const GlvCase& gc : glvs) {
      Planner<Fr> np;
      old::Engine<Fr, TE> op;
      set_knob(knob, np.k, op);
      np.k.glv_bits_assumed = op.glv_bits_assumed_ = gc.assumed;
      const bool glv = gc.glv != 0;
      if (np.scalar_bits(glv, gc.extra) != op.scalar_bits(glv, gc.extra)) mismatch("scalar_bits", name, 0, 0, gc.glv, gc.extra, knob, 1, 1);
      for (uint64_t n : sizes) {
        if (np.default_glv(n) != op.default_glv(n)) mismatch("default_glv", name, n, 0, gc.glv, gc.extra, knob, 1, 1);
        const uint32_t pts_n = (uint32_t)(n + (n & 3));
        for (int c = 0; c <= 24; c++) {
          if (c == 1) continue;
          msmz_opts opt;
          memset(&opt, 0, sizeof(opt));
          opt.c = c;
          opt.glv = gc.glv;
          opt.timing = (int)(n & 1);
          auto check = [&](bool tree, bool fold, uint32_t nprob, uint32_t F) {
            Plan a{};
            old::Plan b{};
            const int sa = np.make_plan(a, n, glv, opt, pts_n, tree, gc.extra, fold, nprob, F);
            const int sb = op.make_plan(b, n, glv, opt, pts_n, tree, gc.extra, fold, nprob, F);
            shapes++;
            if (sa != sb || !same_plan(a, b)) return mismatch("make_plan", name, n, c, gc.glv, gc.extra, knob, nprob, F);
            if (sa != MSMZ_OK) return;
            const SortLayout sl = np.sort_layout(a);
            const auto os = op.sort(b);
            if (sl.two_level != os.sort2) return mismatch("two_level", name, n, c, gc.glv, gc.extra, knob, nprob, F);
            if (sl.two_level && (!same_geom(sl.geom, os.g) || sl.nbins != os.nbins || sl.fbins != os.fbins ||
                                 sl.fine_top != os.fine_top || sl.cspec != os.cspec))
              return mismatch("sort layout", name, n, c, gc.glv, gc.extra, knob, nprob, F);
            if (a.fold_shift != 0 && !sl.two_level) mismatch("folded plan on the fallback sort", name, n, c, gc.glv, gc.extra, knob, nprob, F);
            if (sl.two_level && sl.nbins > (uint32_t)SORT_MAX_BINS) mismatch("nbins > SORT_MAX_BINS", name, n, c, gc.glv, gc.extra, knob, nprob, F);
            uint32_t onc = 0;
            const PlanChunks pa = np.plan_chunks(a), pb = op.chunks(b, nprob, &onc);
            if (pa.chunk != pb.chunk || pa.nb_main != pb.nb_main || pa.n_main != pb.n_main || pa.chunk_top != pb.chunk_top ||
                pa.n_main + (a.nb * nprob - pa.nb_main + pa.chunk_top - 1) / pa.chunk_top != onc)
              return mismatch("plan chunks", name, n, c, gc.glv, gc.extra, knob, nprob, F);
            const Split2d xa = np.split_2d(a);
            const auto xb = op.split_2d(b);
            if (xa.a != xb.a || xa.b != xb.b || xa.H != xb.H || xa.D != xb.D || xa.NC != xb.NC)
              return mismatch("split_2d", name, n, c, gc.glv, gc.extra, knob, nprob, F);
            if (np.first_group_size(a) != op.first_group_size(b))
              return mismatch("first_group_size", name, n, c, gc.glv, gc.extra, knob, nprob, F);
          };
          for (int tree = 0; tree < 2; tree++)
            for (int fold = 0; fold < 2; fold++) check(tree != 0, fold != 0, 1, 1);
          // batches and precomputed sets run with tree rounds and the fold allowed (msm_batch, msm_weierstrass_affine)
          Plan p0{};
          const int K0 = np.make_plan(p0, n, glv, opt, pts_n) == MSMZ_OK ? p0.K : 4;
          for (uint32_t nprob : {1u, 2u, 3u, 16u, 64u, 1000u})
            for (uint32_t F : {1u, 2u, 3u, 5u, (uint32_t)K0, 1024u})
              if (nprob > 1 || F > 1) check(true, true, nprob, F);
          // sub-batches
          if (!TE && gc.extra == 0 && n * (glv ? 2 : 1) <= kMaxEntriesPerPass)
            for (uint32_t factor : {0u, 2u, 3u, 5u, 1024u})
              for (uint32_t rem : {2u, 3u, 16u, 64u, 1000u}) {
                const uint32_t bs = np.batch_size(n, opt, pts_n, factor, rem);
                shapes++;
                if (bs != op.batch_size(typename old::Engine<Fr, TE>::Handle{pts_n, factor}, n, opt, rem)) {
                  mismatch("batch_size", name, n, c, gc.glv, 0, knob, rem, factor);
                  continue;
                }
                // A sub-batch whose plan cannot be made (too many buckets at a large c) fails in make_plan.  Known gap,
                // kept as it is: batch_size re-plans at most four times, and a sub-batch it reached by halving one whose
                // plan could not be made is not checked again (e.g. 1000 problems of 2^20 points at c = 5 -> 63).
                Plan p{}, q{};
                const uint32_t F1 = factor > 1 ? factor : 1;
                if (bs > 1 && np.make_plan(p, n, glv, opt, pts_n, true, 0, true, bs, F1) == MSMZ_OK &&
                    (uint64_t)bs * p.K * p.M > kMaxBatchEntries &&
                    np.make_plan(q, n, glv, opt, pts_n, true, 0, true, 2 * bs, F1) == MSMZ_OK)
                  mismatch("sub-batch beyond kMaxBatchEntries", name, n, c, gc.glv, 0, knob, bs, factor);
              }
          // precomputed sets
          if (gc.extra == 0)
            for (int og : {-1, 0, 1}) {
              if (og != gc.glv && !(og == -1 && gc.glv == 0)) continue;   // (-1: once per assumed length)
              for (uint32_t factor : {0u, 1u, 2u, 3u, 5u, (uint32_t)K0, 1024u}) {
                msmz_opts po;
                memset(&po, 0, sizeof(po));
                po.c = c;
                po.glv = og;
                int c1 = -1, g1 = -1, k1 = -1, c2 = -1, g2 = -1, k2 = -1;
                uint32_t f1 = 0, f2 = 0;
                const int s1 = np.precompute_params(n, &po, factor, &c1, &g1, &f1, &k1);
                const int s2 = op.precompute_params(n, &po, factor, &c2, &g2, &f2, &k2);
                shapes++;
                if (TE) continue;   // (the engine refuses twisted Edwards before it asks the planner)
                if (s1 != s2 || c1 != c2 || g1 != g2 || f1 != f2 || k1 != k2) {
                  mismatch("precompute_params", name, n, c, og, 0, knob, 1, factor);
                  continue;
                }
                if (s1 != MSMZ_OK) continue;
                for (int e = 0; e < 2; e++) {
                  msmz_opts mo;
                  memset(&mo, 0, sizeof(mo));
                  mo.c = c1;
                  mo.glv = g1;
                  Plan p{};
                  if (np.make_plan(p, n, g1 != 0, mo, (uint32_t)n, true, e, true, 1, f1) != MSMZ_OK ||
                      !np.sort_layout(p).fits || (!np.k.force_atomic_sort && !np.sort_layout(p).two_level))
                    mismatch("precomputed set not two-level", name, n, c1, g1, e, knob, 1, f1);
                }
              }
            }
        }
      }
    }
}

// Planner::r2_geom, the 2-D reduction's kernel argument: the split of split_2d (with and without an r2_nc override) cut
// into whole chunks along both directions, two problems per bucket set of the batch
static void r2_geom_cases() {
  for (uint32_t nc : {0u, 1u, 4u, 64u})
    for (int c : {2, 3, 8, 9, 17})
      for (uint32_t nprob : {1u, 3u}) {
        Planner<Bls377Fr> pr;
        pr.k.r2_nc = nc;
        Plan pl{};
        pl.c = c;
        pl.L = 1u << (c - 1);
        pl.K = pl.Keff = 5;
        pl.nprob = nprob;
        pl.nb = (uint32_t)pl.Keff * pl.L;
        const Split2d sp = pr.split_2d(pl);
        const R2Geom g = pr.r2_geom(pl);
        shapes++;
        const bool split = g.L == pl.L && g.H == sp.H && g.D == sp.D && g.NC == sp.NC && g.H == 1u << ((c - 1 + 1) / 2);
        const bool whole = g.H * g.D == g.L && g.chr * g.NC == g.D && g.chc * g.NC == g.H && g.chr >= 1 && g.chc >= 1;
        const bool chunks = (g.NC & (g.NC - 1)) == 0 && g.NC <= g.D && (nc == 0 || g.NC == (nc < g.D ? nc : g.D));
        if (!split || !whole || !chunks || g.nprob != 2u * nprob * (uint32_t)pl.Keff)
          mismatch("r2_geom", "bls12-377", 0, c, 0, 0, (int)nc, nprob, 1);
      }
}

int main() {
  r2_geom_cases();
  replay<Bls377Fr, false>("bls12-377");
  replay<PallasFr, false>("pallas");
  replay<Bls381Fr, false>("bls12-381");
  replay<Ed377Fr, true>("ed-on-bls12-377");
  printf("shapes %ld mismatches %d\n", shapes, bad);
  return bad > 255 ? 255 : bad;
}

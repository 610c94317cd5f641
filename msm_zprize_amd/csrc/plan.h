// Host-only planning of an MSM (window size and geometry, sort layout, plan chunks, 2-D split, sub-batches, precomputed
// sets): engine.h asks a Planner and launches what it says; tests/native/plan_test.cpp runs it on a CPU.  Also the
// limits and POD argument structs that host and kernels share (the kernel headers include this file).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/msmz.h"
#include "multi.h"   // batch_split (host-only)

namespace msmz {

// ------------------------------------------------------------------------------------------------ kernel limits
// two-level bucket sort (sort_kernels.h)
constexpr int COARSE_T = 1024;
constexpr int COARSE_ITEMS = 2;                        // half-scalars (= entries per window) per thread
constexpr int COARSE_TILE = COARSE_T * COARSE_ITEMS;   // entries per window staged by one workgroup
constexpr int COARSE_MAX_BINS = 512;                   // bins per window (top window: incl. its sub-windows) the staging supports
constexpr int SORT_MAX_BINS = 8192;                    // all windows: k_coarse keeps 2 words per bin in LDS (64 KB)
constexpr int FINE_MAX_BITS = 11;
constexpr int FINE_T = 1024;
constexpr int FINE_PER = 37;                           // entries a thread holds in registers
constexpr int FINE_STAGE = FINE_T * FINE_PER;          // 37888 entries staged in LDS: 148 KB + 8 KB of counters (+ static) < 160 KB

// tree-round plan (plan_kernels.h)
constexpr int PLAN_T = 512;
constexpr int PLAN_PER = 2;                       // consecutive buckets per thread (counting / scan phases)
constexpr int PLAN_CHUNK = PLAN_T * PLAN_PER;     // buckets per workgroup
constexpr int PLAN_RMAX = 26;                     // rounds supported (bucket sizes < 2^26)

// three-launch exclusive scan (kernels.h)
constexpr int SCAN_T = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_T * SCAN_ITEMS;

struct SortGeom {
  uint32_t n;          // scalars
  uint32_t M;          // entries per window: n, or 2 n with GLV (entry n + i = endomorphism half of scalar i)
  int c, K, fb, spread, idx_bits;
  uint32_t ncb;        // coarse bins per bucket set = L >> fb
  // The TOP window's bucket sets may use fewer fine bits (fbt <= fb, ncbt = L >> fbt bins each): its digit range is not a
  // power of two, so its buckets are up to 2x denser than the other windows' and a bin of 2^fb of them would not fit
  // k_fine's LDS staging.  Bins of windows 0..K-2 come first (ncb each), then the top window's sub-windows (ncbt each).
  int fbt;
  uint32_t ncbt;
  // A THIN top window (its digit has only a few significant bits) can be FOLDED into its own bucket set instead of
  // spread over sub-windows: bucket weight j = (entry mod 2^fold_rows) * 2^fold_shift + l, i.e. the L buckets of the set
  // hold 2^fold_rows copies ("rows") of the digit's small range, and the two-dimensional reduction's COLUMN sums are
  // exactly the per-digit sums (the row result of that set is not used).  fold_shift = 0: not folded.
  int fold_shift, fold_rows;
  // Precomputed point sets (msmz_precompute_points): F windows share one bucket set.  Window k adds into set k / F and
  // references copy k mod F of the points, whose index rides in the packed word above the entry's `mbits` bits.  The
  // tile-local bins stay per window (k * ncb + coarse: the LDS layouts above are unchanged); only the GLOBAL bin order is
  // permuted (scan_bin) so that the F bins of one set with the same coarse value are adjacent and k_fine sorts them as one
  // bin.  `sbins` = scanned bins per problem (ceil(K / F) * F * ncb).  F = 1: the identity, sbins = nbins.
  uint32_t F;
  int mbits;
  uint32_t sbins;
  // Caller-given scalar bit bound (msmz_opts.reserved[1]): a scalar >= 2^sbits is flagged like one >= the group order
  // and contributes no digit.  256 = no bound.
  int sbits;
};

// One problem of a segmented MSM (msmz_msm_segments) as the sort kernels read it: its scalars are entries
// [first_s, first_s + n) of the scalar set, its points records [first_p, first_p + n) of the point set's base points.
struct SegDesc {
  uint32_t first_s, first_p, n;
};

// chunk_pairs[r * n_chunks + chunk] = pairs of round r in the chunk's buckets, r < PLAN_RMAX
// `chunk` <= PLAN_CHUNK buckets per workgroup (the host picks it so that there are enough workgroups for the GPU even
// when a window has few, long buckets).
// The buckets from `nb_main` on (the top window's bucket sets, up to 2x denser than the others) are cut into chunks of
// `chunk_top` <= chunk buckets, so that their workgroups do not outlast the rest (a launch ends with its slowest one).
struct PlanChunks {
  uint32_t chunk, nb_main, n_main, chunk_top;
};

struct R2Geom {
  uint32_t L, H, D;       // buckets per set, rows, columns (H * D = L, H >= D)
  uint32_t NC;            // chunks per line (power of two)
  uint32_t chr, chc;      // buckets per chunk along a row (D / NC) and along a column (H / NC)
  uint32_t nprob;         // 2 * Keff
};

// ------------------------------------------------------------------------------------------------ engine limits
constexpr int kMaxWindows = 128;
// Largest number of (half-)scalars one pass sorts: index + negate + fine bucket bits share a 32-bit word.
constexpr uint64_t kMaxEntriesPerPass = 1ull << 24;
// Entries (problems x windows x entries per window) one batched pass sorts, plans and adds: slots, descriptors and
// references cost ~100 B per entry (BLS12-377), so a batch beyond 2^26 entries (~7 GB) runs as consecutive
// sub-batches.  (2^26 also keeps the 30-bit location words and the 31-bit bucket numbers far from their limits.)
constexpr uint64_t kMaxBatchEntries = 1ull << 26;

static inline int copy_bits(uint32_t F) {   // bits of a copy index below F
  int r = 0;
  while ((1u << r) < F) r++;
  return r;
}

static inline int ceil_log2_u64(uint64_t x) {
  int r = 0;
  while (((uint64_t)1 << r) < x) r++;
  return r;
}

// default window size.  The reference's tables (msm-common.ts:8-57) were tuned for 16 CPU threads;
// on the GPU the accumulate phase costs ~N*K additions and the reduction ~2*K*2^(c-1), and the latter
// is latency-bound, so c stays well below log2(N).
static inline int default_window(uint64_t n_points) {
  int lg = ceil_log2_u64(n_points < 2 ? 2 : n_points);
  int c = lg - 3;
  if (c < 3) c = 3;
  if (c > 17) c = 17;   // 2^16 buckets per window: the largest the two-level LDS sort handles in one coarse pass
  return c;
}

struct Plan {
  uint32_t n, M, L, nb, nblocks;
  int c, K, b;
  int Keff, spread;           // bucket windows incl. the top window's 2^spread sub-windows
  int fold_shift = 0, fold_rows = 0;   // ... or the top window folded into its own bucket set (SortGeom)
  uint32_t top_range = 1;              // values the top window's digit can take
  bool glv;
  uint32_t endo_delta = 0;    // GLV over a prefix of a set: half-1 entry i reads point record pts_n + i = (n + i) + endo_delta
  uint32_t nprob = 1;         // batched MSM: problems (scalar vectors) sorted, planned and reduced together; nb, M, K,
                              // Keff describe ONE problem, bucket set p * Keff + kw holds window kw of problem p
  uint32_t F = 1;             // precomputed point set: windows per bucket set (Keff = ceil(K / F) sets); 1 = plain
  int sbits = 0;              // caller-given scalar bit bound, normalized (Planner::bound): 0 = none
};

// Window geometry for window size c: K windows, L buckets each, significant bits t_top of the top window's
// digit (from the largest scalar q - 1, or the typical GLV half), and the 2^spread sub-windows the top window
// is spread over when it is sparse.
struct Geometry {
  int c, K, t_top, spread, Keff;
  uint32_t L;
  uint32_t top_range = 0;   // number of values the top window's digit can take (<= L + 1)
  int fold_shift = 0, fold_rows = 0;   // a fold the top window is thin enough for (make_plan takes it if the sort does)
};

// Two-dimensional bucket reduction (reduce2d_kernels.h): c - 1 = a + b bits of the bucket weight
struct Split2d {
  int a, b;            // c - 1 = a + b: high / low bits of the bucket weight
  uint32_t H, D, NC;
};

// How the sort phase sorts a plan's entries: the two-level sort's geometry (geom.sbins = scanned bins per problem),
// tile-local bins per window, k_fine's bins per problem and first bin of the top window's bucket sets, window size of the
// specialized sort kernels (0 = generic); whether the shape fits the two-level sort, and whether it takes it.
struct SortLayout {
  SortGeom geom{};
  uint32_t nbins = 0, fbins = 0, fine_top = 0;
  int cspec = 0;
  bool fits = false, two_level = false;
};

// A tuning knob's value: a release build uses the constant; a development build (-DMSMZ_DEV, tools/build_variant.sh)
// reads the MSMZ_* environment variable when the context is created.
#ifdef MSMZ_DEV
static inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
#else
static inline int env_int(const char*, int dflt) { return dflt; }
#endif

// Planning knobs.  Default-constructed = a release build; a development build fills them from MSMZ_* environment
// variables (engine.h).  None of them changes a result.
struct PlanKnobs {
  bool no_spread = false, no_fold = false, no_window_model = false, force_atomic_sort = false;
  bool no_fbt = false;            // top window's bins as wide as the others
  bool no_plan_top = false;       // top-window bucket sets in full-size plan chunks
  bool no_sort_special = false;   // generic sort kernels for every window size
  int fb_cap = 0;
  uint32_t s1_override = 0, r2_nc = 0;   // first reduction group, chunks per line of the 2-D reduction (0 = automatic)
  int glv_bits_assumed = 0;       // test hook (msmz_test_set_glv_bits): assumed bit length of a GLV half; 0 = GLV_BITS - 1
  uint64_t batch_entries = 0;     // test hook (msmz_test_set_limits): entries per sub-batch; 0 = kMaxBatchEntries
};

template <class Fr>
struct Planner {
  PlanKnobs k;

  // The caller's scalar bit bound (msmz_opts.reserved[1]: every scalar of the call is below 2^bits) as the planner uses
  // it: 0 = none, which is also what a bound of at least the field's bit length says.  (The C ABI refuses values outside
  // [0, 256] before they get here.)
  static int bound(int bits) { return bits <= 0 || bits >= Fr::BITS ? 0 : bits; }

  // bit length the windows are sized for (make_plan's pl.b): the whole scalar (or the caller's bound on it), or a GLV
  // half -- the assumed bound (or the caller's bound on the scalar when that is lower: a half that does not fit is
  // flagged and redone as any other), or with extra_bits the proven one of the retry
  int scalar_bits(bool glv, int extra_bits, int sbits = 0) const {
    const int sb = bound(sbits);
    if (!glv) return sb ? sb : Fr::BITS;
    if (extra_bits) return Fr::GLV_PROVEN_BITS > Fr::GLV_BITS - 1 ? Fr::GLV_PROVEN_BITS : Fr::GLV_BITS - 1;
    const int a = k.glv_bits_assumed > 0 ? k.glv_bits_assumed : Fr::GLV_BITS - 1;
    return sb && sb < a ? sb : a;
  }

  // glv < 0: the engine's choice for n points.  The split halves the windows but doubles the point set (index bits,
  // gathers, tree depth); since the two-dimensional bucket reduction made the reduction cheap per window it is only
  // ahead on the smallest inputs (profiles/r03_sweep.json: 2^14 0.85 vs 0.88 ms, 2^16 1.11 vs 1.07, 2^20 3.87 vs 3.64,
  // 2^23 23.5 vs 20.5).  (Twisted Edwards: its scalar field has no GLV.)
  // A scalar bound of at most the GLV half length: no split, it would only double the point set.
  static bool default_glv(uint64_t n, int sbits = 0) {
    if (bound(sbits) && bound(sbits) <= Fr::GLV_BITS - 1) return false;
    return Fr::HAS_GLV && n < (1ull << 15);
  }

  Geometry geometry(int c, bool glv, uint32_t M, int b, uint32_t F = 1) const {
    Geometry g;
    g.c = c;
    g.K = (b + 1 + c - 1) / c;                              // msm-batched-affine.ts:96
    g.L = 1u << (c - 1);
    const int pos = (g.K - 1) * c;
    g.t_top = b + 1 - pos;
    if (!glv) {
      // the largest scalar: q - 1, or 2^b - 1 < q under a caller-given bound b < Fr::BITS
      uint64_t top = 0;
      for (int j = 0; j < 64 && pos + j < 256; j++) {
        const uint32_t bit = b < Fr::BITS ? (pos + j < b ? 1u : 0u) : (Fr::Q[(pos + j) >> 5] >> ((pos + j) & 31)) & 1u;
        top |= (uint64_t)bit << j;
      }
      if (g.K > 1) top += 1;   // carry from the window below
      g.t_top = ceil_log2_u64(top + 1);
      g.top_range = (uint32_t)(top + 1 > g.L ? g.L : top + 1);
    } else if (Fr::GLV_TYP_BITS + 1 - pos < g.t_top) {
      g.t_top = Fr::GLV_TYP_BITS + 1 - pos;
      if (g.t_top < 1) g.t_top = 1;
    }
    g.spread = 0;
    // (precomputed sets, F > 1: neither fold nor spread -- the top window shares its bucket set with F - 1 windows;
    // choose_window keeps it from being thin)
    if (F == 1 && g.K > 1 && g.t_top <= c - 2) {
      // a thin top window whose digit fits the COLUMN index of the two-dimensional reduction (l < D = 2^b2) can be
      // folded: 2^(c-1-b2) copies of the digit's range fill the set's buckets as evenly as any other window's.  The bound
      // on the digit is the hard one (largest scalar; for GLV halves the bit length the windows were sized for).
      const int b2 = (c - 1) - (c - 1 + 1) / 2;                       // low bits of Split2d
      const int t_bound = glv ? b + 1 - pos : g.t_top;
      if (b2 >= 1 && t_bound <= b2) {
        g.fold_shift = b2;
        g.fold_rows = c - 1 - b2;
      }
      if (!k.no_spread) {   // ... else spread over sub-windows
        g.spread = c - 1 - g.t_top;
        if (g.spread > 3) g.spread = 3;
        const int fbx = fine_bits(c, M);
        while (g.spread > 0 && ((g.L >> fbx) << g.spread) > (uint32_t)COARSE_MAX_BINS) g.spread--;
      }
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
    if (k.fb_cap > 0 && fb > k.fb_cap) fb = k.fb_cap;
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
    if (pl.fold_shift != 0 || k.no_fbt || pl.F > 1) return fb;
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
    if (M >= (1u << 18) || k.no_window_model) {
      // measured optimum of the batched-affine path from 2^18 entries per window on (profiles/r03_sweep.json): 17 without
      // GLV (2^18: 1.60 ms against 1.83 at c = 15), 16 with it (128-bit halves = 8 windows exactly)
      if (tree_rounds && !k.no_window_model) c = glv ? 16 : 17;
      // Under a caller-given scalar bound (b < Fr::BITS) the batched-affine path keeps 17 whatever is left for the top
      // window -- it is spread or folded: at 2^20 with 128-bit scalars c = 17 ran in 2.51 ms, the stepped-down 14 in 2.76
      // (profiles/r06_short_scalars_report.jsonl)
      const bool bounded = tree_rounds && !k.no_window_model && !glv && b < Fr::BITS;
      for (int tries = 0; tries < 3 && c > 4 && !bounded; tries++) {
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
    Plan pl{};
    pl.c = c;
    pl.M = M;
    pl.glv = glv;
    pl.F = F;
    set_geometry(pl, geometry(c, glv, M, b, F));
    // one bucket collects the entries of all W windows of its set (every digit equal in the worst case): the tree rounds
    // take buckets below 2^PLAN_RMAX entries
    return pl.K <= kMaxWindows && (uint64_t)set_windows(pl) * M < (1ull << PLAN_RMAX) && sort_layout(pl).fits;
  }
  int choose_window_pre(bool glv, uint32_t M, int b, uint32_t nprob, uint32_t F) const {
    // measured (profiles/r05_precompute_c_sweep.jsonl): with every window in one set and >= 2^16 entries per window, c = 17
    // is the fastest fitting size (2^16: 0.86 ms against 0.94 at c = 16, 16 x 2^16: 3.26 against 3.43, 2^20: 3.62 against
    // 3.99); with fewer windows per set the model below is (16 x 2^16, F = 2: c = 15 5.98 ms, c = 17 7.76)
    if (!glv && M >= (1u << 16) && F >= (uint32_t)geometry(17, false, M, b, F).K && pre_fits(17, false, M, b, F))
      return 17;
    int best_c = 0;
    double best = 1e30;
    for (int cc = 3; cc <= 20; cc++) {
      if (!pre_fits(cc, glv, M, b, F)) continue;
      const Geometry g = geometry(cc, glv, M, b, F);
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

  static void set_geometry(Plan& pl, const Geometry& g) {
    pl.K = g.K;
    pl.L = g.L;
    pl.spread = g.spread;
    pl.top_range = g.top_range;
    pl.Keff = g.Keff;
  }

  int make_plan(Plan& pl, uint64_t n64, bool glv, const msmz_opts& opt, uint32_t pts_n, bool tree_rounds = true,
                int extra_bits = 0, bool allow_fold = false, uint32_t nprob = 1, uint32_t F = 1) const {
    pl.n = (uint32_t)n64;
    pl.nprob = nprob;
    pl.glv = glv;
    pl.M = glv ? 2 * pl.n : pl.n;
    // scalar bit length.  GLV halves: first attempt assumes |s_j| < 2^127 (every half seen so far; for BLS12-377 the
    // analytic bound is 2^126); k_hist flags a longer half and the MSM is redone (extra_bits = 1) with the proven bound
    // GLV_PROVEN_BITS <= 128, which also is what the 4-word halves of glv_decompose can hold.
    static_assert(!Fr::HAS_GLV || (Fr::GLV_PROVEN_BITS <= 128 && Fr::GLV_PROVEN_BITS <= Fr::GLV_BITS), "GLV halves must fit 4 words");
    pl.sbits = bound(opt.reserved[1]);
    pl.b = scalar_bits(glv, extra_bits, pl.sbits);
    pl.c = opt.c > 0 ? opt.c : choose_window(glv, pl.M, pl.b, tree_rounds, nprob, F);
    if (pl.c < 2) pl.c = 2;
    if (pl.c > 24) pl.c = 24;
    pl.F = F < 1 ? 1 : F;
    const Geometry g = geometry(pl.c, glv, pl.M, pl.b, pl.F);
    set_geometry(pl, g);
    if (allow_fold && !k.no_fold && g.fold_shift != 0) {
      // the folded top window: one bucket set, not spread -- where the two-level sort takes it (the fallback sort numbers
      // buckets by digit alone)
      Plan f = pl;
      f.spread = 0;
      f.Keff = f.K;
      f.fold_shift = g.fold_shift;
      f.fold_rows = g.fold_rows;
      if (sort_layout(f).two_level) pl = f;
    }
    if (pl.F > 1) pl.Keff = (pl.K + (int)set_windows(pl) - 1) / (int)set_windows(pl);   // bucket sets
    const uint64_t nb64 = (uint64_t)pl.Keff * pl.L;
    if (nb64 * nprob + 1 >= (1ull << 31) || (uint64_t)nprob * pl.K * pl.M >= (1ull << 32) || pl.Keff > kMaxWindows)
      return MSMZ_ERR_ARG;
    pl.nb = (uint32_t)nb64;
    pl.nblocks = (pl.nb + SCAN_TILE - 1) / SCAN_TILE;
    pl.endo_delta = glv ? pts_n - pl.n : 0u;
    return MSMZ_OK;
  }

  // The bins of the two-level LDS-staged sort and whether it applies (else the per-entry atomic fallback).  The packed
  // word = fine bucket bits | negate | index: the narrower the index, the more fine bits fit, the fewer (and longer)
  // coarse runs the scatter writes.  Precomputed sets: W windows per bucket set, the packed index = copy << mbits | entry.
  SortLayout sort_layout(const Plan& pl) const {
    SortLayout s;
    const uint32_t W = set_windows(pl);
    const int fb = fine_bits(pl.c, pl.M, W);
    if (fb < 0) return s;
    const int fbt = fine_bits_top(pl, fb);
    const uint32_t ncb = pl.L >> fb, ncbt = pl.L >> fbt;
    const uint32_t top_bin = (uint32_t)(pl.K - 1) * ncb;
    s.nbins = top_bin + (ncbt << pl.spread);
    const int mbits = ceil_log2_u64(pl.M < 2 ? 2 : pl.M);
    const uint32_t sbins = pl.F > 1 ? (uint32_t)pl.Keff * W * ncb : s.nbins;
    s.geom = SortGeom{pl.n, pl.M, pl.c, pl.K, fb, pl.spread, mbits + copy_bits(W), ncb, fbt, ncbt,
                      pl.fold_shift, pl.fold_rows, W, mbits, sbins, pl.sbits ? pl.sbits : 256};
    s.fbins = pl.F > 1 ? (uint32_t)pl.Keff * ncb : s.nbins;
    s.fine_top = pl.F > 1 ? s.fbins - ncb : top_bin;
    // kernels specialized for the window size (unrolled window loop) where one is compiled: 16 / 17, the defaults of
    // large inputs; any other window size takes the generic ones
    s.cspec = (k.no_sort_special || (pl.c != 16 && pl.c != 17) || (pl.glv && pl.c != 16)) ? 0 : pl.c;
    s.fits = pl.M <= (1u << 24) && ncb <= (uint32_t)COARSE_MAX_BINS && (ncbt << pl.spread) <= (uint32_t)COARSE_MAX_BINS &&
             s.nbins <= (uint32_t)SORT_MAX_BINS;
    s.two_level = s.fits && !k.force_atomic_sort;
    return s;
  }

  // buckets per plan workgroup: at most PLAN_CHUNK, fewer when the windows have few (long) buckets, so that the plan
  // still spreads over ~4 workgroups per CU; the top window's bucket sets in half-size chunks when they are denser than
  // the others
  PlanChunks plan_chunks(const Plan& pl) const {
    const uint32_t nb = pl.nb * pl.nprob;   // buckets of all problems
    uint32_t chunk = PLAN_CHUNK;
    while (chunk > 64 && (nb + chunk - 1) / chunk < 1024) chunk >>= 1;
    PlanChunks pc;
    pc.chunk = chunk;
    pc.nb_main = nb;
    pc.chunk_top = chunk;
    if (!k.no_plan_top && pl.nprob == 1 && pl.F == 1 && pl.K > 1 && pl.fold_shift == 0 && chunk >= 128 &&
        (uint64_t)pl.L * 10 > ((uint64_t)pl.top_range << pl.spread) * 13) {
      pc.nb_main = (uint32_t)(pl.K - 1) * pl.L;
      pc.chunk_top = chunk / 2;
    }
    pc.n_main = (pc.nb_main + chunk - 1) / chunk;
    return pc;
  }

  // first level of the 1-D bucket reduction: buckets per group
  uint32_t first_group_size(const Plan& pl) const {
    if (k.s1_override > 0) return k.s1_override < pl.L ? k.s1_override : pl.L;
    uint32_t S1 = 2;
    // L / S1 a power of 4 saves one reduction level; with >= 2^20 buckets groups of 8 still fill the GPU
    // (2 waves per SIMD) and halve the levels above (measured: S1 = 4 -> 1.58 ms, 8 -> 1.45 ms, 16 -> 1.94 ms)
    if (pl.L >= 4 && (ceil_log2_u64(pl.L) & 1) == 0) S1 = 4;
    if ((uint64_t)pl.Keff * pl.L >= (1u << 20) && pl.L >= 8) S1 = 8;
    return S1 < pl.L ? S1 : pl.L;
  }

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
    if (k.r2_nc > 0) {
      nc = 1;
      while (nc < k.r2_nc && nc * 2 <= s.D) nc *= 2;
    }
    s.NC = nc;
    return s;
  }
  // ... as the kernels of the 2-D reduction take it: two problems (rows, columns) per bucket set of the batch
  R2Geom r2_geom(const Plan& pl) const {
    const Split2d sp = split_2d(pl);
    R2Geom g;
    g.L = pl.L;
    g.H = sp.H;
    g.D = sp.D;
    g.NC = sp.NC;
    g.chr = sp.D / sp.NC;
    g.chc = sp.H / sp.NC;
    g.nprob = 2u * pl.nprob * (uint32_t)pl.Keff;
    return g;
  }

  // problems of the next sub-batch over a point set of pts_n points (`factor` copies; <= 1: plain): the window size
  // depends on the batch size, so the plan is made again until the sub-batch fits kMaxBatchEntries (or the lower cap
  // of k.batch_entries); the remaining problems are then dealt into equal sub-batches
  uint32_t batch_size(uint64_t n, const msmz_opts& opt, uint32_t pts_n, uint32_t factor, uint32_t remaining) const {
    uint32_t bs = remaining;
    for (int it = 0; it < 4 && bs > 1; it++) {
      Plan pl;
      if (make_plan(pl, n, opt.glv != 0, opt, pts_n, true, 0, true, bs, factor > 1 ? factor : 1) != MSMZ_OK) {
        bs = (bs + 1) / 2;
        continue;
      }
      const uint32_t fit =
          batch_split(remaining, (uint64_t)pl.K * pl.M, k.batch_entries ? k.batch_entries : kMaxBatchEntries);
      if (fit >= bs) break;
      bs = fit;
    }
    return bs;
  }

  // What a precomputed set over n points is built with: c, GLV choice and copies (factor; 0 = enough copies for every
  // window, the GLV retry's included).  Checks that its bucket sets fit one sort pass and its records the 30-bit field.
  int precompute_params(uint64_t n, const msmz_opts* o, uint32_t factor, int* c_out, int* glv_out, uint32_t* f_out,
                        int* k_out, int* sbits_out = nullptr) const {
    if (n == 0 || factor == 1) return MSMZ_ERR_ARG;
    msmz_opts opt;
    memset(&opt, 0, sizeof(opt));
    if (o) opt = *o; else opt.glv = -1;
    if (opt.buckets == MSMZ_BUCKETS_PROJECTIVE || opt.reserved[0] == 1) return MSMZ_ERR_UNSUPPORTED;
    if (opt.c < 0 || opt.c > 24 || opt.reserved[1] < 0 || opt.reserved[1] > 256) return MSMZ_ERR_ARG;
    const int sb = bound(opt.reserved[1]);
    int glv = opt.glv;
    if (glv < 0) glv = default_glv(n, sb) ? 1 : 0;   // msm()'s choice for n points
    if (glv && !Fr::HAS_GLV) return MSMZ_ERR_UNSUPPORTED;
    glv = glv ? 1 : 0;
    const uint64_t M64 = glv ? 2 * n : n;
    if (M64 > (1ull << 24)) return MSMZ_ERR_ARG;
    const uint32_t M = (uint32_t)M64;
    const int b0 = scalar_bits(glv != 0, 0, sb), b1 = scalar_bits(glv != 0, 1, sb);
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
    if (sbits_out) *sbits_out = sb;
    return MSMZ_OK;
  }
};

}  // namespace msmz

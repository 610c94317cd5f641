// The scalar bit bound (msmz_opts.reserved[1]) in the planner (msm_zprize_amd/csrc/plan.h), on a CPU.  For the four
// scalar fields, the bounds below and window sizes 2..24:
//   - K = ceil((b + 1) / c) with b = min(bound, Fr::BITS) without GLV, min(bound, assumed half length) with it;
//   - bound 0, Fr::BITS, Fr::BITS + 1 and 256 give the same Plan and SortLayout, field by field (plan_test.cpp pins the
//     bound-0 plan to the planner before the bound existed);
//   - top_range = the number of values the top window's digit takes over the scalars up to 2^bound - 1, capped at the L
//     buckets of a set as the field always was; counted by slicing real scalars (every value of the top window's bits
//     x the low parts that decide the carry) with the kernels' signed-digit recoding, for c <= 12.  Without a bound
//     (largest scalar q - 1) the unchanged plan may count one value more: see the check;
//   - a folded plan's fold bound: the largest admissible (half-)scalar's top digit is a valid column, l <= 2^fold_shift;
//   - precompute_params builds the copies of the bounded window count and reports the bound; bad bounds are MSMZ_ERR_ARG;
//   - the engine's GLV choice: none under a bound of at most the GLV half length.
// Prints what the GPU tests rely on (BLS12-377, bound 64: c = 7 folds, c = 17 spreads over 4 sub-windows).
// Exit code = number of failures.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <set>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/plan.h"
using namespace msmz;

static int bad = 0;
static long checks = 0;

#define CHECK(cond, ...)                \
  do {                                  \
    checks++;                           \
    if (!(cond)) {                      \
      if (bad++ < 30) {                 \
        printf("FAIL %s: ", #cond);     \
        printf(__VA_ARGS__);            \
        printf("\n");                   \
      }                                 \
    }                                   \
  } while (0)

// 256-bit little-endian words
struct U256 {
  uint32_t w[8];
};
static uint32_t bits_at(const U256& s, int pos, int c) {
  uint32_t r = 0;
  for (int j = 0; j < c; j++) {
    const int p = pos + j;
    if (p < 256) r |= ((s.w[p >> 5] >> (p & 31)) & 1u) << j;
  }
  return r;
}
static void set_bits(U256& s, int pos, int c, uint32_t v) {
  for (int j = 0; j < c; j++) {
    const int p = pos + j;
    if (p >= 256) continue;
    s.w[p >> 5] &= ~(1u << (p & 31));
    s.w[p >> 5] |= ((v >> j) & 1u) << (p & 31);
  }
}
static bool leq(const U256& a, const U256& b) {
  for (int j = 7; j >= 0; j--)
    if (a.w[j] != b.w[j]) return a.w[j] < b.w[j];
  return true;
}
// the signed digit of window K - 1 (DigitStream::next, sort_kernels.h); *carry_out: the scalar does not fit K windows
static uint32_t top_digit(const U256& s, int c, int K, bool* carry_out) {
  const uint32_t L = 1u << (c - 1);
  uint32_t carry = 0, l = 0;
  for (int k = 0; k < K; k++) {
    l = bits_at(s, k * c, c) + carry;
    carry = 0;
    if (l > L) {
      l = 2 * L - l;
      carry = 1;
    }
  }
  *carry_out = carry != 0;
  return l;
}

template <class Fr>
static U256 largest_scalar(int b) {   // min(q - 1, 2^b - 1)
  U256 s;
  if (b < Fr::BITS) {
    for (int j = 0; j < 8; j++) s.w[j] = 0;
    set_bits(s, 0, b > 32 ? 32 : b, 0xffffffffu);
    for (int p = 32; p < b; p++) s.w[p >> 5] |= 1u << (p & 31);
  } else {
    for (int j = 0; j < 8; j++) s.w[j] = Fr::Q[j];
    for (int j = 0; j < 8; j++)   // - 1
      if (s.w[j]-- != 0) break;
  }
  return s;
}

static bool same_plan(const Plan& a, const Plan& b) {
  return a.n == b.n && a.M == b.M && a.L == b.L && a.nb == b.nb && a.nblocks == b.nblocks && a.c == b.c && a.K == b.K &&
         a.b == b.b && a.Keff == b.Keff && a.spread == b.spread && a.fold_shift == b.fold_shift &&
         a.fold_rows == b.fold_rows && a.top_range == b.top_range && a.glv == b.glv && a.endo_delta == b.endo_delta &&
         a.nprob == b.nprob && a.F == b.F && a.sbits == b.sbits;
}
static bool same_layout(const SortLayout& x, const SortLayout& y) {
  const SortGeom &a = x.geom, &b = y.geom;
  return a.n == b.n && a.M == b.M && a.c == b.c && a.K == b.K && a.fb == b.fb && a.spread == b.spread &&
         a.idx_bits == b.idx_bits && a.ncb == b.ncb && a.fbt == b.fbt && a.ncbt == b.ncbt && a.fold_shift == b.fold_shift &&
         a.fold_rows == b.fold_rows && a.F == b.F && a.mbits == b.mbits && a.sbins == b.sbins && a.sbits == b.sbits &&
         x.nbins == y.nbins && x.fbins == y.fbins && x.fine_top == y.fine_top && x.cspec == y.cspec && x.fits == y.fits &&
         x.two_level == y.two_level;
}

static msmz_opts options(int c, int glv, int bound) {
  msmz_opts o;
  memset(&o, 0, sizeof(o));
  o.c = c;
  o.glv = glv;
  o.reserved[1] = bound;
  return o;
}

template <class Fr>
static void run(const char* name) {
  const Planner<Fr> pr;
  const int bounds[] = {1, 2, 8, 31, 32, 33, 64, 100, 126, 127, 128, 129, 200, Fr::BITS - 1, Fr::BITS, 256};
  const uint64_t sizes[] = {1, 3, 257, 4096, 1u << 16, 1u << 20};
  for (int glv = 0; glv <= (Fr::HAS_GLV ? 1 : 0); glv++) {
    const int full = glv ? Fr::GLV_BITS - 1 : Fr::BITS;
    // ---- bound 0 == bound >= BITS, every field; automatic and fixed window sizes, batches, precomputed sets
    for (uint64_t n : sizes)
      for (int c = 0; c <= 24; c++) {
        if (c == 1) continue;
        for (uint32_t nprob : {1u, 16u})
          for (uint32_t F : {1u, 4u})
            for (int fold = 0; fold <= 1; fold++) {
              Plan p0{};
              const msmz_opts o0 = options(c, glv, 0);
              const int s0 = pr.make_plan(p0, n, glv != 0, o0, (uint32_t)n, true, 0, fold != 0, nprob, F);
              for (int bd : {Fr::BITS, Fr::BITS + 1, 256}) {
                Plan p1{};
                const msmz_opts o1 = options(c, glv, bd);
                const int s1 = pr.make_plan(p1, n, glv != 0, o1, (uint32_t)n, true, 0, fold != 0, nprob, F);
                CHECK(s0 == s1, "%s status n %llu c %d glv %d bound %d", name, (unsigned long long)n, c, glv, bd);
                if (s0 != MSMZ_OK || s1 != MSMZ_OK) continue;
                CHECK(same_plan(p0, p1) && p1.sbits == 0, "%s plan n %llu c %d glv %d bound %d", name, (unsigned long long)n, c, glv, bd);
                // (a precomputed set that fits no sort has no geometry: all zero)
                CHECK(same_layout(pr.sort_layout(p0), pr.sort_layout(p1)) &&
                          pr.sort_layout(p1).geom.sbits == (pr.sort_layout(p1).geom.c ? 256 : 0),
                      "%s layout n %llu c %d glv %d bound %d", name, (unsigned long long)n, c, glv, bd);
              }
            }
      }
    // ---- bounded plans
    for (int bd : bounds) {
      const int b = bd < full ? bd : full;
      CHECK(pr.scalar_bits(glv != 0, 0, bd) == b, "%s scalar_bits glv %d bound %d", name, glv, bd);
      for (int c = 2; c <= 24; c++)
        for (uint64_t n : sizes)
          for (int fold = 0; fold <= 1; fold++) {
            Plan pl{};
            const msmz_opts o = options(c, glv, bd);
            const int st = pr.make_plan(pl, n, glv != 0, o, (uint32_t)n, true, 0, fold != 0);
            Plan pu{};
            const msmz_opts ou = options(c, glv, 0);
            const int su = pr.make_plan(pu, n, glv != 0, ou, (uint32_t)n, true, 0, fold != 0);
            // fewer windows never make a shape unplannable
            CHECK(st == MSMZ_OK || su != MSMZ_OK, "%s make_plan n %llu c %d glv %d bound %d: %d", name, (unsigned long long)n, c, glv, bd, st);
            if (st != MSMZ_OK) continue;
            const int K = (b + 1 + c - 1) / c;
            CHECK(pl.K == K && pl.b == b && pl.c == c, "%s K %d (want %d) b %d c %d glv %d bound %d", name, pl.K, K, pl.b, c, glv, bd);
            CHECK(pl.sbits == (bd < Fr::BITS ? bd : 0), "%s sbits %d bound %d", name, pl.sbits, bd);
            CHECK(pl.Keff >= 1 && pl.Keff <= kMaxWindows && (pl.K > 1 || (pl.spread == 0 && pl.fold_shift == 0 && pl.Keff == 1)),
                  "%s Keff %d K %d spread %d c %d bound %d", name, pl.Keff, pl.K, pl.spread, c, bd);
            const SortLayout sl = pr.sort_layout(pl);
            CHECK(sl.geom.sbits == (pl.sbits ? pl.sbits : 256) && sl.geom.K == K, "%s geom sbits c %d bound %d", name, c, bd);
            if (pl.fold_shift != 0) CHECK(sl.two_level, "%s folded plan not two-level c %d bound %d", name, c, bd);
            const int pos = (K - 1) * c;
            // the largest admissible (half-)scalar: min(q - 1, 2^b - 1), or a half of b bits
            const U256 smax = glv ? largest_scalar<Fr>(b < Fr::BITS ? b : Fr::BITS - 1) : largest_scalar<Fr>(b);
            bool cy = false;
            uint32_t lmax = top_digit(smax, c, K, &cy);
            CHECK(!cy, "%s the largest scalar does not fit K windows c %d bound %d", name, c, bd);
            if (!glv && c <= 12) {
              // every value of the top window's raw bits x low parts {0, all ones, the largest scalar's}
              std::set<uint32_t> seen;
              const uint32_t rmax = bits_at(smax, pos, c);
              for (uint32_t r = 0; r <= rmax; r++)
                for (int lo = 0; lo < 3; lo++) {
                  U256 s = smax;
                  if (lo < 2)
                    for (int p = 0; p < pos; p += 16) set_bits(s, p, pos - p < 16 ? pos - p : 16, lo ? 0xffffu : 0u);
                  set_bits(s, pos, c, r);
                  if (!leq(s, smax)) continue;
                  bool c2 = false;
                  const uint32_t l = top_digit(s, c, K, &c2);
                  CHECK(!c2, "%s a scalar below the bound does not fit K windows c %d bound %d", name, c, bd);
                  seen.insert(l);
                  if (l > lmax) lmax = l;
                }
              const uint32_t want = seen.size() > pl.L ? pl.L : (uint32_t)seen.size();
              if (pl.sbits != 0) {
                CHECK(pl.top_range == want, "%s top_range %u, %u values seen: c %d K %d bound %d", name, pl.top_range, want, c, K, bd);
              } else {
                // No bound: the plan is the one from before the bound existed (checked above), and that one counts the
                // carry into q - 1's top bits whether or not a scalar below q reaches it (BLS12-377, c = 3: the top
                // bits are 1 and no scalar <= q - 1 with that bit set carries).  One value too many at most, never too few.
                const uint32_t up = want + 1 > pl.L ? pl.L : want + 1;
                CHECK(pl.top_range == want || pl.top_range == up, "%s top_range %u, %u values seen: c %d K %d no bound", name,
                      pl.top_range, want, c, K);
              }
            }
            CHECK(lmax <= pl.L, "%s top digit %u > L c %d bound %d", name, lmax, c, bd);
            if (pl.fold_shift != 0)
              CHECK(lmax <= (1u << pl.fold_shift) && pl.fold_shift + pl.fold_rows == c - 1,
                    "%s fold bound: top digit %u, fold_shift %d c %d glv %d bound %d", name, lmax, pl.fold_shift, c, glv, bd);
          }
      // ---- precomputed sets: the copies of the bounded window count
      for (int c : {0, 7, 13, 16, 17})
        for (uint32_t factor : {0u, 2u, 3u, 1000u}) {
          const msmz_opts o = options(c, glv, bd);
          int c1 = 0, g1 = -1, k1 = 0, sb = -1;
          uint32_t f1 = 0;
          const uint64_t n = 1u << 16;
          const int st = pr.precompute_params(n, &o, factor, &c1, &g1, &f1, &k1, &sb);
          if (st != MSMZ_OK) {
            // refused: a single window (nothing to share) or a set that does not fit one sort pass -- never a crash
            CHECK(st == MSMZ_ERR_ARG, "%s precompute status %d c %d bound %d", name, st, c, bd);
            continue;
          }
          const int K0 = (b + 1 + c1 - 1) / c1;
          const int b1 = pr.scalar_bits(glv != 0, 1, bd);
          const int K1 = (b1 + 1 + c1 - 1) / c1;
          const int Kmax = K0 > K1 ? K0 : K1;
          CHECK(g1 == glv && k1 == K0 && sb == (bd < Fr::BITS ? bd : 0), "%s precompute K %d (want %d) sbits %d c %d glv %d bound %d",
                name, k1, K0, sb, c1, glv, bd);
          CHECK(f1 == (factor == 0 || factor > (uint32_t)Kmax ? (uint32_t)Kmax : factor), "%s copies %u factor %u Kmax %d c %d bound %d",
                name, f1, factor, Kmax, c1, bd);
        }
    }
  }
  // ---- bad bounds; the engine's GLV choice
  for (int bd : {-1, -256, 257, 1 << 20}) {
    const msmz_opts o = options(0, 0, bd);
    int c1, g1, k1;
    uint32_t f1;
    CHECK(pr.precompute_params(1u << 16, &o, 0, &c1, &g1, &f1, &k1) == MSMZ_ERR_ARG, "%s bad bound %d accepted", name, bd);
  }
  for (uint64_t n : {1ull, 1ull << 10, 1ull << 14, 1ull << 15, 1ull << 20}) {
    CHECK(pr.default_glv(n, 0) == pr.default_glv(n) && pr.default_glv(n, Fr::BITS) == pr.default_glv(n) &&
              pr.default_glv(n, 256) == pr.default_glv(n), "%s default_glv without a bound n %llu", name, (unsigned long long)n);
    if (Fr::HAS_GLV) {
      for (int bd : {1, 64, Fr::GLV_BITS - 1}) CHECK(!pr.default_glv(n, bd), "%s default_glv n %llu bound %d", name, (unsigned long long)n, bd);
      for (int bd : {Fr::GLV_BITS, 200})
        CHECK(pr.default_glv(n, bd) == pr.default_glv(n), "%s default_glv n %llu bound %d", name, (unsigned long long)n, bd);
    }
  }
}

int main() {
  run<Bls377Fr>("bls12-377");
  run<PallasFr>("pallas");
  run<Bls381Fr>("bls12-381");
  run<Ed377Fr>("ed-on-bls12-377");
  // the shapes the GPU tests name (tests/test_scalar_bits_gpu.py)
  const Planner<Bls377Fr> pr;
  for (int c : {7, 17}) {
    Plan pl{};
    const msmz_opts o = options(c, 0, 64);
    const int st = pr.make_plan(pl, 4096, false, o, 4096, true, 0, true);
    printf("bls12-377 bound 64 c %d: status %d K %d fold_shift %d spread %d top_range %u two_level %d\n", c, st, pl.K,
           pl.fold_shift, pl.spread, pl.top_range, (int)pr.sort_layout(pl).two_level);
    CHECK(st == MSMZ_OK && (c == 7 ? pl.fold_shift != 0 && pl.spread == 0 : pl.fold_shift == 0 && pl.spread == 2),
          "bls12-377 bound 64 c %d: fold_shift %d spread %d", c, pl.fold_shift, pl.spread);
  }
  printf("checks %ld failures %d\n", checks, bad);
  return bad > 255 ? 255 : bad;
}

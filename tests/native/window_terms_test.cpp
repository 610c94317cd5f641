// The host Horner's window terms (csrc/host64.h window_terms + host_horner) against the per-path Horner loops they
// replaced, for every plan shape: window sizes 2..24, spread and folded top windows, precomputed sets of F windows,
// the 2-D reduction's two results per bucket set and reduceAffine's one.  A recording group turns each Horner into its
// sequence of doublings and additions; the sequences must be equal, except that the old folded-top loop doubled the
// point at infinity split_b times before its first addition (a no-op the new Horner skips).  Exit code = number of
// mismatching shapes.
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fp.h"
#include "../../msm_zprize_amd/csrc/curve.h"
#include "../../msm_zprize_amd/csrc/host64.h"
using namespace msmz;

constexpr int DBL = -1;   // an op: DBL, or the index of the result added
static const uint32_t kRes[1024] = {};

struct Recorder {
  struct Pt {};
  std::vector<int>* ops;
  void set_inf(Pt&) const {}
  void dbl(Pt&, const Pt&) const { ops->push_back(DBL); }
  void load_pt(Pt&, const uint32_t* w) const { ops->push_back((int)(w - kRes)); }
  void add_pt(Pt&, const Pt&, const Pt&) const {}
};

// the loops as they were: 1-D (split_b < 0), 2-D with a plain / spread / folded top window, precomputed sets (F > 1)
static std::vector<int> old_loops(int c, int K, int Keff, int F, int split_b, bool fold) {
  std::vector<int> ops;
  auto dbl_n = [&](int n) { ops.insert(ops.end(), n, DBL); };
  if (split_b < 0) {
    for (int k = Keff - 1; k >= 0; k--) {
      if (k < K - 1) dbl_n(c);
      ops.push_back(k);
    }
  } else if (F > 1) {
    for (int s = Keff - 1; s >= 0; s--) {
      if (s < Keff - 1) dbl_n(c * F - split_b);
      ops.push_back(2 * s);
      dbl_n(split_b);
      ops.push_back(2 * s + 1);
    }
  } else {
    for (int k = K - 1; k >= 0; k--) {
      const int hi = k == K - 1 ? Keff - 1 : k;
      if (k < K - 1) dbl_n(c - split_b);
      if (!(fold && k == K - 1))
        for (int kw = k; kw <= hi; kw++) ops.push_back(2 * kw);
      dbl_n(split_b);
      for (int kw = k; kw <= hi; kw++) ops.push_back(2 * kw + 1);
    }
  }
  size_t lead = 0;   // doublings of the point at infinity
  while (lead < ops.size() && ops[lead] == DBL) lead++;
  return std::vector<int>(ops.begin() + lead, ops.end());
}

int main() {
  int bad = 0, shapes = 0;
  auto check = [&](int c, int K, int Keff, int F, int split_b, bool fold) {
    std::vector<int> ops;
    host_horner(Recorder{&ops}, window_terms(c, K, Keff, F, split_b, fold), kRes, 1);
    shapes++;
    if (ops != old_loops(c, K, Keff, F, split_b, fold)) {
      if (bad++ < 10) printf("mismatch: c %d K %d Keff %d F %d split_b %d fold %d\n", c, K, Keff, F, split_b, fold);
    }
  };
  for (int c = 2; c <= 24; c++) {
    const int b2 = (c - 1) - (c - 1 + 1) / 2;   // engine.h split_2d: low bits of the bucket weight
    for (int K = 1; K <= 128; K++) {
      for (int spread = 0; spread <= (K > 1 ? 3 : 0); spread++) {
        const int Keff = K - 1 + (1 << spread);
        if (Keff > 128) continue;
        check(c, K, Keff, 1, -1, false);
        check(c, K, Keff, 1, b2, false);
        if (spread == 0 && K > 1 && b2 >= 1) check(c, K, Keff, 1, b2, true);
      }
      for (int F : {2, 3, 5, K, K + 1}) {
        if (F < 2) continue;
        const int W = F < K ? F : K;
        check(c, K, (K + W - 1) / W, F, b2, false);
      }
    }
  }
  printf("shapes %d mismatches %d\n", shapes, bad);
  return bad;
}

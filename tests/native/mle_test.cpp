// Host-side driver for the host-callable part of msm_zprize_amd/csrc/mle_kernels.h: the run of eq values one thread of
// k_scalars_eq_table / k_scalars_mle_eval owns, the bind of one pair, and the round body of one pair index of
// k_scalars_sumcheck_round with the coefficient preparation of the host, compiled for the CPU from the same templates.
// Driven by tests/test_mle_cpu.py through stdin/stdout, one request per line, values as hex:
//   <curve> eq <n_vars> <g> <scale> <r_0> .. <r_(n_vars-1)>  ->  min(MLE_RUN, 2^n_vars) values scale eq(r, g + k)
//   <curve> bind <lo> <hi> <r>                                 ->  lo + r (hi - lo)
//   <curve> round <nt> <pairs> <n_terms>  then per pair and table <lo> <hi>,  then per term <mask> <coeff or ->
//                                                              ->  degree + 1 values g(0) .. g(degree) over those pairs
//   geometry                                                   ->  MLE_RUN MLE_TILE MSC_TILE MSC_MAX_TABLES MSC_MAX_DEGREE MSC_MAX_TERMS
// No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fr.h"
#include "../../msm_zprize_amd/csrc/mle_kernels.h"
using namespace msmz;

static void parse(const std::string& h, uint32_t* w) {
  std::string s(64 - h.size(), '0'); s += h;
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)strtoul(s.substr((7 - i) * 8, 8).c_str(), nullptr, 16);
}
static void print(const uint32_t* w, const char* end) {
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
  printf("%s", end);
}
static void read(uint32_t* w) {
  std::string s;
  std::cin >> s;
  parse(s, w);
}

template <class Fr> static void run(const std::string& op) {
  if (op == "eq") {
    unsigned n_vars;
    unsigned long long g;
    std::cin >> n_vars >> g;
    uint32_t scale[8];
    read(scale);
    FrEqPoint pt = {};
    for (unsigned j = 0; j < n_vars && j < (unsigned)MLE_MAX_VARS; j++) {
      uint32_t r[8];
      read(r);
      fr_to_mont<Fr>(pt.r[j], r);
    }
    uint32_t e[MLE_RUN][8];
    fr_eq_run<Fr>(e, scale, pt, n_vars, (uint32_t)g);
    const unsigned count = n_vars < 3 ? 1u << n_vars : (unsigned)MLE_RUN;
    for (unsigned k = 0; k < count; k++) print(e[k], k + 1 == count ? "\n" : " ");
  } else if (op == "bind") {
    uint32_t lo[8], hi[8], r[8], out[8];
    read(lo); read(hi); read(r);
    fr_to_mont<Fr>(r, r);
    fr_bind<Fr>(out, lo, hi, r);
    print(out, "\n");
  } else if (op == "round") {
    unsigned nt, pairs, n_terms;
    std::cin >> nt >> pairs >> n_terms;
    // the line carries the pairs before the terms; the terms are needed first, so the pairs are buffered as text
    std::vector<std::string> words((size_t)pairs * nt * 2);
    for (auto& w : words) std::cin >> w;
    FrScTerms T = {};
    T.n_terms = n_terms;
    for (unsigned k = 0; k < n_terms && k < (unsigned)MSC_MAX_TERMS; k++) {
      std::string cs;
      std::cin >> std::hex >> T.mask[k] >> std::dec >> cs;
      uint32_t c[8] = {1, 0, 0, 0, 0, 0, 0, 0};
      if (cs != "-") parse(cs, c);
      const int f = __builtin_popcount(T.mask[k]);
      if ((uint32_t)f > T.degree) T.degree = f;
      fr_sc_coeff<Fr>(T.coeff[k], c, f);
    }
    uint32_t acc[MSC_MAX_DEGREE + 1][8] = {};
    auto body = [&](auto NTc) {
      constexpr int NT = decltype(NTc)::value;
      for (unsigned p = 0; p < pairs; p++) {
        uint32_t cur[NT][8], hi[NT][8];
        for (int j = 0; j < NT; j++) {
          parse(words[((size_t)p * NT + j) * 2], cur[j]);
          parse(words[((size_t)p * NT + j) * 2 + 1], hi[j]);
        }
        fr_sc_pair<Fr, NT>(acc, cur, hi, T);
      }
    };
    switch (nt) {
      case 1: body(std::integral_constant<int, 1>{}); break;
      case 2: body(std::integral_constant<int, 2>{}); break;
      case 3: body(std::integral_constant<int, 3>{}); break;
      case 4: body(std::integral_constant<int, 4>{}); break;
      case 5: body(std::integral_constant<int, 5>{}); break;
      case 6: body(std::integral_constant<int, 6>{}); break;
      default: printf("?\n"); return;
    }
    static_assert(MSC_MAX_TABLES == 6, "one case per table count");
    for (uint32_t t = 0; t <= T.degree; t++) print(acc[t], t == T.degree ? "\n" : " ");
  } else {
    printf("?\n");
  }
}

int main() {
  std::string curve, op;
  while (std::cin >> curve) {
    if (curve == "geometry") {
      printf("%d %d %d %d %d %d\n", MLE_RUN, MLE_TILE, MSC_TILE, MSC_MAX_TABLES, MSC_MAX_DEGREE, MSC_MAX_TERMS);
      continue;
    }
    std::cin >> op;
    if (curve == "bls12-377") run<Bls377Fr>(op);
    else if (curve == "pallas") run<PallasFr>(op);
    else if (curve == "bls12-381") run<Bls381Fr>(op);
    else if (curve == "ed-on-bls12-377") run<Ed377Fr>(op);
    else printf("?\n");
  }
  return 0;
}

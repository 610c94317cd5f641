// Host-side driver for the step bodies of msm_zprize_amd/csrc/mle_kernels.h: fr_sc_step, what one thread of
// k_scalars_sumcheck_step does for one new pair index (two fr_bind per table, then fr_sc_pair), and fr_sc_last, the one
// thread of k_scalars_sumcheck_last, compiled for the CPU from the same templates with the coefficient preparation of
// the host.  Driven by tests/test_sumcheck_step_cpu.py through stdin/stdout, one request per line, values as hex:
//   <curve> step <nt> <pairs> <n_terms> <r>  then per new pair index and table the four source records <lo0> <hi0> <lo1>
//       <hi1> (lo0, hi0 bind into the new lo; lo1, hi1 into the new hi),  then per term <mask> <coeff or ->
//       ->  degree + 1 values g(0) .. g(degree) over those indices, then per index and table the two entries stored
//   <curve> last <nt> <n_terms> <r>  then per table <lo> <hi>,  then per term <mask> <coeff or ->
//       ->  the value by fr_sc_step (both pairs the same, degree 0), the value by fr_sc_last, then per table the entry
//           fr_sc_last stored
//   geometry  ->  MSC_TILE MSC_MAX_TABLES MSC_MAX_DEGREE MSC_MAX_TERMS MSC_STEP_FUSED_TABLES
// A stand-alone program: the same file built with -fsanitize=address,undefined runs the same requests.  No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fr.h"
#include "../../msm_zprize_amd/csrc/mle_kernels.h"
using namespace msmz;

struct Rec {
  uint32_t w[8];
};

static Rec parse(const std::string& h) {
  Rec r;
  std::string s(64 - h.size(), '0');
  s += h;
  for (int i = 0; i < 8; i++) r.w[i] = (uint32_t)strtoul(s.substr((7 - i) * 8, 8).c_str(), nullptr, 16);
  return r;
}
static Rec read() {
  std::string s;
  std::cin >> s;
  return parse(s);
}
static void print(const uint32_t* w) {
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
}

template <class Fr> static bool read_terms(FrScTerms* T, unsigned n_terms) {
  if (n_terms < 1 || n_terms > (unsigned)MSC_MAX_TERMS) return false;
  T->n_terms = n_terms;
  for (unsigned k = 0; k < n_terms; k++) {
    std::string cs;
    std::cin >> std::hex >> T->mask[k] >> std::dec >> cs;
    Rec c = parse("1");
    if (cs != "-") c = parse(cs);
    const int f = __builtin_popcount(T->mask[k]);
    if ((uint32_t)f > T->degree) T->degree = f;
    fr_sc_coeff<Fr>(T->coeff[k], c.w, f);
  }
  return true;
}

template <class Fr, int NT>
static void step(const std::vector<Rec>& src, std::vector<Rec>& dst, unsigned pairs, const FrScTerms& T, const uint32_t* r_mont) {
  uint32_t acc[MSC_MAX_DEGREE + 1][8] = {};
  for (unsigned p = 0; p < pairs; p++) {
    fr_sc_step<Fr, NT>(
        acc, T, r_mont,
        [&](auto J, auto K, uint32_t* out) {
          const Rec& s = src[((size_t)p * NT + J) * 4 + K];
          for (int w = 0; w < 8; w++) out[w] = s.w[w];
          return false;
        },
        [&](auto J, auto K, const uint32_t* in) {
          Rec& d = dst[((size_t)p * NT + J) * 2 + K];
          for (int w = 0; w < 8; w++) d.w[w] = in[w];
        });
  }
  for (uint32_t t = 0; t <= T.degree; t++) print(acc[t]), printf(" ");
}

template <class Fr> static void run(const std::string& op) {
  const bool last = op == "last";
  if (!last && op != "step") {
    printf("?\n");
    return;
  }
  unsigned nt, pairs = 1, n_terms;
  std::cin >> nt;
  if (!last) std::cin >> pairs;
  std::cin >> n_terms;
  if (nt < 1 || nt > (unsigned)MSC_MAX_TABLES || pairs < 1 || pairs > 64) {
    printf("?\n");
    return;
  }
  Rec r = read();
  fr_to_mont<Fr>(r.w, r.w);
  std::vector<Rec> src((size_t)pairs * nt * 4), dst((size_t)pairs * nt * 2);
  for (size_t i = 0; i < (size_t)pairs * nt; i++) {
    src[4 * i] = read(), src[4 * i + 1] = read();
    if (last) src[4 * i + 2] = src[4 * i], src[4 * i + 3] = src[4 * i + 1];   // (both pairs the same: hi = lo)
    else src[4 * i + 2] = read(), src[4 * i + 3] = read();
  }
  FrScTerms T = {};
  if (!read_terms<Fr>(&T, n_terms)) {
    printf("?\n");
    return;
  }
  if (last) T.degree = 0;
  switch (nt) {
    case 1: step<Fr, 1>(src, dst, pairs, T, r.w); break;
    case 2: step<Fr, 2>(src, dst, pairs, T, r.w); break;
    case 3: step<Fr, 3>(src, dst, pairs, T, r.w); break;
    case 4: step<Fr, 4>(src, dst, pairs, T, r.w); break;
    case 5: step<Fr, 5>(src, dst, pairs, T, r.w); break;
    case 6: step<Fr, 6>(src, dst, pairs, T, r.w); break;
  }
  static_assert(MSC_MAX_TABLES == 6, "one case per table count");
  if (!last) {
    for (size_t i = 0; i < dst.size(); i++) print(dst[i].w), printf(i + 1 == dst.size() ? "\n" : " ");
    return;
  }
  uint32_t acc[8] = {};
  std::vector<Rec> bound(nt);
  fr_sc_last<Fr>(
      acc, T, nt, r.w,
      [&](uint32_t j, int k, uint32_t* out) {
        for (int w = 0; w < 8; w++) out[w] = src[4 * (size_t)j + k].w[w];
        return false;
      },
      [&](uint32_t j, const uint32_t* in) {
        for (int w = 0; w < 8; w++) bound[j].w[w] = in[w];
      },
      [&](uint32_t j, uint32_t* out) {
        for (int w = 0; w < 8; w++) out[w] = bound[j].w[w];
      });
  print(acc);
  for (unsigned j = 0; j < nt; j++) printf(" "), print(bound[j].w);
  printf("\n");
}

int main() {
  std::string curve, op;
  while (std::cin >> curve) {
    if (curve == "geometry") {
      printf("%d %d %d %d %d\n", MSC_TILE, MSC_MAX_TABLES, MSC_MAX_DEGREE, MSC_MAX_TERMS, MSC_STEP_FUSED_TABLES);
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

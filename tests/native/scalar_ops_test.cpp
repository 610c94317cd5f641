// Host-side driver for msm_zprize_amd/csrc/fr.h and the host-callable part of scalar_kernels.h: the F_q functions the
// scalar-set kernels (k_scalars_combine / _dot / _powers) are built from, compiled for the CPU from the same templates.
// Driven by tests/test_scalar_ops_cpu.py through stdin/stdout, one request per line, values as hex:
//   <curve> ops <a> <b>                    ->  <a + b> <a - b> <a b 2^-256> <a b>           (all mod q)
//   <curve> const                          ->  <R2> <ONE>
//   <curve> pow <base> <ratio> <g> <count> ->  count values base ratio^(g + j): the table of ratio^(2^k) and the body of
//                                              one thread of k_scalars_powers (fr_pow_run), count <= SPOW_RUN
//   geometry                               ->  SDOT_TILE SDOT_PASS SPOW_RUN
// No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fr.h"
#include "../../msm_zprize_amd/csrc/scalar_kernels.h"
using namespace msmz;

static void parse(const std::string& h, uint32_t* w) {
  std::string s(64 - h.size(), '0'); s += h;
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)strtoul(s.substr((7 - i) * 8, 8).c_str(), nullptr, 16);
}
static void print(const uint32_t* w, const char* end) {
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
  printf("%s", end);
}

template <class Fr> static void run(const std::string& op) {
  if (op == "ops") {
    std::string as, bs;
    std::cin >> as >> bs;
    uint32_t a[8], b[8], r[8];
    parse(as, a); parse(bs, b);
    fr_add<Fr>(r, a, b); print(r, " ");
    fr_sub<Fr>(r, a, b); print(r, " ");
    fr_mont_mul<Fr>(r, a, b); print(r, " ");
    fr_mul<Fr>(r, a, b); print(r, "\n");
  } else if (op == "const") {
    print(Fr::R2, " "); print(Fr::ONE, "\n");
  } else if (op == "pow") {
    std::string bs, rs;
    unsigned long long g;
    unsigned count;
    std::cin >> bs >> rs >> g >> count;
    uint32_t base[8], ratio[8];
    parse(bs, base); parse(rs, ratio);
    FrPowTable t;
    fr_pow_table<Fr>(t, ratio);
    alignas(16) uint32_t out[SPOW_RUN * 8];
    if (count > (unsigned)SPOW_RUN) count = SPOW_RUN;
    fr_pow_run<Fr>(out, base, t, (uint32_t)g, count);
    for (unsigned j = 0; j < count; j++) print(out + j * 8, j + 1 == count ? "\n" : " ");
  } else {
    printf("?\n");
  }
}

int main() {
  std::string curve, op;
  while (std::cin >> curve) {
    if (curve == "geometry") { printf("%d %d %d\n", SDOT_TILE, SDOT_PASS, SPOW_RUN); continue; }
    std::cin >> op;
    if (curve == "bls12-377") run<Bls377Fr>(op);
    else if (curve == "pallas") run<PallasFr>(op);
    else if (curve == "bls12-381") run<Bls381Fr>(op);
    else if (curve == "ed-on-bls12-377") run<Ed377Fr>(op);
    else printf("?\n");
  }
  return 0;
}

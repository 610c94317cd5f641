// Host-side driver for msm_zprize_amd/csrc/sqrt.h and the `decompress` of both curve groups (curve.h): the templates
// the compressed-import kernel instantiates, compiled for the CPU.  Driven by tests/test_compressed_cpu.py through
// stdin/stdout, one request per line, values canonical hex:
//   sqrt <curve> <a>                       -> <1 / 0> <root>          (fe_sqrt over the curve's base field)
//   dec  <curve> <wire> <sign> <parity>    -> <status> <x> <y>        (WeierGroup / TeGroup ::decompress)
//   sign <curve> <value> <parity>          -> <sign> <is zero>        (fe_wire_sign: what compression writes)
//   info                                   -> S, C, N, DELTA, products of the four fields
// No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fp.h"
#include "../../msm_zprize_amd/csrc/curve.h"
using namespace msmz;

template <class F> static void to_mont(Fe<F>& r, const std::string& h) {
  constexpr int NW = F::NW;
  uint32_t w[NW];
  std::string s(NW * 8 - h.size(), '0'); s += h;
  for (int i = 0; i < NW; i++) w[i] = (uint32_t)strtoul(s.substr((NW - 1 - i) * 8, 8).c_str(), nullptr, 16);
  Fe<F> c;
  fe_unpack<F>(c, w);
  fe_to_mont(r, c);
}

template <class F> static std::string canon(const Fe<F>& m) {
  Fe<F> t;
  uint32_t w[F::NW];
  fe_from_mont(t, m);
  fe_to_canon_words<F>(w, t);
  std::string out;
  char buf[9];
  for (int i = F::NW - 1; i >= 0; i--) { snprintf(buf, sizeof buf, "%08x", w[i]); out += buf; }
  return out;
}

template <class G> static void request(const std::string& op) {
  using F = typename G::F;
  std::string a;
  int sign, parity;
  if (op == "sqrt") {
    std::cin >> a;
    Fe<F> m, r;
    to_mont<F>(m, a);
    const bool ok = fe_sqrt<F>(r, m);
    printf("%d %s\n", ok ? 1 : 0, ok ? canon<F>(r).c_str() : "0");
  } else if (op == "dec") {
    std::cin >> a >> sign >> parity;
    Fe<F> m, x, y;
    to_mont<F>(m, a);
    const int st = G::decompress(x, y, m, sign != 0, parity);
    if (st) printf("%d 0 0\n", st);
    else printf("0 %s %s\n", canon<F>(x).c_str(), canon<F>(y).c_str());
  } else {
    std::cin >> a >> parity;
    Fe<F> m;
    bool zero;
    to_mont<F>(m, a);
    const bool s = fe_wire_sign<F>(&zero, m, parity);
    printf("%d %d\n", s ? 1 : 0, zero ? 1 : 0);
  }
}

template <class F> static void info() {
  printf("%d %d %d %d %d\n", F::SQRT_S, F::SQRT_C, F::SQRT_N, F::SQRT_DELTA, F::SQRT_PRODUCTS);
}

int main() {
  std::string op, curve;
  while (std::cin >> op) {
    if (op == "info") {
      info<Bls377Fp>(); info<PallasFp>(); info<Bls381Fp>(); info<Ed377Fp>();
      continue;
    }
    std::cin >> curve;
    if (curve == "bls12-377") request<WeierGroup<Bls377Fp>>(op);
    else if (curve == "pallas") request<WeierGroup<PallasFp>>(op);
    else if (curve == "bls12-381") request<WeierGroup<Bls381Fp>>(op);
    else if (curve == "ed-on-bls12-377") request<TeGroup<Ed377Fp>>(op);
    else return 2;
  }
  return 0;
}

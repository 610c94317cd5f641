// Host-side driver for msm_zprize_amd/csrc/check_kernels.h: the curve equations and the chain [q]P the validation
// kernels run (k_check_curve / k_check_subgroup) over the groups of curve.h, compiled for the CPU from the same
// templates.  Driven by tests/test_check_points_cpu.py through stdin/stdout: one point per line
//   <curve> <x hex> <y hex> <flagged as infinity: 0 / 1>
// in canonical form; it is brought to the resident record's form (lazy Montgomery words, Niels form on the twisted
// Edwards curve) the way the upload kernels do, and the verdict byte of msmz_check_points is printed.  No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fp.h"
#include "../../msm_zprize_amd/csrc/check_kernels.h"
using namespace msmz;

template <int NW> static void parse(const std::string& h, uint32_t* w) {
  std::string s(NW * 8 - h.size(), '0'); s += h;
  for (int i = 0; i < NW; i++) w[i] = (uint32_t)strtoul(s.substr((NW - 1 - i) * 8, 8).c_str(), nullptr, 16);
}

// canonical words -> the value a kernel unpacks from a resident record: Montgomery form, stored to [0, 3p), reloaded
template <class F> static void resident(Fe<F>& r, const Fe<F>& mont) {
  uint32_t w[F::NW];
  fe_store<F>(w, mont);
  fe_unpack<F>(r, w);
}
template <class F> static void to_mont(Fe<F>& r, const std::string& h) {
  uint32_t w[F::NW];
  Fe<F> c;
  parse<F::NW>(h, w);
  fe_unpack<F>(c, w);
  fe_to_mont(r, c);
}

template <class F, class Fr> static int weier(const std::string& xs, const std::string& ys, int inf) {
  using G = WeierGroup<F>;
  if (inf) return 0;   // the all-zero record
  Fe<F> mx, my, x, y;
  to_mont<F>(mx, xs); to_mont<F>(my, ys);
  uint32_t w[2 * F::NW];
  fe_store<F>(w, mx); fe_store<F>(w + F::NW, my);
  if (words_point_is_inf<F>(w)) return 0;   // load_affine: the all-zero record is the point at infinity
  fe_unpack<F>(x, w); fe_unpack<F>(y, w + F::NW);
  if (!G::on_curve(x, y)) return CHECK_OFF_CURVE;
  if (Fr::PRIME_ORDER) return 0;
  typename G::Base b;
  G::base_from_affine(b, x, y, false);
  return group_times_order_is_zero<G, Fr>(b) ? 0 : CHECK_OFF_SUBGROUP;
}

template <class F, class Fr> static int te(const std::string& xs, const std::string& ys) {
  using G = TeGroup<F>;
  Fe<F> mx, my, x, y;
  to_mont<F>(mx, xs); to_mont<F>(my, ys);
  typename G::Base n, b;
  G::base_from_affine(n, mx, my, false);                        // TePolicy::store_resident (kernels.h)
  resident<F>(b.ym, n.ym); resident<F>(b.yp, n.yp); resident<F>(b.kt, n.kt); resident<F>(x, mx);
  fe_add(y, b.ym, x);                                           // TePolicy::load_resident_affine
  if (!G::on_curve(x, y)) return CHECK_OFF_CURVE;
  return group_times_order_is_zero<G, Fr>(b) ? 0 : CHECK_OFF_SUBGROUP;
}

int main() {
  std::string curve, x, y; int inf;
  while (std::cin >> curve >> x >> y >> inf) {
    int v = -1;
    if (curve == "bls12-377") v = weier<Bls377Fp, Bls377Fr>(x, y, inf);
    else if (curve == "pallas") v = weier<PallasFp, PallasFr>(x, y, inf);
    else if (curve == "bls12-381") v = weier<Bls381Fp, Bls381Fr>(x, y, inf);
    else if (curve == "ed-on-bls12-377") v = te<Ed377Fp, Ed377Fr>(x, y);
    printf("%d\n", v);
  }
  printf("weights %d %d %d %d\n", order_weight<Bls377Fr>(), order_weight<PallasFr>(), order_weight<Bls381Fr>(), order_weight<Ed377Fr>());
  return 0;
}

// Host-side driver for msm_zprize_amd/csrc/check_kernels.h: the curve equations and the chain [q]P the validation
// kernels run (k_check_curve / k_check_subgroup and their twisted-Edwards twins), compiled for the CPU from the same
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
  if (inf) return 0;   // the all-zero record
  Affine<F> m, a;
  to_mont<F>(m.x, xs); to_mont<F>(m.y, ys);
  uint32_t w[2 * F::NW];
  fe_store<F>(w, m.x); fe_store<F>(w + F::NW, m.y);
  if (words_point_is_inf<F>(w)) return 0;   // load_affine: the all-zero record is the point at infinity
  fe_unpack<F>(a.x, w); fe_unpack<F>(a.y, w + F::NW);
  if (!weier_on_curve<F>(a)) return CHECK_OFF_CURVE;
  if (Fr::PRIME_ORDER) return 0;
  return point_times_order_is_zero<F, Fr>(a) ? 0 : CHECK_OFF_SUBGROUP;
}

template <class F, class Fr> static int te(const std::string& xs, const std::string& ys) {
  Fe<F> mx, my, ym, yp, t, k, kt, x, y;
  to_mont<F>(mx, xs); to_mont<F>(my, ys);
  fe_sub(ym, my, mx); fe_add(yp, my, mx); fe_mul(t, mx, my);   // te_store_niels (gen_kernels.h)
  fe_set_const<F>(k, F::K2D); fe_mul(kt, t, k);
  TeNiels<F> b;
  resident<F>(b.ym, ym); resident<F>(b.yp, yp); resident<F>(b.kt, kt); resident<F>(x, mx);
  fe_add(y, b.ym, x); fe_carry(y);                              // k_te_check_curve
  if (!te_on_curve<F>(x, y)) return CHECK_OFF_CURVE;
  return te_point_times_order_is_zero<F, Fr>(b) ? 0 : CHECK_OFF_SUBGROUP;
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

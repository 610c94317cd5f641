// Host-side driver for msm_zprize_amd/csrc/mul_kernels.h: the chain [s]P and the final addition that k_points_mul /
// k_te_points_mul run, compiled for the CPU from the same templates.  Driven by tests/test_points_mul_cpu.py through
// stdin/stdout: one case per line
//   <curve> <s hex> <px hex> <py hex> <P at infinity: 0 / 1> <addend: 0 / 1> <qx hex> <qy hex> <Q at infinity: 0 / 1>
// in canonical form; the points are brought to the resident record's form (lazy Montgomery words, Niels form on the
// twisted Edwards curve) the way the upload kernels do, and [s]P (+ Q) is printed as  <x hex> <y hex> <infinity>.
// No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fp.h"
#include "../../msm_zprize_amd/csrc/curve.h"
#include "../../msm_zprize_amd/csrc/mul_kernels.h"
using namespace msmz;

template <int NW> static void parse(const std::string& h, uint32_t* w) {
  std::string s(NW * 8 - h.size(), '0'); s += h;
  for (int i = 0; i < NW; i++) w[i] = (uint32_t)strtoul(s.substr((NW - 1 - i) * 8, 8).c_str(), nullptr, 16);
}
template <int NW> static void print(const uint32_t* w) {
  for (int i = NW - 1; i >= 0; i--) printf("%08x", w[i]);
}

template <class F> static void to_mont(Fe<F>& r, const std::string& h) {
  uint32_t w[F::NW];
  Fe<F> c;
  parse<F::NW>(h, w);
  fe_unpack<F>(c, w);
  fe_to_mont(r, c);
}
// canonical words -> the value a kernel unpacks from a resident record: Montgomery form, stored to [0, 3p), reloaded
template <class F> static void resident(Fe<F>& r, const Fe<F>& mont) {
  uint32_t w[F::NW];
  fe_store<F>(w, mont);
  fe_unpack<F>(r, w);
}

struct Case {
  std::string s, px, py, qx, qy;
  int pinf, addend, qinf;
};

template <class F> static bool weier_load(Affine<F>& a, const std::string& xs, const std::string& ys, int inf) {
  Affine<F> m;
  to_mont<F>(m.x, xs); to_mont<F>(m.y, ys);
  resident<F>(a.x, m.x); resident<F>(a.y, m.y);
  return inf != 0;   // (the all-zero record of a flagged point: load_affine reports it, the coordinates are not read)
}

template <class F, class Fr> static void weier(const Case& c) {
  uint32_t s[8];
  parse<8>(c.s, s);
  Affine<F> p, q;
  const bool pinf = weier_load<F>(p, c.px, c.py, c.pinf);
  Xyzz<F> r;
  if (c.addend) {
    const bool qinf = weier_load<F>(q, c.qx, c.qy, c.qinf);
    point_times_scalar_plus<F, Fr>(r, p, pinf, s, q, qinf);
  } else {
    point_times_scalar<F, Fr>(r, p, pinf, s);
  }
  uint32_t w[2 * F::NW];
  const bool inf = fe_is_zero_mod_p(r.ZZZ) || xyzz_to_affine_canon<F>(w, r);   // the kernel's test, then the conversion
  if (inf) for (int i = 0; i < 2 * F::NW; i++) w[i] = 0;
  print<F::NW>(w); printf(" "); print<F::NW>(w + F::NW); printf(" %d\n", inf ? 1 : 0);
}

template <class F> static void te_load(TeNiels<F>& b, const std::string& xs, const std::string& ys) {
  Fe<F> mx, my, ym, yp, t, k, kt;
  to_mont<F>(mx, xs); to_mont<F>(my, ys);
  fe_sub(ym, my, mx); fe_add(yp, my, mx); fe_mul(t, mx, my);   // te_store_niels (gen_kernels.h)
  fe_set_const<F>(k, F::K2D); fe_mul(kt, t, k);
  resident<F>(b.ym, ym); resident<F>(b.yp, yp); resident<F>(b.kt, kt);
}

template <class F, class Fr> static void te(const Case& c) {
  uint32_t s[8];
  parse<8>(c.s, s);
  TeNiels<F> p, q;
  te_load<F>(p, c.px, c.py);
  TeExt<F> r;
  if (c.addend) {
    te_load<F>(q, c.qx, c.qy);
    te_point_times_scalar_plus<F, Fr>(r, p, s, q);
  } else {
    te_point_times_scalar<F, Fr>(r, p, s);
  }
  uint32_t w[2 * F::NW];
  te_to_affine_canon<F>(w, r);
  print<F::NW>(w); printf(" "); print<F::NW>(w + F::NW); printf(" 0\n");
}

int main() {
  std::string curve;
  Case c;
  while (std::cin >> curve >> c.s >> c.px >> c.py >> c.pinf >> c.addend >> c.qx >> c.qy >> c.qinf) {
    if (curve == "bls12-377") weier<Bls377Fp, Bls377Fr>(c);
    else if (curve == "pallas") weier<PallasFp, PallasFr>(c);
    else if (curve == "bls12-381") weier<Bls381Fp, Bls381Fr>(c);
    else if (curve == "ed-on-bls12-377") te<Ed377Fp, Ed377Fr>(c);
    else printf("?\n");
  }
  printf("products %d %d %d %d\n", points_mul_products<Bls377Fr>(false, true), points_mul_products<PallasFr>(false, true),
         points_mul_products<Bls381Fr>(false, true), points_mul_products<Ed377Fr>(true, true));
  return 0;
}

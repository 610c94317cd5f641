// Host-side driver for msm_zprize_amd/csrc/mul_kernels.h: the chain [s]P and the final addition that k_points_mul
// runs over the groups of curve.h, compiled for the CPU from the same templates.  Driven by tests/test_points_mul_cpu.py through
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

// a canonical point as the base a kernel loads from its resident record
template <class G> static void load(typename G::Base& b, const std::string& xs, const std::string& ys, int inf) {
  using F = typename G::F;
  Fe<F> mx, my;
  to_mont<F>(mx, xs); to_mont<F>(my, ys);
  if constexpr (G::TE) {
    typename G::Base n;
    G::base_from_affine(n, mx, my, false);   // TePolicy::store_resident (kernels.h)
    resident<F>(b.ym, n.ym); resident<F>(b.yp, n.yp); resident<F>(b.kt, n.kt);
  } else {
    Fe<F> x, y;
    resident<F>(x, mx); resident<F>(y, my);
    // (the all-zero record of a flagged point: load_affine reports it, the coordinates are not read)
    G::base_from_affine(b, x, y, inf != 0);
  }
}

template <class G, class Fr> static void run(const Case& c) {
  using F = typename G::F;
  uint32_t s[8];
  parse<8>(c.s, s);
  typename G::Base p, q;
  load<G>(p, c.px, c.py, c.pinf);
  typename G::Acc r;
  if (c.addend) {
    load<G>(q, c.qx, c.qy, c.qinf);
    group_times_scalar_plus<G, Fr>(r, p, s, q);
  } else {
    group_times_scalar<G, Fr>(r, p, s);
  }
  uint32_t w[2 * F::NW];
  // the kernel's test, then the conversion (twisted Edwards: Z != 0 for every multiple of a point of the curve)
  const bool inf = !G::TE && (fe_is_zero_mod_p(G::denominator(r)) || G::is_identity(r));
  if (inf) for (int i = 0; i < 2 * F::NW; i++) w[i] = 0; else G::to_affine_canon(w, r);
  print<F::NW>(w); printf(" "); print<F::NW>(w + F::NW); printf(" %d\n", inf ? 1 : 0);
}

int main() {
  std::string curve;
  Case c;
  while (std::cin >> curve >> c.s >> c.px >> c.py >> c.pinf >> c.addend >> c.qx >> c.qy >> c.qinf) {
    if (curve == "bls12-377") run<WeierGroup<Bls377Fp>, Bls377Fr>(c);
    else if (curve == "pallas") run<WeierGroup<PallasFp>, PallasFr>(c);
    else if (curve == "bls12-381") run<WeierGroup<Bls381Fp>, Bls381Fr>(c);
    else if (curve == "ed-on-bls12-377") run<TeGroup<Ed377Fp>, Ed377Fr>(c);
    else printf("?\n");
  }
  printf("products %d %d %d %d\n", points_mul_products<Bls377Fr>(false, true), points_mul_products<PallasFr>(false, true),
         points_mul_products<Bls381Fr>(false, true), points_mul_products<Ed377Fr>(true, true));
  return 0;
}

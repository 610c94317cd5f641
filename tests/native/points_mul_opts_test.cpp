// Host-side driver for the chains of msmz_points_mul_opts (msm_zprize_amd/csrc/mul_kernels.h): the bounded plain chain
// and the GLV chain (table, joint walk) that k_points_mul / k_points_mul_glv run, compiled for the CPU from the same
// templates.  Driven by tests/test_points_mul_opts_cpu.py through stdin/stdout: one case per line
//   <curve> <plain | glv> <bits> <s hex> <px hex> <py hex> <P at infinity: 0 / 1> <addend: 0 / 1> <qx hex> <qy hex> <Q at infinity>
// in canonical form; the points are brought to the resident record's form the way the upload kernels do.  `plain` walks
// `bits` bits of s; `glv` decomposes s with the real glv_decompose, builds the table (the inverse of the unequal-sign
// case comes from fe_inverse, where the kernel shares one across a wave) and walks the halves.  Printed per case:
//   <x hex> <y hex> <infinity> <neg0> <neg1> <inverted: 0 / 1>
// and after the last case the chain choices and the cost models.  No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fp.h"
#include "../../msm_zprize_amd/csrc/curve.h"
#include "../../msm_zprize_amd/csrc/scalar.h"
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
  std::string mode, s, px, py, qx, qy;
  int bits, pinf, addend, qinf;
};

// a canonical point as the base a kernel loads from its resident record
template <class G> static void load(typename G::Base& b, const std::string& xs, const std::string& ys, int inf) {
  using F = typename G::F;
  Fe<F> mx, my;
  to_mont<F>(mx, xs); to_mont<F>(my, ys);
  if constexpr (G::TE) {
    typename G::Base n;
    G::base_from_affine(n, mx, my, false);
    resident<F>(b.ym, n.ym); resident<F>(b.yp, n.yp); resident<F>(b.kt, n.kt);
  } else {
    Fe<F> x, y;
    resident<F>(x, mx); resident<F>(y, my);
    if (inf) { fe_zero(x); fe_zero(y); }   // the all-zero record of a flagged point
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
  uint32_t neg0 = 0, neg1 = 0;
  int inverted = 0;
  if (c.mode == "glv") {
    if constexpr (Fr::HAS_GLV) {
      uint32_t k0[4], k1[4];
      glv_decompose<Fr>(k0, k1, neg0, neg1, s);
      GlvFlags tb;
      GlvSlotsRegs<F> slots;
      Fe<F> d, inv;
      glv_table_begin<G>(tb, slots, d, p, neg0, neg1);
      fe_set_const<F>(inv, F::ONE);
      if (tb.flip && !tb.t_inf) {   // (the lanes that feed their own d to the wave's inversion)
        fe_inverse(inv, d);
        inverted = 1;
      }
      glv_table_finish<G>(tb, slots, inv);
      group_times_glv<G, Fr>(r, tb, slots, k0, k1);
    } else {
      printf("?\n");
      return;
    }
  } else {
    group_times_scalar<G, Fr>(r, p, s, c.bits);
  }
  if (c.addend) {
    typename G::Acc t;
    load<G>(q, c.qx, c.qy, c.qinf);
    G::madd(t, r, q);
    r = t;
  }
  uint32_t w[2 * F::NW];
  const bool inf = !G::TE && (fe_is_zero_mod_p(G::denominator(r)) || G::is_identity(r));
  if (inf) for (int i = 0; i < 2 * F::NW; i++) w[i] = 0; else G::to_affine_canon(w, r);
  print<F::NW>(w); printf(" "); print<F::NW>(w + F::NW); printf(" %d %u %u %d\n", inf ? 1 : 0, neg0, neg1, inverted);
}

template <class Fr> static void chains(const char* label) {
  const int bs[5] = {0, 64, Fr::GLV_PROVEN_BITS, Fr::GLV_PROVEN_BITS + 1, 256};
  for (int flag = 0; flag < 2; flag++)
    for (int b : bs) {
      const MulChain ch = points_mul_chain<Fr>(flag != 0, b);
      printf("chain %s %d %d %d %d\n", label, flag, b, ch.kind, ch.steps);
    }
}

int main() {
  std::string curve;
  Case c;
  while (std::cin >> curve >> c.mode >> c.bits >> c.s >> c.px >> c.py >> c.pinf >> c.addend >> c.qx >> c.qy >> c.qinf) {
    if (curve == "bls12-377") run<WeierGroup<Bls377Fp>, Bls377Fr>(c);
    else if (curve == "pallas") run<WeierGroup<PallasFp>, PallasFr>(c);
    else if (curve == "bls12-381") run<WeierGroup<Bls381Fp>, Bls381Fr>(c);
    else if (curve == "ed-on-bls12-377") run<TeGroup<Ed377Fp>, Ed377Fr>(c);
    else printf("?\n");
  }
  chains<Bls377Fr>("bls12-377");
  chains<PallasFr>("pallas");
  chains<Bls381Fr>("bls12-381");
  chains<Ed377Fr>("ed-on-bls12-377");
  printf("products_glv %d %d %d %d %d %d\n", points_mul_products_glv<Bls377Fr>(true), points_mul_products_glv<PallasFr>(true),
         points_mul_products_glv<Bls381Fr>(true), points_mul_products_glv<Bls377Fr>(false),
         points_mul_products_glv<PallasFr>(false), points_mul_products_glv<Bls381Fr>(false));
  printf("products_bounded %d %d %d %d\n", points_mul_products_bounded<Bls377Fr>(false, true, 128),
         points_mul_products_bounded<PallasFr>(false, true, 128), points_mul_products_bounded<Bls381Fr>(false, true, 64),
         points_mul_products_bounded<Ed377Fr>(true, true, 128));
  return 0;
}

// Host-side driver for msm_zprize_amd/csrc/fixed_base.h: the digit slicer, the planner and the group steps that
// k_fixed_table and k_fixed_mul run, compiled for the CPU from the same MSMZ_HD functions.  Driven by
// tests/test_fixed_base_cpu.py through stdin/stdout, one request per line:
//   digits <c> <K> <s hex>                          ->  the K signed digits of s, bottom first
//   mul <curve> <c> <bits> <s hex> <bx hex> <by hex> <B at infinity: 0 / 1>
//                                                   ->  [s]B as  <x hex> <y hex> <infinity>, accumulated over a table
//                                                       built here the way the kernels build and read theirs
//   plan <curve> <n> <bits>                         ->  <c> <K> <entries> <record bytes>
//   products <curve> <c> <K>                        ->  <per entry> <per point>
// Values are canonical; `bits` is the bound as fixed_base_bits normalises it (0 = none).  No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fp.h"
#include "../../msm_zprize_amd/csrc/curve.h"
#include "../../msm_zprize_amd/csrc/fixed_base.h"
using namespace msmz;

template <int NW> static void parse(const std::string& h, uint32_t* w) {
  std::string s(NW * 8 - h.size(), '0'); s += h;
  for (int i = 0; i < NW; i++) w[i] = (uint32_t)strtoul(s.substr((NW - 1 - i) * 8, 8).c_str(), nullptr, 16);
}
template <int NW> static void print(const uint32_t* w) {
  for (int i = NW - 1; i >= 0; i--) printf("%08x", w[i]);
}

// The table of one (curve, base, c): the bases 2^(ck) B as PointOps::window_bases (point_ops.h) computes them on the host, and the
// entries as k_fixed_table computes and stores them -- built when first read, since a test reads a few hundred of the
// up to 2^19.
template <class G> struct Table {
  using F = typename G::F;
  static constexpr int RW = 2 * F::NW;
  int c;
  std::vector<uint32_t> bases;                       // K records, all zero: the point at infinity
  std::map<uint32_t, std::vector<uint32_t>> entries;

  Table(int c_, int K, const std::string& bx, const std::string& by, int binf) : c(c_), bases((size_t)K * RW, 0) {
    uint32_t w[RW];
    parse<F::NW>(bx, w); parse<F::NW>(by, w + F::NW);
    Fe<F> cx, cy, x, y;
    fe_unpack<F>(cx, w); fe_unpack<F>(cy, w + F::NW);
    fe_to_mont(x, cx); fe_to_mont(y, cy);
    typename G::Acc g, t;
    if (!G::TE && binf) G::set_identity(g); else G::from_affine(g, x, y);
    for (int k = 0; k < K; k++) {
      if (G::TE || !fe_is_zero_mod_p(G::denominator(g))) {
        Fe<F> inv;
        fe_inverse(inv, G::denominator(g));
        G::affine_from_inverse(x, y, g, inv);
        fe_store<F>(bases.data() + (size_t)k * RW, x);
        fe_store<F>(bases.data() + (size_t)k * RW + F::NW, y);
      }
      for (int j = 0; j < c; j++) { G::dbl(t, g); g = t; }
    }
  }

  static bool unpack(Fe<F>& x, Fe<F>& y, const uint32_t* rec) {
    fe_unpack<F>(x, rec); fe_unpack<F>(y, rec + F::NW);
    return words_point_is_inf<F>(rec);
  }

  const uint32_t* entry(uint32_t idx) {
    auto it = entries.find(idx);
    if (it != entries.end()) return it->second.data();
    const uint32_t k = idx >> (c - 1), w = (idx & ((1u << (c - 1)) - 1u)) + 1u;
    Fe<F> x, y;
    const bool inf = unpack(x, y, bases.data() + (size_t)k * RW);
    typename G::Base b;
    fixed_entry_base<G>(b, x, y, inf, 0);
    typename G::Acc acc;
    fixed_table_multiple<G>(acc, b, w, c);
    std::vector<uint32_t> rec(RW, 0);
    const bool dead = fe_is_zero_mod_p(G::denominator(acc));
    if (!dead) {
      Fe<F> inv;
      fe_inverse(inv, G::denominator(acc));
      G::affine_from_inverse(x, y, acc, inv);
      fe_store<F>(rec.data(), x); fe_store<F>(rec.data() + F::NW, y);
    } else if (G::TE) {
      fe_zero(x); fe_set_const<F>(y, F::ONE);
      fe_store<F>(rec.data(), x); fe_store<F>(rec.data() + F::NW, y);
    }
    return entries.emplace(idx, std::move(rec)).first->second.data();
  }
};

template <class G, class Fr> static void mul(std::istringstream& in, const std::string& curve) {
  using F = typename G::F;
  int c, bits, binf;
  std::string ss, bx, by;
  in >> c >> bits >> ss >> bx >> by >> binf;
  const int K = fixed_base_windows(fixed_base_bits(bits, Fr::BITS), c);
  static std::map<std::string, Table<G>*> tables;
  std::ostringstream key;
  key << curve << ' ' << c << ' ' << K << ' ' << bx << ' ' << by << ' ' << binf;
  Table<G>*& tb = tables[key.str()];
  if (!tb) tb = new Table<G>(c, K, bx, by, binf);
  uint32_t s[8];
  parse<8>(ss, s);
  FixedDigits dg;
  fixed_digits_begin(dg, s);
  typename G::Acc acc;
  G::set_identity(acc);
  for (int k = 0; k < K; k++) {
    const int32_t d = fixed_digits_next(dg, c);
    if (d == 0) continue;
    const uint32_t idx = fixed_entry_index(k, d, c);
    if (idx >= fixed_base_entries(c, K)) { printf("index out of the table\n"); return; }
    Fe<F> x, y;
    const bool inf = Table<G>::unpack(x, y, tb->entry(idx));
    fixed_add_entry<G>(acc, x, y, inf, d < 0 ? 1u : 0u);
  }
  uint32_t w[2 * F::NW];
  const bool inf = !G::TE && (fe_is_zero_mod_p(G::denominator(acc)) || G::is_identity(acc));
  if (inf) for (int i = 0; i < 2 * F::NW; i++) w[i] = 0; else G::to_affine_canon(w, acc);
  print<F::NW>(w); printf(" "); print<F::NW>(w + F::NW); printf(" %d\n", inf ? 1 : 0);
}

template <class G, class Fr> static void plan(std::istringstream& in) {
  unsigned long long n;
  int bits;
  in >> n >> bits;
  const int rec = 2 * G::F::NW * 4;
  const FixedPlan p = fixed_base_plan(n, fixed_base_bits(bits, Fr::BITS), G::TE, rec);
  printf("%d %d %llu %d\n", p.c, p.K, (unsigned long long)p.entries, rec);
}

template <class G, class Fr> static void products(std::istringstream& in) {
  int c, K;
  in >> c >> K;
  printf("%d %d\n", fixed_entry_products(G::TE, c), fixed_point_products(G::TE, K));
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, curve;
    in >> cmd;
    if (cmd == "digits") {
      int c, K;
      std::string ss;
      in >> c >> K >> ss;
      uint32_t s[8];
      parse<8>(ss, s);
      FixedDigits dg;
      fixed_digits_begin(dg, s);
      for (int k = 0; k < K; k++) printf("%d%c", fixed_digits_next(dg, c), k + 1 == K ? '\n' : ' ');
      continue;
    }
    in >> curve;
#define DISPATCH(fn, ...)                                                                   \
  do {                                                                                      \
    if (curve == "bls12-377") fn<WeierGroup<Bls377Fp>, Bls377Fr>(__VA_ARGS__);              \
    else if (curve == "pallas") fn<WeierGroup<PallasFp>, PallasFr>(__VA_ARGS__);            \
    else if (curve == "bls12-381") fn<WeierGroup<Bls381Fp>, Bls381Fr>(__VA_ARGS__);         \
    else if (curve == "ed-on-bls12-377") fn<TeGroup<Ed377Fp>, Ed377Fr>(__VA_ARGS__);        \
    else printf("?\n");                                                                     \
  } while (0)
    if (cmd == "mul") DISPATCH(mul, in, curve);
    else if (cmd == "plan") DISPATCH(plan, in);
    else if (cmd == "products") DISPATCH(products, in);
    else printf("?\n");
  }
  return 0;
}

// Host-side driver for the F_q inversion and the affine maps of msm_zprize_amd/csrc/fr.h and for the per-thread bodies
// of scan_kernels.h (k_scalars_rec_tile / _carry / _apply, k_scalars_inverse), compiled for the CPU from the same
// templates.  Driven by tests/test_scalar_scan_cpu.py through stdin/stdout, one request per line, values as hex:
//   <curve> inv <x>                          ->  <fr_inv(x)> <x * fr_inv(x)>
//   <curve> map <a2> <b2> <a1> <b1>          ->  <A> <B> of (a2, b2) o (a1, b1), A out of Montgomery form
//   <curve> map3 <a3> <b3> <a2> <b2> <a1> <b1>
//                                            ->  <A> <B> of (m3 o m2) o m1, then <A> <B> of m3 o (m2 o m1)
//   <curve> rec <am> <hb> <flags> <n> <init> <k> <a_0 .. a_(n-1) if am == 2> <b_0 .. b_(n-1) if hb>
//                                            ->  n output entries and the final value: the runs of SREC_E positions are
//                                                composed (srec_compose_run), combined in order (fr_map_compose), applied
//                                                to init (fr_map_apply) and walked (srec_walk_run), as the three kernels
//                                                chain them; am: 0 no multiplier, 1 broadcast k, 2 resident
//   <curve> sinv <count> <x_0 .. x_(count-1)> ->  count inverses and the zero mask: one thread of k_scalars_inverse
//                                                (sinv_forward, fr_inv of its total, sinv_backward), count <= SINV_E
//   geometry                                 ->  SREC_TILE SREC_PASS SINV_CHUNK SREC_E SINV_E
// No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fr.h"
#include "../../msm_zprize_amd/csrc/scan_kernels.h"
using namespace msmz;

static void parse(const std::string& h, uint32_t* w) {
  std::string s(64 - h.size(), '0'); s += h;
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)strtoul(s.substr((7 - i) * 8, 8).c_str(), nullptr, 16);
}
static void print(const uint32_t* w, const char* end) {
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
  printf("%s", end);
}
static void read_value(uint32_t* w) {
  std::string s;
  std::cin >> s;
  parse(s, w);
}

// a map from canonical (a, b); and back
template <class Fr> static void make_map(FrMap& m, const uint32_t* a, const uint32_t* b) {
  fr_to_mont<Fr>(m.A, a);
  for (int j = 0; j < 8; j++) m.B[j] = b[j];
}
template <class Fr> static void print_map(const FrMap& m, const char* end) {
  const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  uint32_t a[8];
  fr_mont_mul<Fr>(a, m.A, one);
  print(a, " "); print(m.B, end);
}

template <class Fr, int AM, bool HB>
static void recurrence(uint32_t flags, uint64_t n, const uint32_t* init, const uint32_t* k, const uint32_t* a,
                       const uint32_t* b) {
  constexpr bool HA = AM != SREC_A_NONE;
  const bool rev = flags & SREC_REVERSE, excl = flags & SREC_EXCLUSIVE;
  const uint64_t runs = (n + SREC_E - 1) / SREC_E;
  std::vector<uint32_t> out(n * 8, 0xa5a5a5a5u);
  FrMap before;   // the composition of the runs so far
  fr_map_identity<Fr, HA, HB>(before);
  uint32_t y[8];
  for (uint64_t r = 0; r < runs; r++) {
    FrMap m;
    if (srec_compose_run<Fr, AM, HB>(m, a, b, k, r * SREC_E, n, rev)) { printf("range\n"); return; }
    for (int j = 0; j < 8; j++) y[j] = init[j];
    fr_map_apply<Fr, HA, HB>(y, before);   // the incoming value of run r
    srec_walk_run<Fr, AM, HB>(out.data(), y, a, b, k, r * SREC_E, n, rev, excl);
    fr_map_compose<Fr, HA, HB>(before, m, before);
    uint32_t z[8];
    for (int j = 0; j < 8; j++) z[j] = init[j];
    fr_map_apply<Fr, HA, HB>(z, before);
    for (int j = 0; j < 8; j++)
      if (z[j] != y[j]) { printf("mismatch\n"); return; }   // the walk and the composed map agree on the run's end
  }
  for (uint64_t i = 0; i < n; i++) print(out.data() + i * 8, " ");
  print(y, "\n");
}

template <class Fr> static void run(const std::string& op) {
  if (op == "inv") {
    uint32_t x[8], r[8], p[8];
    read_value(x);
    fr_inv<Fr>(r, x);
    fr_mul<Fr>(p, x, r);
    print(r, " "); print(p, "\n");
  } else if (op == "map" || op == "map3") {
    const int count = op == "map" ? 2 : 3;
    FrMap m[3];
    for (int i = count - 1; i >= 0; i--) {   // the last map of the composition comes first on the line
      uint32_t a[8], b[8];
      read_value(a); read_value(b);
      make_map<Fr>(m[i], a, b);
    }
    FrMap r, s;
    if (count == 2) {
      fr_map_compose<Fr, true, true>(r, m[1], m[0]);
      print_map<Fr>(r, "\n");
    } else {
      fr_map_compose<Fr, true, true>(r, m[2], m[1]);
      fr_map_compose<Fr, true, true>(r, r, m[0]);
      fr_map_compose<Fr, true, true>(s, m[1], m[0]);
      fr_map_compose<Fr, true, true>(s, m[2], s);
      print_map<Fr>(r, " "); print_map<Fr>(s, "\n");
    }
  } else if (op == "rec") {
    int am, hb;
    unsigned flags;
    unsigned long long n;
    std::cin >> am >> hb >> flags >> n;
    uint32_t init[8], kc[8], k[8];
    read_value(init); read_value(kc);
    fr_to_mont<Fr>(k, kc);
    std::vector<uint32_t> a(am == 2 ? n * 8 : 8), b(hb ? n * 8 : 8);
    if (am == 2) for (unsigned long long i = 0; i < n; i++) read_value(a.data() + i * 8);
    if (hb) for (unsigned long long i = 0; i < n; i++) read_value(b.data() + i * 8);
    if (am == 0 && hb) recurrence<Fr, SREC_A_NONE, true>(flags, n, init, k, a.data(), b.data());
    else if (am == 1 && !hb) recurrence<Fr, SREC_A_BROADCAST, false>(flags, n, init, k, a.data(), b.data());
    else if (am == 1 && hb) recurrence<Fr, SREC_A_BROADCAST, true>(flags, n, init, k, a.data(), b.data());
    else if (am == 2 && !hb) recurrence<Fr, SREC_A_RESIDENT, false>(flags, n, init, k, a.data(), b.data());
    else if (am == 2 && hb) recurrence<Fr, SREC_A_RESIDENT, true>(flags, n, init, k, a.data(), b.data());
    else printf("?\n");
  } else if (op == "sinv") {
    unsigned count;
    std::cin >> count;
    if (count > (unsigned)SINV_E) count = SINV_E;
    std::vector<uint32_t> x(SINV_E * 8), out(SINV_E * 8, 0xa5a5a5a5u);
    for (unsigned i = 0; i < count; i++) read_value(x.data() + i * 8);
    uint32_t P[SINV_E][8], zeros, inv[8];
    if (sinv_forward<Fr>(P, &zeros, x.data(), 0, count)) { printf("range\n"); return; }
    fr_inv<Fr>(inv, P[SINV_E - 1]);
    sinv_backward<Fr>(out.data(), x.data(), P, inv, zeros, 0, count);
    for (unsigned i = 0; i < count; i++) print(out.data() + i * 8, " ");
    printf("%x\n", zeros);
  } else {
    printf("?\n");
  }
}

int main() {
  std::string curve, op;
  while (std::cin >> curve) {
    if (curve == "geometry") { printf("%d %d %d %d %d\n", SREC_TILE, SREC_PASS, SINV_CHUNK, SREC_E, SINV_E); continue; }
    std::cin >> op;
    if (curve == "bls12-377") run<Bls377Fr>(op);
    else if (curve == "pallas") run<PallasFr>(op);
    else if (curve == "bls12-381") run<Bls381Fr>(op);
    else if (curve == "ed-on-bls12-377") run<Ed377Fr>(op);
    else printf("?\n");
  }
  return 0;
}

// Host-side driver for msm_zprize_amd/csrc/dot_kernels.h: fr_dot_many_index, what one thread of k_scalars_dot_many does
// for one element index (NC column values, then RG row values, RG x NC products into the register block), compiled for
// the CPU from the same template, and the planner dot_many_plan.  Driven by tests/test_dot_many_cpu.py through
// stdin/stdout, one request per line, values as hex:
//   <curve> block <nc> <live> <count>  then per element index the nc column values and the `live` row values
//       (1 <= live <= rg = dot_many_rg(nc); the rows beyond `live` are the row tail: predicated off, never loaded --
//       the driver aborts if the body asks for one -- and their sums must stay zero)
//       ->  live * nc values, row-major: the block's sums over the `count` indices, converted as k_scalars_dot_fold does
//   plan <n> <max_groups>  ->  for every n_rows 1 .. 128 and n_cols 1 .. 8, row-major: rg tiles groups row_groups
//       scratch_bytes (decimal)
//   geometry  ->  SDOT_TILE SDOT_THREADS SDOT_E DOT_MANY_GROUPS MAX_ROWS MAX_COLS sizeof(DotManyVecs), then
//       dot_many_rg(1 .. 8) (decimal)
// A stand-alone program: the same file built with -fsanitize=address,undefined runs the same requests.  No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fr.h"
#include "../../msm_zprize_amd/csrc/dot_kernels.h"
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
  return s.size() > 64 ? Rec{} : parse(s);
}
static void print(const uint32_t* w) {
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
}

template <class Fr, int NC>
static void block(unsigned live, unsigned count) {
  constexpr int RG = dot_many_rg(NC);
  if (live < 1 || live > (unsigned)RG || count < 1 || count > 256) {
    printf("?\n");
    return;
  }
  std::vector<Rec> col((size_t)count * NC), row((size_t)count * live);
  for (unsigned i = 0; i < count; i++) {
    for (int c = 0; c < NC; c++) col[(size_t)i * NC + c] = read();
    for (unsigned j = 0; j < live; j++) row[(size_t)i * live + j] = read();
  }
  uint32_t acc[RG][NC][8] = {};
  for (unsigned i = 0; i < count; i++) {
    fr_dot_many_index<Fr, NC, RG>(
        acc, live,
        [&](auto C, uint32_t* out) {
          for (int w = 0; w < 8; w++) out[w] = col[(size_t)i * NC + C].w[w];
          return false;
        },
        [&](auto J, uint32_t* out) {
          if ((unsigned)J >= live) abort();   // (the row tail is never loaded)
          for (int w = 0; w < 8; w++) out[w] = row[(size_t)i * live + (unsigned)J].w[w];
          return false;
        });
  }
  for (unsigned j = live; j < (unsigned)RG; j++)
    for (int c = 0; c < NC; c++)
      for (int w = 0; w < 8; w++)
        if (acc[j][c][w]) abort();   // (a surplus row's sums stay zero)
  for (unsigned j = 0; j < live; j++) {
    for (int c = 0; c < NC; c++) {
      uint32_t r[8];
      fr_to_mont<Fr>(r, acc[j][c]);
      print(r), printf(j + 1 == live && c + 1 == NC ? "\n" : " ");
    }
  }
}

template <class Fr> static void run(const std::string& op) {
  unsigned nc = 0, live = 0, count = 0;
  if (op != "block" || !(std::cin >> nc >> live >> count)) {
    printf("?\n");
    return;
  }
  switch (nc) {
    case 1: block<Fr, 1>(live, count); break;
    case 2: block<Fr, 2>(live, count); break;
    case 3: block<Fr, 3>(live, count); break;
    case 4: block<Fr, 4>(live, count); break;
    case 5: block<Fr, 5>(live, count); break;
    case 6: block<Fr, 6>(live, count); break;
    case 7: block<Fr, 7>(live, count); break;
    case 8: block<Fr, 8>(live, count); break;
    default: printf("?\n");
  }
  static_assert(DOT_MANY_MAX_COLS == 8, "one case per column count");
}

int main() {
  std::string curve, op;
  while (std::cin >> curve) {
    if (curve == "geometry") {
      printf("%d %d %d %u %d %d %zu", SDOT_TILE, SDOT_THREADS, SDOT_E, DOT_MANY_GROUPS, DOT_MANY_MAX_ROWS, DOT_MANY_MAX_COLS,
             sizeof(DotManyVecs));
      for (int nc = 1; nc <= DOT_MANY_MAX_COLS; nc++) printf(" %d", dot_many_rg(nc));
      printf("\n");
      continue;
    }
    if (curve == "plan") {
      unsigned long long n = 0;
      unsigned max_groups = 0;
      if (!(std::cin >> n >> max_groups) || n < 1 || n >> 32 || max_groups < 1 || max_groups > DOT_MANY_GROUPS) {
        std::cin.clear();
        printf("?\n");
        continue;
      }
      for (uint32_t r = 1; r <= (uint32_t)DOT_MANY_MAX_ROWS; r++) {
        for (uint32_t c = 1; c <= (uint32_t)DOT_MANY_MAX_COLS; c++) {
          const DotManyPlan p = dot_many_plan(n, r, c, max_groups);
          printf("%u %u %u %u %llu ", p.rg, p.tiles, p.groups, p.row_groups, (unsigned long long)p.scratch_bytes);
        }
      }
      printf("\n");
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

// Host driver for what the exports (msmz_export_scalars / _points) compute off the GPU: fr_to_mont and fr_from_mont
// (msm_zprize_amd/csrc/fr.h, scalar.h), the export constant RSTD of constants_gen.h, and the layout of msmz_dst.
// argv[1]: a file of lines "<field 0..3> <64 hex digits, big-endian>"; stdout, after the header lines
//   "layout <name> <sizeof> <offsets of ptr stride width flags stream is_inf>"   for msmz_src and msmz_dst
//   "const <field> RSTD <N> <W> <limb> ..."                                      (base-field limbs, signed decimal)
// one line "<field> <to_mont: 64 hex digits> <from_mont(to_mont): 64 hex digits>" per input line.
#include <cstddef>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include "../../include/msmz.h"
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fp.h"
#include "../../msm_zprize_amd/csrc/scalar.h"
#include "../../msm_zprize_amd/csrc/fr.h"

using namespace msmz;

static void put(const uint32_t* w) {
  for (int j = 7; j >= 0; j--) printf("%08x", w[j]);
}

template <class Fr>
static void convert(int field, const char* hex) {
  uint32_t a[8], m[8], back[8], alias[8];
  for (int j = 0; j < 8; j++) {
    char w[9];
    memcpy(w, hex + 8 * (7 - j), 8);
    w[8] = 0;
    a[j] = (uint32_t)strtoul(w, nullptr, 16);
  }
  fr_to_mont<Fr>(m, a);
  memcpy(alias, a, sizeof(a));
  fr_to_mont<Fr>(alias, alias);   // in place, as k_export_scalars calls it
  if (memcmp(alias, m, sizeof(m)) != 0) {
    printf("alias mismatch\n");
    return;
  }
  fr_from_mont<Fr>(back, m);
  printf("%d ", field);
  put(m);
  printf(" ");
  put(back);
  printf("\n");
}

template <class F>
static void constants(int field) {
  printf("const %d RSTD %d %d", field, F::N, F::W);
  for (int j = 0; j < F::N; j++) printf(" %d", F::RSTD[j]);
  printf("\n");
}

#define LAYOUT(T)                                                                                                     \
  printf("layout " #T " %zu %zu %zu %zu %zu %zu %zu\n", sizeof(T), offsetof(T, ptr), offsetof(T, stride),              \
         offsetof(T, width), offsetof(T, flags), offsetof(T, stream), offsetof(T, is_inf))

int main(int argc, char** argv) {
  LAYOUT(msmz_src);
  LAYOUT(msmz_dst);
  constants<Bls377Fp>(0);
  constants<PallasFp>(1);
  constants<Bls381Fp>(2);
  constants<Ed377Fp>(3);
  if (argc < 2) return 0;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int field;
  char hex[80];
  while (fscanf(f, "%d %64s", &field, hex) == 2) {
    if (strlen(hex) != 64) return 3;
    switch (field) {
      case 0: convert<Bls377Fr>(field, hex); break;
      case 1: convert<PallasFr>(field, hex); break;
      case 2: convert<Bls381Fr>(field, hex); break;
      case 3: convert<Ed377Fr>(field, hex); break;
      default: return 4;
    }
  }
  fclose(f);
  return 0;
}

// Host driver for fr_from_mont (msm_zprize_amd/csrc/scalar.h) and the import constants of constants_gen.h.
// argv[1]: a file of lines "<field 0..3> <64 hex digits, big-endian>"; stdout: one line "<field> <64 hex digits>" per
// input line with a * 2^-256 mod q, after the constants:
//   "const <field> QINV32 <hex>"  and  "const <field> R2STD|R2 <N> <W> <limb> ..." (base-field limbs, signed decimal).
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fp.h"
#include "../../msm_zprize_amd/csrc/scalar.h"

using namespace msmz;

template <class Fr>
static void convert(int field, const char* hex) {
  uint32_t a[8], r[8];
  for (int j = 0; j < 8; j++) {
    char w[9];
    memcpy(w, hex + 8 * (7 - j), 8);
    w[8] = 0;
    a[j] = (uint32_t)strtoul(w, nullptr, 16);
  }
  fr_from_mont<Fr>(r, a);
  fr_from_mont<Fr>(a, a);   // in place gives the same
  if (memcmp(a, r, sizeof(a)) != 0) {
    printf("alias mismatch\n");
    return;
  }
  printf("%d ", field);
  for (int j = 7; j >= 0; j--) printf("%08x", r[j]);
  printf("\n");
}

template <class F, class Fr>
static void constants(int field) {
  printf("const %d QINV32 %08x\n", field, Fr::QINV32);
  printf("const %d R2STD %d %d", field, F::N, F::W);
  for (int j = 0; j < F::N; j++) printf(" %d", F::R2STD[j]);
  printf("\nconst %d R2 %d %d", field, F::N, F::W);
  for (int j = 0; j < F::N; j++) printf(" %d", F::R2[j]);
  printf("\n");
}

int main(int argc, char** argv) {
  constants<Bls377Fp, Bls377Fr>(0);
  constants<PallasFp, PallasFr>(1);
  constants<Bls381Fp, Bls381Fr>(2);
  constants<Ed377Fp, Ed377Fr>(3);
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

// Host-side driver for the host-callable part of msm_zprize_amd/csrc/matrix_kernels.h: the counting sort that builds a
// form of a sparse matrix, and the product itself emulated tile by tile on the CPU from the same templates the kernels
// instantiate -- mat_run for each of the MAT_THREADS runs of a tile, the segmented scan as a sequential chain of
// mat_combine, mat_finish, and the carry fold (mat_fold_part / mat_fold_ends / mat_fold_apply) in passes of
// MAT_FOLD_PASS.  Driven by tests/test_matrix_cpu.py through stdin/stdout, one request per line, values as hex:
//   geometry                                             ->  MAT_TILE MAT_RUN MAT_FOLD_PASS
//   sort <n_keys> <nnz> then per triple <key> <other>     ->  nnz times "seg gidx perm" (decimal)
//   badindex <n_rows> <n_cols> <nnz> then per triple <row> <col>  ->  mat_first_bad_index (decimal)
//   <curve> mul <n_out> <n_in> <nnz> <has_vals> then per triple <seg> <gidx> [<val>], then n_in values of x
//        (the triples sorted by seg, val canonical)       ->  n_out values, then the error bit (0 / 1)
// No GPU needed.  Also built with -fsanitize=address,undefined and run over the same requests.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fr.h"
#include "../../msm_zprize_amd/csrc/matrix_kernels.h"
using namespace msmz;

static void parse(const std::string& h, uint32_t* w) {
  std::string s(64 - h.size(), '0'); s += h;
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)strtoul(s.substr((7 - i) * 8, 8).c_str(), nullptr, 16);
}
static void print(const uint32_t* w, const char* end) {
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
  printf("%s", end);
}

// records of 8 words, 16-byte aligned as device memory is
struct Records {
  std::vector<uint32_t> store;
  uint32_t* p;
  explicit Records(size_t n) : store(n * 8 + 4, 0) {
    p = store.data();
    while (reinterpret_cast<uintptr_t>(p) % 16) p++;
  }
};

template <class Fr> static void mul() {
  unsigned long long n_out, n_in, nnz;
  int has_vals;
  std::cin >> n_out >> n_in >> nnz >> has_vals;
  std::vector<uint32_t> seg(nnz), gidx(nnz);
  Records val(has_vals ? nnz : 0), x(n_in), out(n_out);
  std::string s;
  for (size_t k = 0; k < nnz; k++) {
    std::cin >> seg[k] >> gidx[k];
    if (has_vals) {
      std::cin >> s;
      uint32_t v[8];
      parse(s, v);
      fr_to_mont<Fr>(val.p + k * 8, v);   // what k_matrix_pack stores
    }
  }
  for (size_t i = 0; i < n_in; i++) {
    std::cin >> s;
    parse(s, x.p + i * 8);
  }
  const MatView m = {gidx.data(), seg.data(), has_vals ? val.p : nullptr};
  const uint32_t tiles = (uint32_t)((nnz + MAT_TILE - 1) / MAT_TILE);
  Records carry((size_t)tiles * MAT_CARRY_WORDS / 8);
  bool bad = false;
  // k_matrix_mul, one tile after the other (out was cleared: Records starts as zeros)
  for (uint32_t tile = 0; tile < tiles; tile++) {
    const uint64_t tile_first = (uint64_t)tile * MAT_TILE;
    const uint64_t tile_end = tile_first + MAT_TILE < nnz ? tile_first + MAT_TILE : nnz;
    std::vector<MatRun> runs(MAT_THREADS);
    std::vector<MatPart> parts(MAT_THREADS);
    std::vector<bool> active(MAT_THREADS);
    for (int t = 0; t < MAT_THREADS; t++) {
      const uint64_t first = tile_first + (uint64_t)t * MAT_RUN;
      active[t] = first < tile_end;
      mat_part_identity(parts[t]);
      if (!active[t]) continue;
      const uint64_t left = tile_end - first;
      mat_run<Fr>(runs[t], out.p, m, x.p, first, left < MAT_RUN ? (uint32_t)left : (uint32_t)MAT_RUN, tile_first, tile_end);
      mat_run_part(parts[t], runs[t]);
    }
    MatPart excl;   // the scan: excl = the parts of threads 0 .. t - 1 combined
    mat_part_identity(excl);
    for (int t = 0; t < MAT_THREADS; t++) {
      if (active[t]) {
        bad |= (runs[t].flags & MAT_BAD) != 0;
        mat_finish<Fr>(out.p, carry.p + (size_t)tile * MAT_CARRY_WORDS, runs[t], excl);
      }
      MatPart incl = parts[t];
      mat_combine<Fr>(incl, excl);
      excl = incl;
    }
  }
  // k_matrix_fold: passes of MAT_FOLD_PASS carries, the sum of a pass handed to the next
  MatPart pass_carry;
  mat_part_identity(pass_carry);
  for (uint32_t base = 0; base < tiles; base += MAT_FOLD_PASS) {
    MatPart excl;
    mat_part_identity(excl);
    MatPart last;
    mat_part_identity(last);
    for (uint32_t t = 0; t < (uint32_t)MAT_FOLD_PASS; t++) {
      const uint32_t c = base + t;
      MatPart a;
      mat_part_identity(a);
      if (c < tiles) mat_fold_part(a, carry.p, c);
      mat_combine<Fr>(a, excl);
      excl = a;
      mat_combine<Fr>(a, pass_carry);
      if (c < tiles && mat_fold_ends(carry.p, c, tiles)) mat_fold_apply<Fr>(out.p, carry.p[(size_t)c * MAT_CARRY_WORDS], a.v);
      last = a;
    }
    pass_carry = last;
  }
  for (size_t i = 0; i < n_out; i++) print(out.p + i * 8, " ");
  printf("%d\n", bad ? 1 : 0);
}

int main() {
  std::string curve, op;
  while (std::cin >> curve) {
    if (curve == "geometry") {
      printf("%d %d %d\n", MAT_TILE, MAT_RUN, MAT_FOLD_PASS);
      continue;
    }
    if (curve == "sort") {
      unsigned long long n_keys, nnz;
      std::cin >> n_keys >> nnz;
      std::vector<uint32_t> key(nnz), other(nnz), seg(nnz), gidx(nnz), perm(nnz);
      for (size_t k = 0; k < nnz; k++) std::cin >> key[k] >> other[k];
      mat_sort_form(key.data(), other.data(), nnz, (uint32_t)n_keys, seg.data(), gidx.data(), perm.data());
      for (size_t k = 0; k < nnz; k++) printf("%u %u %u%s", seg[k], gidx[k], perm[k], k + 1 == nnz ? "" : " ");
      printf("\n");
      continue;
    }
    if (curve == "badindex") {
      unsigned long long n_rows, n_cols, nnz;
      std::cin >> n_rows >> n_cols >> nnz;
      std::vector<uint32_t> row(nnz), col(nnz);
      for (size_t k = 0; k < nnz; k++) std::cin >> row[k] >> col[k];
      printf("%llu\n", (unsigned long long)mat_first_bad_index(row.data(), col.data(), nnz, (uint32_t)n_rows, (uint32_t)n_cols));
      continue;
    }
    std::cin >> op;
    if (op != "mul") printf("?\n");
    else if (curve == "bls12-377") mul<Bls377Fr>();
    else if (curve == "pallas") mul<PallasFr>();
    else if (curve == "bls12-381") mul<Bls381Fr>();
    else if (curve == "ed-on-bls12-377") mul<Ed377Fr>();
    else printf("?\n");
  }
  return 0;
}

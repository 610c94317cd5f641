// Host-side driver for the host/device half of msm_zprize_amd/csrc/expr_kernels.h: the index function, the overlap
// rule, the compile step and the body of one entry (fr_expr_entry, and fr_expr_entry_slots of the register-resident
// variant), run on the CPU from the same templates the kernels instantiate.  Driven by tests/test_expr_cpu.py through
// stdin/stdout, one request per line, field values as hex, everything else decimal:
//   geometry                                   ->  EXPR_THREADS EXPR_REGISTER_SLOTS EXPR_SLOTS_MAX sizeof(ExprProgram)
//   index <i> <rot> <n>                        ->  expr_index(i, expr_reduce_rot(rot, n), n)       (rot: any int32)
//   overlap <named> <first> <first_out> <n>    ->  expr_overlap_ok: 1 or 0
//   <curve> compile <DESC>                     ->  the status of expr_compile, the status of expr_coeffs (- if not
//        reached), and after two MSMZ_OK: n_ops rotated, the operands as column:rot, per term its operand indices
//        joined by ',' (- for none), named[c] per column, and per term its prepared coefficient
//   <curve> eval <slots> <DESC> then n_columns * n values, column by column
//        slots: 0 = fr_expr_entry, 2 | 4 | 8 = fr_expr_entry_slots of that size
//        ->  n values, then 1 if a record read was >= q, else 0     (or `status <st>` if the description is refused)
//   DESC = <n> <n_columns> <flags> <cols: ok|null> <terms: ok|null> <n_terms> then per term
//          <coeff: hex, or - for NULL> <reserved> <n_factors> <factors: ok|null> then, with ok, n_factors pairs <column> <rot>
// No GPU needed.  Also built with -fsanitize=address,undefined and run over the same requests.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fr.h"
#include "../../msm_zprize_amd/csrc/expr_kernels.h"
using namespace msmz;

static void parse(const std::string& h, uint32_t* w) {
  std::string s(64 - h.size(), '0'); s += h;
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)strtoul(s.substr((7 - i) * 8, 8).c_str(), nullptr, 16);
}
static void print(const uint32_t* w, const char* end) {
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
  printf("%s", end);
}

// a description as the caller of msmz_scalars_expr would hold it
struct Desc {
  msmz_expr e{};
  std::vector<msmz_expr_column> columns;
  std::vector<msmz_expr_term> terms;
  std::vector<std::vector<msmz_expr_factor>> factors;
  std::vector<std::vector<uint8_t>> coeffs;
  void read() {
    unsigned long long n;
    unsigned nc, flags, nt;
    std::string cols, trms;
    std::cin >> n >> nc >> flags >> cols >> trms >> nt;
    columns.assign(nc ? nc : 1, msmz_expr_column{0, 0});
    terms.assign(nt ? nt : 1, msmz_expr_term{});
    factors.resize(nt);
    coeffs.resize(nt);
    for (unsigned k = 0; k < nt; k++) {
      std::string c, fptr;
      unsigned reserved, nf;
      std::cin >> c >> reserved >> nf >> fptr;
      if (c != "-") {
        uint32_t w[8];
        parse(c, w);
        coeffs[k].resize(32);
        memcpy(coeffs[k].data(), w, 32);   // (little-endian host: the 32 bytes of the header)
      }
      if (fptr == "ok") {
        factors[k].resize(nf);
        for (unsigned f = 0; f < nf; f++) {
          long long col, rot;
          std::cin >> col >> rot;
          factors[k][f] = {(uint32_t)col, (int32_t)rot};
        }
      }
      terms[k].coeff = coeffs[k].empty() ? nullptr : coeffs[k].data();
      terms[k].factors = fptr == "ok" && nf ? factors[k].data() : nullptr;
      if (fptr == "ok" && nf == 0) terms[k].factors = nullptr;
      terms[k].n_factors = nf;
      terms[k].reserved = reserved;
    }
    e.columns = cols == "ok" ? columns.data() : nullptr;
    e.terms = trms == "ok" ? terms.data() : nullptr;
    e.n_columns = nc, e.n_terms = nt, e.n = n, e.flags = flags;
  }
};

template <class Fr> static void compile() {
  Desc d;
  d.read();
  ExprProgram P;
  uint8_t named[EXPR_MAX_COLUMNS];
  int st = expr_compile(d.e, &P, named);
  if (st) {
    printf("%d -\n", st);
    return;
  }
  const int st2 = expr_coeffs<Fr>(d.e, &P);
  printf("%d %d", st, st2);
  if (st2) {
    printf("\n");
    return;
  }
  printf(" %u %u", P.n_ops, P.rotated);
  for (uint32_t o = 0; o < P.n_ops; o++) printf(" %u:%u", P.op[o].column, P.op[o].rot);
  for (uint32_t k = 0; k < P.n_terms; k++) {
    printf(" ");
    if (!P.n_factors[k]) printf("-");
    for (uint32_t f = 0; f < P.n_factors[k]; f++) printf("%s%u", f ? "," : "", (unsigned)((P.ops[k] >> (8 * f)) & 0xff));
  }
  for (uint32_t c = 0; c < d.e.n_columns; c++) printf(" %u", named[c]);
  for (uint32_t k = 0; k < P.n_terms; k++) {
    printf(" ");
    print(P.coeff[k], "");
  }
  printf("\n");
}

template <class Fr> static void eval() {
  int slots;
  std::cin >> slots;
  Desc d;
  d.read();
  const uint64_t n = d.e.n;
  std::vector<std::vector<uint32_t>> cols(d.e.n_columns, std::vector<uint32_t>(n * 8));
  for (auto& c : cols)
    for (uint64_t i = 0; i < n; i++) {
      std::string s;
      std::cin >> s;
      parse(s, c.data() + i * 8);
    }
  ExprProgram P;
  uint8_t named[EXPR_MAX_COLUMNS];
  int st = expr_compile(d.e, &P, named);
  if (!st) st = expr_coeffs<Fr>(d.e, &P);
  if (st || (slots && P.n_ops > (uint32_t)slots)) {
    printf("status %d\n", st ? st : -1);
    return;
  }
  for (uint32_t o = 0; o < P.n_ops; o++) P.op[o].base = cols[P.op[o].column].data();
  auto load = [](uint32_t* v, const uint32_t* base, uint32_t at) {
    memcpy(v, base + (size_t)at * 8, 32);
    return words_geq<8>(v, Fr::Q);
  };
  bool bad = false;
  for (uint64_t i = 0; i < n; i++) {
    uint32_t acc[8];
    switch (slots) {
      case 0: bad |= fr_expr_entry<Fr>(acc, P, (uint32_t)i, load); break;
      case 2: bad |= fr_expr_entry_slots<Fr, 2>(acc, P, (uint32_t)i, load); break;
      case 4: bad |= fr_expr_entry_slots<Fr, 4>(acc, P, (uint32_t)i, load); break;
      default: bad |= fr_expr_entry_slots<Fr, 8>(acc, P, (uint32_t)i, load); break;
    }
    print(acc, " ");
  }
  printf("%d\n", bad ? 1 : 0);
}

template <class Fr> static void dispatch(const std::string& op) {
  if (op == "compile") compile<Fr>();
  else if (op == "eval") eval<Fr>();
  else printf("?\n");
}

int main() {
  std::string curve, op;
  while (std::cin >> curve) {
    if (curve == "geometry") {
      printf("%d %d %d %zu\n", EXPR_THREADS, EXPR_REGISTER_SLOTS, EXPR_SLOTS_MAX, sizeof(ExprProgram));
      continue;
    }
    if (curve == "index") {
      unsigned long long i, n;
      long long rot;
      std::cin >> i >> rot >> n;
      printf("%u\n", expr_index((uint32_t)i, expr_reduce_rot((int32_t)rot, n), (uint32_t)n));
      continue;
    }
    if (curve == "overlap") {
      unsigned named;
      unsigned long long first, first_out, n;
      std::cin >> named >> first >> first_out >> n;
      printf("%d\n", expr_overlap_ok((uint8_t)named, first, first_out, n) ? 1 : 0);
      continue;
    }
    std::cin >> op;
    if (curve == "bls12-377") dispatch<Bls377Fr>(op);
    else if (curve == "pallas") dispatch<PallasFr>(op);
    else if (curve == "bls12-381") dispatch<Bls381Fr>(op);
    else if (curve == "ed-on-bls12-377") dispatch<Ed377Fr>(op);
    else printf("?\n");
  }
  return 0;
}

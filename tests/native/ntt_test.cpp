// Host-side driver for the number-theoretic transform: the planner (msm_zprize_amd/csrc/ntt_plan.h), the roots of unity
// and the per-thread bodies of ntt_kernels.h (load, radix-4 / radix-2 steps, store, the two-level powers), compiled for
// the CPU from the same templates and chained exactly as k_ntt_pass and NttOps::scalars_ntt (ntt_ops.h) chain them: one tile
// memory of NTT_LDS_WORDS words per plane, NTT_THREADS virtual threads per phase, one pass after the other through
// scratch.  Driven by tests/test_ntt_cpu.py through stdin/stdout, one request per line, values as hex:
//   geometry                      ->  NTT_PASS_LOG NTT_RUN_LOG NTT_THREADS NTT_LDS_WORDS NTT_MAX_PASSES   (decimal)
//   plan <log_n>                  ->  n_passes tile_log split, then s log_c log_t s_next first last per pass  (decimal)
//   <curve> consts                ->  TWO_ADICITY ROOT_MAX
//   <curve> root <log_n>          ->  the default root, or "unsupported"
//   <curve> primitive <log_n> <w> ->  1 / 0
//   <curve> tw <log_n> <count> <e ...>
//                                 ->  w^e through the two-level tables of the plan, default root
//   clash <a> <na> <b> <nb>       ->  ranges_clash (csrc/ranges.h): 1 / 0   (decimal)
//   lds <s> <log_c> <log_t>       ->  the LDS slots of one pass of that shape, as the thread bodies touch them: one group per
//                                     LDS instruction (the k-th access of every thread in a phase), groups separated by
//                                     "|", NTT_THREADS decimal slots each, -1 for a thread that makes no such access
//   <curve> ntt <log_n> <flags> <count> <n_in> <shift> <count * n_in values>
//                                 ->  count * n outputs (flags: 1 inverse, 2 coset; shift ignored without coset), or "range"
// No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/fr.h"
#include "../../msm_zprize_amd/csrc/ntt_kernels.h"
#include "../../msm_zprize_amd/csrc/ranges.h"
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

// the tile memory of one workgroup, bounds checked
struct HostLds {
  std::vector<uint32_t> w = std::vector<uint32_t>((size_t)8 * NTT_LDS_WORDS, 0xdeadbeefu);
  void load(uint32_t slot, uint32_t* x) const {
    if (slot >= (uint32_t)NTT_LDS_WORDS) { fprintf(stderr, "LDS slot %u\n", slot); exit(2); }
    for (int j = 0; j < 8; j++) x[j] = w[(size_t)j * NTT_LDS_WORDS + slot];
  }
  void store(uint32_t slot, const uint32_t* x) {
    if (slot >= (uint32_t)NTT_LDS_WORDS) { fprintf(stderr, "LDS slot %u\n", slot); exit(2); }
    for (int j = 0; j < 8; j++) w[(size_t)j * NTT_LDS_WORDS + slot] = x[j];
  }
};

// a tile memory that notes which slot each access touches
struct RecordLds {
  std::vector<int> slots;
  void load(uint32_t slot, uint32_t* x) { slots.push_back((int)slot); for (int j = 0; j < 8; j++) x[j] = 0; }
  void store(uint32_t slot, const uint32_t*) { slots.push_back((int)slot); }
};

static void lds_trace() {
  using Fr = Bls377Fr;
  uint32_t s, log_c, log_t;
  std::cin >> s >> log_c >> log_t;
  NttArgs A{};
  A.pass.s = s, A.pass.log_c = log_c, A.pass.log_t = log_t, A.pass.log_n = s + log_c + log_t, A.pass.last = 1;
  const uint64_t n = 1ull << A.pass.log_n;
  std::vector<uint32_t> in(n * 8, 0), out(n * 8, 0), tw((1u << s) * 8 + 8, 0);
  A.in = in.data(), A.out = out.data(), A.tile_tw = tw.data(), A.tile_log = s, A.count = 1;
  bool first = true;
  auto phase = [&](auto body) {
    std::vector<std::vector<int>> per(NTT_THREADS);
    size_t most = 0;
    for (uint32_t u = 0; u < (uint32_t)NTT_THREADS; u++) {
      RecordLds lds;
      body(lds, u);
      per[u] = lds.slots;
      if (per[u].size() > most) most = per[u].size();
    }
    for (size_t k = 0; k < most; k++) {
      printf("%s", first ? "" : " |");
      first = false;
      for (uint32_t u = 0; u < (uint32_t)NTT_THREADS; u++) printf(" %d", k < per[u].size() ? per[u][k] : -1);
    }
  };
  phase([&](RecordLds& l, uint32_t u) { ntt_thread_load<Fr>(l, A, A.in, 0, u); });
  uint32_t rem = s;
  for (; rem >= 2; rem -= 2) phase([&](RecordLds& l, uint32_t u) { ntt_thread_step<Fr>(l, A, rem - 2, true, u); });
  if (rem) phase([&](RecordLds& l, uint32_t u) { ntt_thread_step<Fr>(l, A, 0, false, u); });
  phase([&](RecordLds& l, uint32_t u) { ntt_thread_store<Fr>(l, A, out.data(), 0, u); });
  printf("\n");
}

// a table as k_scalars_powers fills it: runs of SPOW_RUN entries, one fr_pow_run each
template <class Fr> static void fill_table(uint32_t* out, const NttTableSpec& s) {
  FrPowTable t;
  fr_pow_table<Fr>(t, s.ratio);
  for (uint64_t first = 0; first < s.count; first += SPOW_RUN) {
    const uint64_t left = s.count - first;
    fr_pow_run<Fr>(out + first * 8, s.base, t, (uint32_t)first, left < SPOW_RUN ? (uint32_t)left : (uint32_t)SPOW_RUN);
  }
}

template <class Fr> static std::vector<uint32_t> twiddle_tables(const NttPlan& p, const uint32_t* w) {
  // 16-byte aligned records: a vector of uint32_t from operator new is
  std::vector<uint32_t> t(ntt_twiddle_entries(p) * 8);
  NttTableSpec spec[3];
  ntt_twiddle_specs<Fr>(p, w, spec);
  uint32_t* at = t.data();
  for (int k = 0; k < 3; k++) {
    fill_table<Fr>(at, spec[k]);
    at += spec[k].count * 8;
  }
  return t;
}

// one launch of k_ntt_pass: every (tile, vector) workgroup, phase by phase
template <class Fr> static bool run_pass(const NttArgs& A) {
  bool bad = false;
  for (uint32_t tile = 0; tile < ntt_pass_tiles(A.pass); tile++) {
    HostLds lds;
    for (uint32_t v = 0; v < A.count; v++) {
      const uint32_t* in = A.in + (uint64_t)v * A.in_stride * 8;
      uint32_t* out = A.out + (uint64_t)v * A.out_stride * 8;
      for (uint32_t u = 0; u < (uint32_t)NTT_THREADS; u++) bad |= ntt_thread_load<Fr>(lds, A, in, tile, u);
      uint32_t rem = A.pass.s;
      for (; rem >= 2; rem -= 2)
        for (uint32_t u = 0; u < (uint32_t)NTT_THREADS; u++) ntt_thread_step<Fr>(lds, A, rem - 2, true, u);
      if (rem)
        for (uint32_t u = 0; u < (uint32_t)NTT_THREADS; u++) ntt_thread_step<Fr>(lds, A, 0, false, u);
      for (uint32_t u = 0; u < (uint32_t)NTT_THREADS; u++) ntt_thread_store<Fr>(lds, A, out, tile, u);
    }
  }
  return bad;
}

template <class Fr> static void transform() {
  uint32_t log_n, flags, count;
  uint64_t n_in;
  uint32_t shift[8];
  std::cin >> log_n >> flags >> count >> n_in;
  read_value(shift);
  const bool inverse = flags & 1, coset = flags & 2;
  const uint64_t n = 1ull << log_n;
  std::vector<uint32_t> x(count * n_in * 8);
  for (uint64_t i = 0; i < count * n_in; i++) read_value(x.data() + i * 8);
  if (log_n > (uint32_t)Fr::TWO_ADICITY) { printf("unsupported\n"); return; }
  const NttPlan plan = ntt_plan(log_n);
  uint32_t w[8];
  fr_root_of_unity<Fr>(w, log_n);
  if (inverse) fr_inv<Fr>(w, w);
  const std::vector<uint32_t> tw = twiddle_tables<Fr>(plan, w);
  NttCall call{};
  call.plan = plan;
  call.twiddles = tw.data();
  call.inverse = inverse;
  call.n_in = n_in;
  call.count = count;
  uint32_t nn[8] = {}, ninv[8];
  nn[log_n >> 5] = 1u << (log_n & 31);
  fr_inv<Fr>(ninv, nn);
  fr_to_mont<Fr>(call.ninv.w, ninv);
  std::vector<uint32_t> cos;
  if (coset) {
    NttTableSpec lo, hi;
    uint32_t g[8];
    for (int j = 0; j < 8; j++) g[j] = shift[j];
    if (inverse) fr_inv<Fr>(g, g);
    ntt_two_level_specs<Fr>(plan, g, inverse ? call.ninv.w : Fr::ONE, &lo, &hi);
    cos.resize((lo.count + hi.count) * 8);
    fill_table<Fr>(cos.data(), lo);
    fill_table<Fr>(cos.data() + lo.count * 8, hi);
    call.coset = cos.data();
  }
  uint32_t err = 0;
  call.err = &err;
  // in -> scratch 0 -> scratch 1 -> scratch 0 -> ... -> out, as the engine does
  std::vector<uint32_t> out(count * n * 8, 0xa5a5a5a5u), s0(plan.n_passes > 1 ? count * n * 8 : 0, 0x5a5a5a5au),
      s1(plan.n_passes > 2 ? count * n * 8 : 0, 0x5a5a5a5au);
  const uint32_t* src = x.data();
  uint64_t stride = n_in;
  bool bad = false;
  for (uint32_t j = 0; j < plan.n_passes; j++) {
    uint32_t* dst = j + 1 == plan.n_passes ? out.data() : (j & 1) ? s1.data() : s0.data();
    bad |= run_pass<Fr>(ntt_pass_args(call, j, src, stride, dst));
    src = dst;
    stride = n;
  }
  if (bad) { printf("range\n"); return; }
  for (uint64_t i = 0; i < count * n; i++) print(out.data() + i * 8, i + 1 == count * n ? "\n" : " ");
}

template <class Fr> static void run(const std::string& op) {
  const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  if (op == "consts") {
    printf("%x ", Fr::TWO_ADICITY);
    print(Fr::ROOT_MAX, "\n");
  } else if (op == "root") {
    uint32_t log_n, w[8];
    std::cin >> log_n;
    if (log_n > (uint32_t)Fr::TWO_ADICITY) { printf("unsupported\n"); return; }
    fr_root_of_unity<Fr>(w, log_n);
    print(w, "\n");
  } else if (op == "primitive") {
    uint32_t log_n, w[8];
    std::cin >> log_n;
    read_value(w);
    printf("%d\n", fr_is_primitive_root<Fr>(w, log_n) ? 1 : 0);
  } else if (op == "tw") {
    uint32_t log_n, count, w[8];
    std::cin >> log_n >> count;
    const NttPlan plan = ntt_plan(log_n);
    fr_root_of_unity<Fr>(w, log_n);
    const std::vector<uint32_t> tw = twiddle_tables<Fr>(plan, w);
    NttCall call{};
    call.plan = plan;
    call.twiddles = tw.data();
    const NttArgs a = ntt_pass_args(call, 0, nullptr, 0, nullptr);
    for (uint32_t i = 0; i < count; i++) {
      unsigned long long e;
      std::cin >> std::hex >> e >> std::dec;
      uint32_t x[8];
      for (int j = 0; j < 8; j++) x[j] = one[j];
      ntt_mul_power<Fr>(x, a.tw, e);
      print(x, i + 1 == count ? "\n" : " ");
    }
  } else if (op == "ntt") {
    transform<Fr>();
  } else {
    printf("bad op\n");
  }
}

int main() {
  std::string curve, op;
  while (std::cin >> curve) {
    if (curve == "geometry") {
      printf("%d %d %d %d %d\n", NTT_PASS_LOG, NTT_RUN_LOG, NTT_THREADS, NTT_LDS_WORDS, NTT_MAX_PASSES);
      continue;
    }
    if (curve == "clash") {
      unsigned long long a, na, b, nb;
      std::cin >> a >> na >> b >> nb;
      printf("%d\n", ranges_clash(a, na, b, nb) ? 1 : 0);
      continue;
    }
    if (curve == "lds") {
      lds_trace();
      continue;
    }
    if (curve == "plan") {
      uint32_t log_n;
      std::cin >> log_n;
      const NttPlan p = ntt_plan(log_n);
      printf("%u %u %u", p.n_passes, p.tile_log, p.split);
      for (uint32_t j = 0; j < p.n_passes; j++) {
        const NttPass& s = p.pass[j];
        printf(" %u %u %u %u %u %u", s.s, s.log_c, s.log_t, s.s_next, s.first, s.last);
      }
      printf("\n");
      continue;
    }
    std::cin >> op;
    if (curve == "bls12-377") run<Bls377Fr>(op);
    else if (curve == "pallas") run<PallasFr>(op);
    else if (curve == "bls12-381") run<Bls381Fr>(op);
    else if (curve == "ed-on-bls12-377") run<Ed377Fr>(op);
    else printf("bad curve\n");
  }
  return 0;
}

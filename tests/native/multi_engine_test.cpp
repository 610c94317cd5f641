// The multi-device context (msm_zprize_amd/csrc/multi.h, MultiEngine) over G mock engines on a toy group, G = 1, 2, 3,
// 5, 7 and 8, without a GPU: the block split, the per-engine threads, the host folds and the error paths, every result
// compared with a FLAT MODEL -- the same operation computed in this file on the caller's unsplit arrays.
//
// Toy data.  MultiEngine(curve, fe_bytes = 4, ...): a point record is 8 bytes, one uint64_t, and the group is Z/2^64 under
// addition (msmz_point_add below).  A scalar is a 32-byte record whose value is below 2^32, so every sum of fewer than
// 2^21 products stays far below q: the host's fr_add is integer addition and the model a 128-bit sum.
//
// The mock keeps its sets as vectors keyed by handle and refuses what a real engine refuses (unknown handle, wrong kind,
// a range beyond the LOCAL set: MSMZ_ERR_ARG), so a local range that MultiEngine gets wrong comes back as a status.  The
// handles of engine g start at 1000 (g + 1): a handle sent to the wrong engine is unknown there.  Nothing here uses the
// index arithmetic of multi.h; the one place the mock speaks about the split is for_runs ("local block b of shard g is
// set block b G + g"), and the model's owner() says which engine holds entry i by division.
//
// stdout: failures (operation, G, n, range), then "cases N".  Exit status 1 on any failure.  The same source is built
// plain, with -fsanitize=thread and with -fsanitize=address,undefined (tests/test_multi_engine_cpu.py).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>

#include "../../msm_zprize_amd/csrc/multi.h"

using namespace msmz;

// ---------------------------------------------------------------------------------------------- the toy group
static uint64_t load64(const uint8_t* p) {
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
}
static uint32_t load32(const uint8_t* p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
}
// the same on 4- and 8-byte aligned addresses inside the big arrays (the sanitizers see one plain access, not a call)
#define MSMZ_TEST_INLINE inline __attribute__((always_inline))
// The flat model and the comparisons run on the caller's thread over the caller's own arrays, which no worker writes:
// they are kept out of the thread sanitizer's instrumentation, which would only slow them.  Everything that touches a
// mock or the context (the mocks, multi.h, the methods of Ctx) is instrumented.
#define MSMZ_TEST_MODEL __attribute__((no_sanitize("thread")))
typedef uint32_t __attribute__((may_alias)) word32;
typedef uint64_t __attribute__((may_alias)) word64;
static MSMZ_TEST_INLINE uint32_t ld32(const uint8_t* p) { return *reinterpret_cast<const word32*>(p); }
static MSMZ_TEST_INLINE uint64_t ld64(const uint8_t* p) { return *reinterpret_cast<const word64*>(p); }
static MSMZ_TEST_INLINE void st32(uint8_t* p, uint32_t v) { *reinterpret_cast<word32*>(p) = v; }
static MSMZ_TEST_INLINE void st64(uint8_t* p, uint64_t v) { *reinterpret_cast<word64*>(p) = v; }
static const uint64_t POISON = 0xDEADBEEFDEADBEEFull;   // the bytes of a record flagged infinite: never to be added

// Z/2^64: the flags decide, the bytes of an operand flagged infinite are not read; infinity <=> sum 0
extern "C" int msmz_point_add(int, const uint8_t* a, int a_inf, const uint8_t* b, int b_inf, uint8_t* out, int* out_inf) {
  const uint64_t sum = (a_inf ? 0 : load64(a)) + (b_inf ? 0 : load64(b));
  const uint64_t rec = sum ? sum : POISON;
  memcpy(out, &rec, 8);
  *out_inf = sum == 0;
  return MSMZ_OK;
}

namespace {

constexpr uint64_t BLK = 65536;

MSMZ_TEST_INLINE uint64_t mix(uint64_t x) {   // splitmix64
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// The fixed toy functions, one statement each for the mock and the model (values, not indices).
// A point value keeps its top two bits for check_points: 1 = off the curve, 2 = off the subgroup, 0 = fine.
MSMZ_TEST_INLINE uint64_t gen_point(uint64_t seed, uint64_t i, uint8_t* inf) {
  const uint64_t h = mix(seed * 0x100000001B3ull + i);
  *inf = h % 97 == 0;
  uint64_t v = (h >> 2) | 1;
  if (h % 4099 == 5) v |= 1ull << 62;
  if (h % 4099 == 6) v |= 2ull << 62;
  return v;
}
MSMZ_TEST_INLINE uint32_t gen_scalar(uint64_t seed, uint64_t i) {
  const uint64_t h = mix(~seed * 0x100000001B3ull + i);
  return h % 1013 == 3 ? 0 : (uint32_t)(h >> 16);
}
MSMZ_TEST_INLINE uint32_t pow_entry(uint32_t base, uint32_t ratio, uint64_t i) { return base + ratio * (uint32_t)i; }
MSMZ_TEST_INLINE uint32_t toy_inverse(uint32_t x) { return x ? (x * 2654435761u) | 1u : 0; }
MSMZ_TEST_INLINE uint64_t expand32(uint32_t c, bool parity) { return ((((uint64_t)c * 0x9E3779B97F4A7C15ull) >> 2) | 1) + (parity ? 2 : 0); }
MSMZ_TEST_INLINE uint32_t compress64(uint64_t v, bool parity) { return (uint32_t)(v ^ (v >> 32)) + (parity ? 0x51EDu : 0u); }
MSMZ_TEST_INLINE int verdict_of(uint64_t v, uint8_t inf, uint32_t what) {
  if (inf) return 0;
  const int t = (int)(v >> 62);
  return t == 1 ? 1 : (t == 2 && (what & MSMZ_CHECK_SUBGROUP)) ? 2 : 0;
}
MSMZ_TEST_INLINE uint64_t mul_value(uint32_t s, uint64_t p, uint8_t p_inf, bool has_q, uint64_t q, uint8_t q_inf, const msmz_mul_opts& o) {
  return (p_inf ? 0 : s * p) + (has_q && !q_inf ? q : 0) + (uint64_t)o.scalar_bits * (o.flags + 1);
}
msmz_log toy_log(uint32_t id, uint64_t cnt, uint32_t batch, const msmz_opts* o) {
  msmz_log l{};
  for (int i = 0; i < MSMZ_N_STAGES; i++) l.stage_ms[i] = (float)((id * 5 + 3 + i) % 7) + 0.25f * (float)i;
  for (int i = 0; i < 32; i++) l.batch_add_ms[i] = (float)((id * 3 + i) % 5);
  l.scatter_kernel_ms = (float)((id * 4 + 1) % 9);
  l.c = 10 + (int)id + (o ? o->c : 0);
  l.K = 20 + (int)id;
  l.glv = (int)(id & 1);
  l.rounds = (int)((id * 2) % 3) + 1;
  l.max_bucket = (id * 3) % 5 + 1;
  l.n_entries = cnt * batch;
  l.n_pairs = 1000 + id;
  l.scatter_launches = id + 2;
  return l;
}

// ---------------------------------------------------------------------------------------------- what the mocks share
struct Barrier {
  std::mutex mu;
  std::condition_variable cv;
  uint32_t expected = 0, arrived = 0;
  bool broken = false;
  void arm(uint32_t e) {
    std::lock_guard<std::mutex> lk(mu);
    expected = e, arrived = 0, broken = false;
  }
  // every engine with a share has entered, or 10 s have passed (a hang guard: a mock call takes microseconds)
  void arrive() {
    std::unique_lock<std::mutex> lk(mu);
    if (!expected) return;
    arrived++;
    cv.notify_all();
    const auto until = std::chrono::system_clock::now() + std::chrono::seconds(10);
    if (!cv.wait_until(lk, until, [this] { return arrived >= expected || broken; })) {
      broken = true;
      cv.notify_all();
    }
  }
  bool met() {
    std::lock_guard<std::mutex> lk(mu);
    return !broken && arrived == expected;
  }
};

struct Shared {
  std::atomic<int> destroyed{0};
  std::atomic<int> thread_violations{0};
  std::atomic<int> forbidden{0};   // calls MultiEngine refuses itself and must never forward
  Barrier barrier;
};

struct MockSet {
  int kind = 0;
  uint64_t n = 0;
  std::vector<uint8_t> rec, inf;   // points: 8 n bytes + n flags
  std::vector<uint32_t> sc;        // scalars: the values (a record is the value and 28 zero bytes)
  bool pre = false;
  int c = 0, glv = 0, sbits = 0;
  uint32_t copies = 0;
  static MockSet make(int kind, uint64_t n) {
    MockSet s;
    s.kind = kind, s.n = n;
    if (kind) s.sc.assign(n, 0);
    else s.rec.assign(n * 8, 0), s.inf.assign(n, 0);
    return s;
  }
  uint64_t pv(uint64_t i) const { return ld64(&rec[i * 8]); }
  uint32_t sv(uint64_t i) const { return sc[i]; }
  void set_point(uint64_t i, uint64_t v) {   // a value of the group: 0 is infinity
    st64(&rec[i * 8], v ? v : POISON);
    inf[i] = v == 0;
  }
};

// f(local index, set index, length) over the n local records of a shard, or of an unsplit engine
template <class F>
void for_runs(uint64_t n, const GenMap* m, F f) {
  if (!m) return f((uint64_t)0, (uint64_t)0, n);
  const uint64_t blk = 1ull << m->blk_shift;
  for (uint64_t b = 0; b * blk < n; b++)
    f(b * blk, (b * m->nshards + m->shard) * blk, std::min(blk, n - b * blk));   // local block b = set block b G + g
}

class Mock : public IEngine {
 public:
  Mock(uint32_t id, Shared* sh) : id(id), sh_(sh), next_(1000ull * (id + 1) + 1) {}
  ~Mock() override { sh_->destroyed++; }

  // read and written by the test between calls of the context (the workers' hand-over orders them)
  const uint32_t id;
  mutable uint64_t calls = 0;
  uint64_t worker_calls = 0;
  int fail_next = 0;              // the status the next call that arrives on the worker returns, doing nothing
  std::thread::id tid;
  bool has_tid = false;
  int glv_bits = -1;
  uint64_t limits[2] = {0, 0};
  int hook_status = 0;
  size_t live() const { return sets_.size(); }

  int upload_points(const uint8_t* xy, const uint8_t* inf, uint64_t n, uint64_t* h, const GenMap* split) override {
    if (int st = worker()) return st;
    if (!xy || !h || !n) return MSMZ_ERR_ARG;
    MockSet s = MockSet::make(0, n);
    for_runs(n, split, [&](uint64_t li, uint64_t si, uint64_t len) {
      memcpy(&s.rec[li * 8], xy + si * 8, len * 8);
      if (inf) memcpy(&s.inf[li], inf + si, len);
    });
    return put(std::move(s), h);
  }
  int upload_scalars(const uint8_t* sc, uint64_t n, uint64_t* h, const GenMap* split) override {
    if (int st = worker()) return st;
    if (!sc || !h || !n) return MSMZ_ERR_ARG;
    MockSet s = MockSet::make(1, n);
    for_runs(n, split, [&](uint64_t li, uint64_t si, uint64_t len) {
      for (uint64_t k = 0; k < len; k++) s.sc[li + k] = ld32(sc + (si + k) * 32);
    });
    return put(std::move(s), h);
  }
  int import_points(const msmz_src& src, uint64_t n, uint64_t* h, const GenMap* split) override {
    if (int st = worker()) return st;
    uint32_t w;
    uint64_t stride;
    if (!h || !n || src_check(&src, 4, &w, &stride) || (src.flags & MSMZ_SRC_DEVICE)) return MSMZ_ERR_ARG;
    const bool parity = (src.flags & MSMZ_SRC_SIGN_PARITY) != 0;
    MockSet s = MockSet::make(0, n);
    for_runs(n, split, [&](uint64_t li, uint64_t si, uint64_t len) {
      for (uint64_t k = 0; k < len; k++) {
        const uint8_t* r = (const uint8_t*)src.ptr + (si + k) * stride;
        st64(&s.rec[(li + k) * 8], w == 4 ? expand32(ld32(r), parity) : ld32(r) | (uint64_t)ld32(r + 4) << 32);
        if (src.is_inf) s.inf[li + k] = src.is_inf[si + k];
      }
    });
    return put(std::move(s), h);
  }
  int import_scalars(const msmz_src& src, uint64_t n, uint64_t* h, const GenMap* split) override {
    if (int st = worker()) return st;
    uint32_t w;
    uint64_t stride;
    if (!h || !n || src_check(&src, 0, &w, &stride) || (src.flags & MSMZ_SRC_DEVICE)) return MSMZ_ERR_ARG;
    MockSet s = MockSet::make(1, n);
    for_runs(n, split, [&](uint64_t li, uint64_t si, uint64_t len) {
      for (uint64_t k = 0; k < len; k++) s.sc[li + k] = ld32((const uint8_t*)src.ptr + (si + k) * stride);   // (w >= 4)
    });
    return put(std::move(s), h);
  }
  int import_scalars_into(uint64_t, uint64_t, const msmz_src&, uint64_t) override { return forbidden(); }
  int gather_src(const msmz_src& s, int point_fe_bytes, uint64_t n, std::vector<uint8_t>* recs,
                 std::vector<uint8_t>* flags) override {
    calls++;
    uint32_t w;
    uint64_t stride;
    if (!recs || !flags || !n || src_check(&s, point_fe_bytes, &w, &stride)) return MSMZ_ERR_ARG;
    recs->resize(n * w);
    for (uint64_t i = 0; i < n; i++) memcpy(recs->data() + i * w, (const uint8_t*)s.ptr + i * stride, w);
    flags->clear();
    if (s.is_inf) flags->assign(s.is_inf, s.is_inf + n);
    return MSMZ_OK;
  }
  int random_points(uint64_t n, uint64_t seed, const GenMap& map, uint64_t* h) override {
    if (int st = worker()) return st;
    if (!h || !n) return MSMZ_ERR_ARG;
    MockSet s = MockSet::make(0, n);
    for_runs(n, &map, [&](uint64_t li, uint64_t si, uint64_t len) {
      for (uint64_t k = 0; k < len; k++) {
        st64(&s.rec[(li + k) * 8], gen_point(seed, si + k, &s.inf[li + k]));
      }
    });
    return put(std::move(s), h);
  }
  int random_scalars(uint64_t n, uint64_t seed, const GenMap& map, uint64_t* h) override {
    if (int st = worker()) return st;
    if (!h || !n) return MSMZ_ERR_ARG;
    MockSet s = MockSet::make(1, n);
    for_runs(n, &map, [&](uint64_t li, uint64_t si, uint64_t len) {
      for (uint64_t k = 0; k < len; k++) s.sc[li + k] = gen_scalar(seed, si + k);
    });
    return put(std::move(s), h);
  }
  int scalars_powers(const uint8_t* base, const uint8_t* ratio, uint64_t n, const GenMap& map, uint64_t* h) override {
    if (int st = worker()) return st;
    if (!h || !ratio || !n) return MSMZ_ERR_ARG;
    MockSet s = MockSet::make(1, n);
    for_runs(n, &map, [&](uint64_t li, uint64_t si, uint64_t len) {
      for (uint64_t k = 0; k < len; k++) s.sc[li + k] = pow_entry(base ? load32(base) : 1u, load32(ratio), si + k);
    });
    return put(std::move(s), h);
  }

  int download_points(uint64_t h, uint64_t first, uint64_t count, uint8_t* xy, uint8_t* inf) override {
    calls++;
    const MockSet* s = find(h, 0, first, count);
    if (!s || !xy) return MSMZ_ERR_ARG;
    memcpy(xy, &s->rec[first * 8], count * 8);
    if (inf) memcpy(inf, &s->inf[first], count);
    return MSMZ_OK;
  }
  int download_points_compressed(uint64_t h, uint64_t first, uint64_t count, uint8_t* out, uint8_t* inf,
                                 uint32_t flags) override {
    calls++;
    const MockSet* s = find(h, 0, first, count);
    if (!s || !out || (flags & ~(uint32_t)MSMZ_SRC_SIGN_PARITY)) return MSMZ_ERR_ARG;
    for (uint64_t i = 0; i < count; i++) {
      st32(out + i * 4, compress64(s->pv(first + i), flags != 0));
    }
    if (inf) memcpy(inf, &s->inf[first], count);
    return MSMZ_OK;
  }
  int download_scalars(uint64_t h, uint64_t first, uint64_t count, uint8_t* out) override {
    calls++;
    const MockSet* s = find(h, 1, first, count);
    if (!s || !out) return MSMZ_ERR_ARG;
    memset(out, 0, count * 32);
    for (uint64_t i = 0; i < count; i++) st32(out + i * 32, s->sc[first + i]);
    return MSMZ_OK;
  }
  int free_handle(uint64_t h) override {
    calls++;
    return sets_.erase(h) ? MSMZ_OK : MSMZ_ERR_ARG;
  }

  // sum s p over the share; a sum of 0 is infinity and its record bytes are poison
  int msm_batch(uint64_t ph, const uint8_t* host_scalars, uint64_t sh, uint64_t n, uint32_t batch, const msmz_opts* o,
                uint8_t* out, int* out_inf, msmz_log* log, const GenMap* split, uint64_t host_stride) override {
    if (int st = worker()) return st;
    sh_->barrier.arrive();
    const MockSet* P = find(ph, 0, 0, n);
    if (!P || !out || !out_inf || !n || !batch) return MSMZ_ERR_ARG;
    const MockSet* S = nullptr;
    if (!host_scalars && (!(S = find(sh, 1, 0, 0)) || S->n / batch < n)) return MSMZ_ERR_ARG;
    const uint64_t stride = host_stride ? host_stride : n;
    for (uint32_t k = 0; k < batch; k++) {
      uint64_t sum = 0;
      if (S) {
        for (uint64_t i = 0; i < n; i++) sum += P->inf[i] ? 0 : S->sv(k * n + i) * P->pv(i);
      } else {
        for_runs(n, split, [&](uint64_t li, uint64_t si, uint64_t len) {
          for (uint64_t j = 0; j < len; j++)
            sum += P->inf[li + j] ? 0 : ld32(host_scalars + (k * stride + si + j) * 32) * P->pv(li + j);
        });
      }
      const uint64_t rec = sum ? sum : POISON;
      memcpy(out + (size_t)k * 8, &rec, 8);
      out_inf[k] = sum == 0;
    }
    if (log) *log = toy_log(id, n, batch, o);
    return MSMZ_OK;
  }
  int msm_segments(uint64_t, uint64_t, const msmz_segment*, uint32_t, const msmz_opts*, uint8_t*, int*, msmz_log*) override {
    return forbidden();
  }

  int precompute_params(uint64_t n, const msmz_opts* o, uint32_t factor, int* c, int* glv, uint32_t* copies, int* K,
                        int* sbits) const override {
    calls++;
    *c = 7 + (int)(n % 5), *glv = o ? o->glv : 1, *copies = factor ? factor : 3, *K = 11 + (int)id;
    *sbits = o ? o->reserved[1] : 0;
    return MSMZ_OK;
  }
  int precompute_points(uint64_t ph, uint64_t n, int c, int glv, uint32_t copies, int sbits, uint64_t* h) override {
    if (int st = worker()) return st;
    const MockSet* P = find(ph, 0, 0, n);
    if (!h || !P || P->pre || !n) return MSMZ_ERR_ARG;
    MockSet s = MockSet::make(0, n);
    memcpy(s.rec.data(), P->rec.data(), n * 8);
    memcpy(s.inf.data(), P->inf.data(), n);
    s.pre = true, s.c = c, s.glv = glv, s.copies = copies, s.sbits = sbits;
    return put(std::move(s), h);
  }
  int precomputed_info(uint64_t h, int32_t* c, int32_t* glv, uint32_t* factor, uint32_t* K, uint64_t* records,
                       int32_t* sbits) override {
    calls++;
    const MockSet* s = find(h, 0, 0, 0);
    if (!s || !s->pre) return MSMZ_ERR_ARG;
    if (c) *c = s->c;
    if (glv) *glv = s->glv;
    if (factor) *factor = s->copies;
    if (K) *K = 100 + id;
    if (records) *records = 0xBAD;   // (the engine's own share: the context answers for the whole set)
    if (sbits) *sbits = s->sbits;
    return MSMZ_OK;
  }

  int check_points(uint64_t h, uint64_t first, uint64_t count, uint32_t what, msmz_check_result* out,
                   uint8_t* verdicts) override {
    if (int st = worker()) return st;
    const MockSet* s = find(h, 0, 0, 0);
    if (!s || !out || !count || !what) return MSMZ_ERR_ARG;
    if (s->pre) return MSMZ_ERR_UNSUPPORTED;
    if (!in_range(first, count, s->n)) return MSMZ_ERR_ARG;
    *out = msmz_check_result{0, 0, UINT64_MAX};
    for (uint64_t i = 0; i < count; i++) {
      const int v = verdict_of(s->pv(first + i), s->inf[first + i], what);
      out->off_curve += v == 1, out->off_subgroup += v == 2;
      if (v && out->first_bad == UINT64_MAX) out->first_bad = first + i;   // absolute in the local set
      if (verdicts) verdicts[i] = (uint8_t)v;
    }
    return MSMZ_OK;
  }

  int points_mul(const msmz_mul& m, const msmz_mul_opts& o, uint64_t n, uint64_t* h) override {
    if (int st = worker()) return st;
    const MockSet* P = find(m.points_handle, 0, m.first_p, n);
    const MockSet* Q = m.addend_handle ? find(m.addend_handle, 0, m.first_q, n) : nullptr;
    const MockSet* S = m.scalars_handle ? find(m.scalars_handle, 1, m.first_s, n) : nullptr;
    if (!h || !n || !P || (m.addend_handle && !Q) || (m.scalars_handle ? !S : !m.scalar)) return MSMZ_ERR_ARG;
    if (P->pre || (Q && Q->pre)) return MSMZ_ERR_UNSUPPORTED;
    MockSet r = MockSet::make(0, n);
    for (uint64_t i = 0; i < n; i++)
      r.set_point(i, mul_value(S ? S->sv(m.first_s + i) : load32(m.scalar), P->pv(m.first_p + i), P->inf[m.first_p + i],
                               Q != nullptr, Q ? Q->pv(m.first_q + i) : 0, Q ? Q->inf[m.first_q + i] : 0, o));
    return put(std::move(r), h);
  }

  int scalars_combine(const msmz_scalar_term& x, const msmz_scalar_term* y, uint64_t n, uint64_t first_out,
                      uint64_t* out_handle) override {
    if (int st = worker()) return st;
    if (!out_handle || !n || (*out_handle == 0 && first_out)) return MSMZ_ERR_ARG;
    const msmz_scalar_term* in[2] = {&x, y};
    std::vector<uint32_t> acc(n, 0);
    for (int k = 0; k < 2; k++) {
      if (!in[k]) continue;
      const MockSet* v = find(in[k]->handle, 1, in[k]->first, n);
      const MockSet* c = in[k]->coeff_handle ? find(in[k]->coeff_handle, 1, in[k]->coeff_first, n) : nullptr;
      if (!v || (in[k]->coeff_handle && !c)) return MSMZ_ERR_ARG;
      const uint32_t bc = in[k]->coeff ? load32(in[k]->coeff) : 1u;
      for (uint64_t i = 0; i < n; i++) acc[i] += (c ? c->sv(in[k]->coeff_first + i) : bc) * v->sv(in[k]->first + i);
    }
    return write_scalars(acc, first_out, out_handle);
  }
  int scalars_dot(uint64_t xh, uint64_t first_x, uint64_t yh, uint64_t first_y, uint64_t n, uint8_t* out) override {
    if (int st = worker()) return st;
    const MockSet* X = find(xh, 1, first_x, n);
    const MockSet* Y = yh ? find(yh, 1, first_y, n) : nullptr;
    if (!out || !n || !X || (yh && !Y)) return MSMZ_ERR_ARG;
    unsigned __int128 sum = 0;
    for (uint64_t i = 0; i < n; i++) sum += (unsigned __int128)X->sv(first_x + i) * (Y ? Y->sv(first_y + i) : 1u);
    memset(out, 0, 32);
    memcpy(out, &sum, 16);
    return MSMZ_OK;
  }
  int scalars_recurrence(const msmz_scalar_rec&, uint64_t, uint64_t, uint64_t*, uint8_t*) override { return forbidden(); }
  int scalars_inverse(uint64_t h, uint64_t first, uint64_t n, uint64_t first_out, uint64_t* out_handle,
                      uint64_t* n_zero) override {
    if (int st = worker()) return st;
    const MockSet* X = find(h, 1, first, n);
    if (!out_handle || !n || !X || (*out_handle == 0 && first_out)) return MSMZ_ERR_ARG;
    std::vector<uint32_t> r(n);
    uint64_t zeros = 0;
    for (uint64_t i = 0; i < n; i++) {
      r[i] = toy_inverse(X->sv(first + i));
      zeros += X->sv(first + i) == 0;
    }
    if (int st = write_scalars(r, first_out, out_handle)) return st;
    if (n_zero) *n_zero = zeros;
    return MSMZ_OK;
  }
  int scalars_ntt(const msmz_ntt&, uint64_t, uint64_t*) override { return forbidden(); }

  int test_set_glv_bits(int bits) override {
    calls++;
    glv_bits = bits;
    return hook_status;
  }
  int test_retries() override { return (int)id + 1; }
  int test_set_limits(uint64_t a, uint64_t b) override {
    calls++;
    limits[0] = a, limits[1] = b;
    return hook_status;
  }
  void test_passes(uint64_t* range_passes, uint64_t* sub_batches) override {
    *range_passes = id + 1, *sub_batches = 2 * id + 1;
  }
  ITestHooks* test_hooks() override { return reinterpret_cast<ITestHooks*>(this); }

 private:
  // a call the context posts to this engine's thread: always the same thread, and the place errors are injected
  int worker() {
    calls++, worker_calls++;
    const std::thread::id me = std::this_thread::get_id();
    if (!has_tid) tid = me, has_tid = true;
    if (tid != me) sh_->thread_violations++;
    const int st = fail_next;
    fail_next = 0;
    return st;
  }
  int forbidden() {
    calls++;
    sh_->forbidden++;
    return MSMZ_ERR_HIP;
  }
  int put(MockSet&& s, uint64_t* h) {
    *h = next_++;
    sets_[*h] = std::move(s);
    return MSMZ_OK;
  }
  const MockSet* find(uint64_t h, int kind, uint64_t first, uint64_t n) const {
    auto it = sets_.find(h);
    return it == sets_.end() || it->second.kind != kind || !in_range(first, n, it->second.n) ? nullptr : &it->second;
  }
  int write_scalars(const std::vector<uint32_t>& v, uint64_t first_out, uint64_t* out_handle) {
    if (*out_handle == 0) {
      MockSet s = MockSet::make(1, v.size());
      s.sc = v;
      return put(std::move(s), out_handle);
    }
    auto it = sets_.find(*out_handle);
    if (it == sets_.end() || it->second.kind != 1 || !in_range(first_out, v.size(), it->second.n)) return MSMZ_ERR_ARG;
    std::copy(v.begin(), v.end(), it->second.sc.begin() + (ptrdiff_t)first_out);
    return MSMZ_OK;
  }

  Shared* sh_;
  uint64_t next_;
  std::map<uint64_t, MockSet> sets_;
};

// ---------------------------------------------------------------------------------------------- reporting
long g_cases = 0;
int g_fails = 0;
char g_where[64] = "";

void report(const char* fmt, ...) {
  if (++g_fails > 25) return;
  printf("FAIL [%s] ", g_where);
  va_list ap;
  va_start(ap, fmt);
  vprintf(fmt, ap);
  va_end(ap);
  printf("\n");
  fflush(stdout);   // (a wrong index can end the run)
}
#define CASE(cond, ...)              \
  do {                               \
    g_cases++;                       \
    if (!(cond)) report(__VA_ARGS__); \
  } while (0)

struct Rng {
  uint64_t s;
  uint64_t next() { return s = mix(s + 0x1234567); }
  uint64_t below(uint64_t m) { return next() % m; }
};

// ---------------------------------------------------------------------------------------------- the flat model
struct Points {
  std::vector<uint8_t> rec, inf;
  explicit Points(uint64_t n = 0) : rec(n * 8, 0), inf(n, 0) {}
  uint64_t n() const { return inf.size(); }
  MSMZ_TEST_INLINE uint64_t val(uint64_t i) const { return ld64(&rec[i * 8]); }
  MSMZ_TEST_INLINE void set(uint64_t i, uint64_t v, uint8_t f) {
    st64(&rec[i * 8], v);
    inf[i] = f;
  }
  MSMZ_TEST_INLINE void set_group(uint64_t i, uint64_t v) { set(i, v ? v : POISON, v == 0); }
};
struct Scalars {   // the values of a scalar set; wire(): its 32-byte records, as a caller hands them over
  std::vector<uint32_t> v;
  explicit Scalars(uint64_t n = 0) : v(n, 0) {}
  uint64_t n() const { return v.size(); }
  MSMZ_TEST_INLINE uint32_t val(uint64_t i) const { return v[i]; }
  MSMZ_TEST_INLINE void set(uint64_t i, uint32_t x) { v[i] = x; }
  MSMZ_TEST_MODEL std::vector<uint8_t> wire() const {
    std::vector<uint8_t> rec(v.size() * 32, 0);
    for (size_t i = 0; i < v.size(); i++) st32(&rec[i * 32], v[i]);
    return rec;
  }
};
// count records at `rec` hold the values from `want` on, zero-extended
MSMZ_TEST_MODEL bool records_equal(const uint8_t* rec, const uint32_t* want, uint64_t count) {
  for (uint64_t i = 0; i < count; i++) {
    const uint8_t* r = rec + i * 32;
    if (ld32(r) != want[i] || ld32(r + 4) || ld64(r + 8) || ld64(r + 16) || ld64(r + 24)) return false;
  }
  return true;
}

typedef std::vector<std::pair<uint64_t, uint64_t>> Ranges;

// >= 200 seeded (first, count), half of them starting just before a block boundary, plus ranges that start or end exactly
// on one
MSMZ_TEST_MODEL Ranges make_ranges(uint64_t n, uint32_t G, Rng& r) {
  Ranges v;
  for (int k = 0; k < 200; k++) {
    const uint64_t kind = r.below(100), maxc = kind < 96 ? 300 : 70000;
    uint64_t first = r.below(n);
    if (n > BLK && r.below(2)) {
      const uint64_t B = (1 + r.below(n / BLK)) * BLK;
      first = B - r.below(200);
    }
    if (first >= n) first = n - 1;
    v.push_back({first, 1 + r.below(std::min(maxc, n - first))});
  }
  std::set<uint64_t> bounds;
  for (uint64_t k : {(uint64_t)1, (uint64_t)2, (uint64_t)G, (uint64_t)G + 1, (uint64_t)2 * G, n / BLK})
    if (k && k * BLK <= n) bounds.insert(k * BLK);
  for (uint64_t B : bounds) {
    if (B < n) v.push_back({B, std::min<uint64_t>(n - B, 5)}), v.push_back({B - 3, std::min<uint64_t>(n - B + 3, 6)});
    v.push_back({B - 3, 3});
    v.push_back({B - BLK, BLK});
    if (B == *bounds.begin()) v.push_back({0, B});
    if (B == *bounds.rbegin() && B < n) v.push_back({B, n - B});
  }
  v.push_back({0, n});
  v.push_back({n - 1, 1});
  v.push_back({0, 1});
  return v;
}

MSMZ_TEST_MODEL void model_msm(const Points& P, const uint32_t* s, uint64_t n, uint64_t* val, int* inf) {
  uint64_t sum = 0;
  for (uint64_t i = 0; i < n; i++) sum += P.inf[i] ? 0 : s[i] * P.val(i);
  *val = sum, *inf = sum == 0;
}
bool same_point(const uint8_t* got, int got_inf, uint64_t want, int want_inf) {
  return got_inf == want_inf && (want_inf || load64(got) == want);   // (the bytes of infinity are nobody's)
}

// ---------------------------------------------------------------------------------------------- one context
struct Ctx {
  uint32_t G;
  Shared sh;
  std::vector<Mock*> mocks;   // owned by `me`
  std::vector<uint8_t> buf, flags;   // where downloads land
  MultiEngine* me = nullptr;

  explicit Ctx(uint32_t G) : G(G) {
    std::vector<IEngine*> e;
    for (uint32_t g = 0; g < G; g++) mocks.push_back(new Mock(g, &sh)), e.push_back(mocks.back());
    me = new MultiEngine((int)(G % 4), 4, e);   // (every curve id gets a turn: only scalars_dot reads it)
  }
  uint32_t owner(uint64_t i) const { return (uint32_t)((i / BLK) % G); }   // the engine that holds set entry i
  // engines that hold any of the first n entries, in device order
  std::vector<uint32_t> used(uint64_t n) const {
    std::vector<uint32_t> u;
    for (uint32_t g = 0; g < G; g++)
      if (g * BLK < n) u.push_back(g);
    return u;
  }
  std::vector<uint64_t> calls() const {
    std::vector<uint64_t> c;
    for (Mock* m : mocks) c.push_back(m->calls);
    return c;
  }
  std::vector<size_t> live() const {
    std::vector<size_t> c;
    for (Mock* m : mocks) c.push_back(m->live());
    return c;
  }
  void inject(uint32_t g, int status) { mocks[g]->fail_next = status; }
  // were all injected statuses taken?  (one left over means its engine was not called; it is cleared)
  bool injections_consumed() {
    bool consumed = true;
    for (Mock* m : mocks) consumed = consumed && m->fail_next == 0, m->fail_next = 0;
    return consumed;
  }
  bool live_is(const std::vector<size_t>& base, size_t extra) const {
    bool same = true;
    for (uint32_t g = 0; g < G; g++) same = same && mocks[g]->live() == base[g] + extra;
    return same;
  }
  uint64_t total_calls() const {
    uint64_t t = 0;
    for (Mock* m : mocks) t += m->calls;
    return t;
  }
};

// download every point set / scalar set over the ranges and compare with the flat arrays
MSMZ_TEST_MODEL void check_point_set(Ctx& c, const char* what, uint64_t h, const Points& flat, const Ranges& ranges) {
  int k = 0;
  for (auto [first, count] : ranges) {
    c.buf.assign(count * 8, 0xCC), c.flags.assign(count, 0xCC);
    const bool with_inf = k++ % 3 != 2;
    const int st = c.me->download_points(h, first, count, c.buf.data(), with_inf ? c.flags.data() : nullptr);
    CASE(st == MSMZ_OK && !memcmp(c.buf.data(), &flat.rec[first * 8], count * 8) &&
             (!with_inf || !memcmp(c.flags.data(), &flat.inf[first], count)),
         "download_points of %s: status %d, range (%llu, %llu)", what, st, (unsigned long long)first, (unsigned long long)count);
  }
}
MSMZ_TEST_MODEL void check_scalar_set(Ctx& c, const char* what, uint64_t h, const Scalars& flat, const Ranges& ranges) {
  for (auto [first, count] : ranges) {
    c.buf.assign(count * 32, 0xCC);
    const int st = c.me->download_scalars(h, first, count, c.buf.data());
    CASE(st == MSMZ_OK && records_equal(c.buf.data(), &flat.v[first], count),
         "download_scalars of %s: status %d, range (%llu, %llu)", what, st, (unsigned long long)first, (unsigned long long)count);
  }
}
MSMZ_TEST_MODEL bool whole_points_equal(Ctx& c, uint64_t h, const Points& flat) {
  c.buf.assign(flat.n() * 8, 0xCC), c.flags.assign(flat.n(), 0xCC);
  return c.me->download_points(h, 0, flat.n(), c.buf.data(), c.flags.data()) == MSMZ_OK && c.buf == flat.rec && c.flags == flat.inf;
}
MSMZ_TEST_MODEL bool whole_scalars_equal(Ctx& c, uint64_t h, const Scalars& flat) {
  c.buf.assign(flat.n() * 32, 0xCC);
  return c.me->download_scalars(h, 0, flat.n(), c.buf.data()) == MSMZ_OK && records_equal(c.buf.data(), flat.v.data(), flat.n());
}

// the merged log of a call over the first n entries: LogMerge::PARALLEL over the engines with a share
MSMZ_TEST_MODEL void check_parallel_log(Ctx& c, const char* what, const msmz_log& got, uint64_t n, uint32_t batch, const msmz_opts* o) {
  msmz_log want{};
  uint64_t local_total = 0;
  for (uint32_t g : c.used(n)) {
    uint64_t cnt = 0;   // entries of the first n on engine g, block by block
    for (uint64_t b = g; b * BLK < n; b += c.G) cnt += std::min(BLK, n - b * BLK);
    local_total += cnt;
    const msmz_log l = toy_log(g, cnt, batch, o);
    for (int i = 0; i < MSMZ_N_STAGES; i++) want.stage_ms[i] = std::max(want.stage_ms[i], l.stage_ms[i]);
    for (int i = 0; i < 32; i++) want.batch_add_ms[i] = std::max(want.batch_add_ms[i], l.batch_add_ms[i]);
    want.scatter_kernel_ms = std::max(want.scatter_kernel_ms, l.scatter_kernel_ms);
    want.n_entries += l.n_entries, want.n_pairs += l.n_pairs, want.scatter_launches += l.scatter_launches;
    want.max_bucket = std::max(want.max_bucket, l.max_bucket);
    want.rounds = std::max(want.rounds, l.rounds);
    want.c = l.c, want.K = l.K, want.glv = l.glv;   // the last used engine's
  }
  bool same = local_total == n && got.n_entries == n * batch && got.n_entries == want.n_entries &&
              got.n_pairs == want.n_pairs && got.scatter_launches == want.scatter_launches &&
              got.max_bucket == want.max_bucket && got.rounds == want.rounds && got.c == want.c && got.K == want.K &&
              got.glv == want.glv && got.scatter_kernel_ms == want.scatter_kernel_ms;
  for (int i = 0; i < MSMZ_N_STAGES; i++) same = same && got.stage_ms[i] == want.stage_ms[i];
  for (int i = 0; i < 32; i++) same = same && got.batch_add_ms[i] == want.batch_add_ms[i];
  CASE(same, "merged log of %s, n' = %llu: c %d K %d glv %d entries %llu", what, (unsigned long long)n, got.c, got.K, got.glv,
       (unsigned long long)got.n_entries);
}

// one size on one context: every operation, every prefix
MSMZ_TEST_MODEL void run_size(Ctx& c, uint64_t n, bool scheduler_cases) {
  snprintf(g_where, sizeof g_where, "G=%u n=%llu", c.G, (unsigned long long)n);
  MultiEngine* me = c.me;
  const uint32_t G = c.G;
  Rng rng{n * 31 + G};
  const std::vector<size_t> live0 = c.live();
  const std::vector<uint64_t> calls0 = c.calls();
  auto ull = [](uint64_t v) { return (unsigned long long)v; };

  // ---- the caller's flat arrays
  const uint64_t nblocks = (n + BLK - 1) / BLK;
  Points P(n), PGf(n), PCf(n);
  Scalars SGf(n), SIf(n), SPf(n), S3(3 * n);
  std::vector<uint32_t> comp(n), narrow(2 * n);
  for (uint64_t i = 0; i < n; i++) {
    uint8_t f;
    uint64_t v = gen_point(11, i, &f);
    P.set(i, f ? mix(i) : v, f);   // (the bytes of a point flagged infinite are junk)
    v = gen_point(21, i, &f);
    PGf.set(i, v, f);
    comp[i] = (uint32_t)mix(i + 77);
    PCf.set(i, expand32(comp[i], (G & 1) != 0), i % 89 == 0);
    SGf.set(i, gen_scalar(22, i));
    narrow[2 * i] = (uint32_t)mix(i + 5), narrow[2 * i + 1] = 0xFFFFFFFFu;   // (stride 8: the odd words are padding)
    SIf.set(i, narrow[2 * i]);
    SPf.set(i, pow_entry(G & 1 ? 1u : 5u, 77u, i));
  }
  for (uint64_t i = 0; i < 3 * n; i++) S3.set(i, gen_scalar(12, i));
  const std::vector<uint8_t> S3w = S3.wire();
  const uint64_t planted[3] = {std::min<uint64_t>(3, n - 1), std::min((nblocks / 2) * BLK + 17, n - 1), n - 1};
  for (int k = 0; k < 3; k++) P.set(planted[k], (P.val(planted[k]) & ~(3ull << 62)) | ((uint64_t)(1 + k % 2) << 62), 0);
  std::vector<uint8_t> strided(n * 16, 0xEE);   // point records at a stride of 16 bytes
  for (uint64_t i = 0; i < n; i++) memcpy(&strided[i * 16], &P.rec[i * 8], 8);

  // ---- A. the sets of n entries: engines beyond the blocks of n stay untouched until part B
  uint64_t PU = 0, PI = 0, PC = 0, PG = 0, SG = 0, SI = 0, SP = 0;
  CASE(me->upload_points(P.rec.data(), P.inf.data(), n, &PU) == MSMZ_OK && PU, "upload_points");
  msmz_src src{};
  src.ptr = strided.data(), src.stride = 16, src.is_inf = P.inf.data();
  CASE(me->import_points(src, n, &PI) == MSMZ_OK && PI, "import_points, stride 16");
  src = msmz_src{};
  src.ptr = comp.data(), src.is_inf = PCf.inf.data();
  src.flags = MSMZ_SRC_COMPRESSED | (G & 1 ? MSMZ_SRC_SIGN_PARITY : 0);
  CASE(me->import_points(src, n, &PC) == MSMZ_OK && PC, "import_points, compressed");
  CASE(me->random_points(n, 21, GenMap{}, &PG) == MSMZ_OK && PG, "random_points");
  CASE(me->random_scalars(n, 22, GenMap{}, &SG) == MSMZ_OK && SG, "random_scalars");
  src = msmz_src{};
  src.ptr = narrow.data(), src.stride = 8, src.width = 4;
  CASE(me->import_scalars(src, n, &SI) == MSMZ_OK && SI, "import_scalars, width 4 stride 8");
  const uint32_t base = 5, ratio = 77;
  CASE(me->scalars_powers(G & 1 ? nullptr : (const uint8_t*)&base, (const uint8_t*)&ratio, n, GenMap{}, &SP) == MSMZ_OK && SP,
       "scalars_powers");
  {
    const std::set<uint64_t> hs{PU, PI, PC, PG, SG, SI, SP};
    CASE(hs.size() == 7 && !hs.count(0), "seven distinct handles");
  }

  const Ranges ranges = make_ranges(n, G, rng);
  check_point_set(c, "uploaded points", PU, P, ranges);
  check_point_set(c, "imported points", PI, P, ranges);
  check_point_set(c, "imported compressed points", PC, PCf, ranges);
  check_point_set(c, "generated points", PG, PGf, ranges);
  check_scalar_set(c, "generated scalars", SG, SGf, ranges);
  check_scalar_set(c, "imported scalars", SI, SIf, ranges);
  check_scalar_set(c, "powers", SP, SPf, ranges);
  {
    int k = 0;
    for (auto [first, count] : ranges) {
      const uint32_t flags = k++ & 1 ? MSMZ_SRC_SIGN_PARITY : 0;
      std::vector<uint8_t> out(count * 4, 0xCC), inf(count, 0xCC);
      const int st = me->download_points_compressed(PG, first, count, out.data(), inf.data(), flags);
      bool same = st == MSMZ_OK && !memcmp(inf.data(), &PGf.inf[first], count);
      for (uint64_t i = 0; i < count && same; i++) same = ld32(&out[i * 4]) == compress64(PGf.val(first + i), flags != 0);
      CASE(same, "download_points_compressed: status %d, range (%llu, %llu)", st, ull(first), ull(count));
    }
  }

  // prefixes n' <= n of the resident sets: a block boundary and one past it, a cycle boundary and one past it
  // (those past the first block only for the sums, which make no set)
  std::vector<uint64_t> prefixes{n};
  size_t n_elementwise = 1;
  for (uint64_t p : {BLK, BLK + 1, (uint64_t)G * BLK + 1, (uint64_t)G * BLK, n - 1})
    if (p && p < n && std::find(prefixes.begin(), prefixes.end(), p) == prefixes.end()) {
      prefixes.push_back(p);
      if (p == BLK || p == BLK + 1) n_elementwise = prefixes.size();
    }

  msmz_opts opts{};
  opts.c = 2;
  for (const uint64_t& np : prefixes) {
    uint64_t want;
    int want_inf, inf1 = -1;
    uint8_t out1[8];
    msmz_log log{};
    // route 1: resident scalars, batch 1 -- every engine reads its own share of both sets
    model_msm(P, SGf.v.data(), np, &want, &want_inf);
    int st = me->msm_batch(PU, nullptr, SG, np, 1, &opts, out1, &inf1, &log);
    CASE(st == MSMZ_OK && same_point(out1, inf1, want, want_inf), "msm resident batch 1, n' = %llu: status %d", ull(np), st);
    check_parallel_log(c, "msm resident batch 1", log, np, 1, &opts);
    // route 3: host scalars, batch 3 -- split copies, vector k at k n' of the caller's buffer
    uint8_t out3[24];
    int inf3[3] = {-1, -1, -1};
    st = me->msm_batch(PI, S3w.data(), 0, np, 3, nullptr, out3, inf3, &log);
    bool same = st == MSMZ_OK;
    for (uint32_t k = 0; k < 3 && same; k++) {
      model_msm(P, &S3.v[k * np], np, &want, &want_inf);
      same = same_point(out3 + 8 * k, inf3[k], want, want_inf);
    }
    CASE(same, "msm host scalars batch 3, n' = %llu: status %d", ull(np), st);
    check_parallel_log(c, "msm host batch 3", log, np, 3, nullptr);

    // scalars_dot: the engines' sums added mod q
    unsigned __int128 dot = 0, sum = 0;
    for (uint64_t i = 0; i < np; i++) dot += (unsigned __int128)SGf.val(i) * SIf.val(i), sum += SGf.val(i);
    uint8_t d[32], wantd[32] = {};
    memcpy(wantd, &dot, 16);
    st = me->scalars_dot(SG, 0, SI, 0, np, d);
    CASE(st == MSMZ_OK && !memcmp(d, wantd, 32), "scalars_dot, n' = %llu: status %d", ull(np), st);
    memcpy(wantd, &sum, 16);
    st = me->scalars_dot(SG, 0, 0, 0, np, d);
    CASE(st == MSMZ_OK && !memcmp(d, wantd, 32), "scalars_dot without y, n' = %llu: status %d", ull(np), st);
    if ((size_t)(&np - prefixes.data()) >= n_elementwise) continue;

    // points_mul: resident scalars and an addend, under options every engine must see
    msmz_mul m{};
    m.points_handle = PU, m.scalars_handle = SG, m.addend_handle = PG;
    msmz_mul_opts mo{};
    mo.flags = MSMZ_MUL_SUBGROUP, mo.scalar_bits = 9;
    uint64_t hm = 0;
    st = me->points_mul(m, mo, np, &hm);
    Points wantm(np);
    for (uint64_t i = 0; i < np; i++)
      wantm.set_group(i, mul_value(SGf.val(i), P.val(i), P.inf[i], true, PGf.val(i), PGf.inf[i], mo));
    CASE(st == MSMZ_OK && whole_points_equal(c, hm, wantm), "points_mul resident + addend, n' = %llu: status %d", ull(np), st);
    CASE(me->download_points(hm, np, 1, out3, nullptr) == MSMZ_ERR_ARG, "the product has n' entries");
    CASE(me->free_handle(hm) == MSMZ_OK, "free the product");

    // scalars_combine into a new set: a broadcast and a resident coefficient
    const uint32_t three = 3;
    msmz_scalar_term x{}, y{};
    x.handle = SG, x.coeff = (const uint8_t*)&three;
    y.handle = SI, y.coeff_handle = SP;
    uint64_t hc = 0;
    st = me->scalars_combine(x, &y, np, 0, &hc);
    Scalars wantc(np);
    for (uint64_t i = 0; i < np; i++) wantc.set(i, 3u * SGf.val(i) + SPf.val(i) * SIf.val(i));
    CASE(st == MSMZ_OK && whole_scalars_equal(c, hc, wantc), "scalars_combine fresh, n' = %llu: status %d", ull(np), st);
    CASE(me->free_handle(hc) == MSMZ_OK, "free the combination");

    // scalars_inverse into a new set: the zero counts of the shares add up
    uint64_t hi = 0, zeros = 12345, want_zeros = 0;
    st = me->scalars_inverse(SG, 0, np, 0, &hi, &zeros);
    Scalars wanti(np);
    for (uint64_t i = 0; i < np; i++) wanti.set(i, toy_inverse(SGf.val(i))), want_zeros += SGf.val(i) == 0;
    CASE(st == MSMZ_OK && zeros == want_zeros && whole_scalars_equal(c, hi, wanti),
         "scalars_inverse fresh, n' = %llu: status %d, zeros %llu (want %llu)", ull(np), st, ull(zeros), ull(want_zeros));
    CASE(me->free_handle(hi) == MSMZ_OK, "free the inverses");

    // precompute: every engine its share; the context answers for the whole set
    const int glv = (int)(np & 1);
    uint64_t hp = 0;
    st = me->precompute_points(PU, np, 5, glv, 3, 64, &hp);
    int32_t ic = 0, iglv = -1, isb = 0;
    uint32_t ifac = 0, iK = 0;
    uint64_t irec = 0;
    const int st2 = me->precomputed_info(hp, &ic, &iglv, &ifac, &iK, &irec, &isb);
    CASE(st == MSMZ_OK && st2 == MSMZ_OK && ic == 5 && iglv == glv && ifac == 3 && iK == 100 && isb == 64 &&
             irec == 3 * np * (glv ? 2 : 1),
         "precompute_points / precomputed_info, n' = %llu: status %d %d, records %llu", ull(np), st, st2, ull(irec));
    model_msm(P, SGf.v.data(), np, &want, &want_inf);
    st = me->msm_batch(hp, nullptr, SG, np, 1, nullptr, out1, &inf1, nullptr);
    CASE(st == MSMZ_OK && same_point(out1, inf1, want, want_inf), "msm over a precomputed set, n' = %llu: status %d", ull(np), st);
    if (np == n) {
      msmz_check_result cr;
      uint64_t h2 = 0;
      CASE(me->check_points(hp, 0, np, MSMZ_CHECK_CURVE, &cr, nullptr) == MSMZ_ERR_UNSUPPORTED, "check_points of a precomputed set");
      CASE(me->check_points(hp, 1, np, MSMZ_CHECK_CURVE, &cr, nullptr) == MSMZ_ERR_UNSUPPORTED,
           "check_points of a precomputed set: UNSUPPORTED before the range, as the header orders them");
      m = msmz_mul{};
      m.points_handle = hp, m.scalars_handle = SG;
      CASE(me->points_mul(m, msmz_mul_opts{}, np, &h2) == MSMZ_ERR_UNSUPPORTED && !h2, "points_mul of a precomputed set");
      CASE(me->precompute_points(hp, np, 5, glv, 3, 0, &h2) == MSMZ_ERR_ARG && !h2, "precompute of a precomputed set");
      CASE(me->precomputed_info(PU, nullptr, nullptr, nullptr, nullptr, &irec, nullptr) == MSMZ_ERR_ARG, "precomputed_info of a plain set");
      CASE(me->msm_batch(hp, nullptr, SG, np + 1, 1, nullptr, out1, &inf1, nullptr) == MSMZ_ERR_ARG, "msm beyond a precomputed set");
    }
    CASE(me->free_handle(hp) == MSMZ_OK, "free the precomputed set");
  }

  // precompute_params is the first engine's
  {
    int pc = 0, pg = 0, pk = 0, ps = 0;
    uint32_t pcopies = 0;
    const int st = me->precompute_params(n, &opts, 0, &pc, &pg, &pcopies, &pk, &ps);
    CASE(st == MSMZ_OK && pc == 7 + (int)(n % 5) && pg == 0 && pcopies == 3 && pk == 11 && ps == 0, "precompute_params");
  }

  // points_mul with one broadcast scalar and no addend; in-place combine and inverse over a whole set
  {
    const uint32_t s = 0x10001;
    msmz_mul m{};
    m.points_handle = PG, m.scalar = (const uint8_t*)&s;
    uint64_t hm = 0;
    int st = me->points_mul(m, msmz_mul_opts{}, n, &hm);
    Points wantm(n);
    for (uint64_t i = 0; i < n; i++) wantm.set_group(i, mul_value(s, PGf.val(i), PGf.inf[i], false, 0, 0, msmz_mul_opts{}));
    CASE(st == MSMZ_OK && whole_points_equal(c, hm, wantm), "points_mul broadcast: status %d", st);
    CASE(me->free_handle(hm) == MSMZ_OK, "free the product");

    msmz_scalar_term x{};
    x.handle = SG;   // coefficient NULL = 1: a copy
    uint64_t D = 0;
    st = me->scalars_combine(x, nullptr, n, 0, &D);
    CASE(st == MSMZ_OK && whole_scalars_equal(c, D, SGf), "scalars_combine, one term, no coefficient: status %d", st);
    const uint32_t nine = 9;
    msmz_scalar_term y{};
    x.handle = D, y.handle = SI, y.coeff = (const uint8_t*)&nine;
    uint64_t same_handle = D;
    const std::vector<size_t> live_before = c.live();
    st = me->scalars_combine(x, &y, n, 0, &same_handle);
    Scalars want(n);
    for (uint64_t i = 0; i < n; i++) want.set(i, SGf.val(i) + 9u * SIf.val(i));
    CASE(st == MSMZ_OK && same_handle == D && c.live() == live_before && whole_scalars_equal(c, D, want),
         "scalars_combine in place over a whole set: status %d", st);
    uint64_t zeros = 777, want_zeros = 0;
    for (uint64_t i = 0; i < n; i++) want_zeros += want.val(i) == 0, want.set(i, toy_inverse(want.val(i)));
    st = me->scalars_inverse(D, 0, n, 0, &same_handle, &zeros);
    CASE(st == MSMZ_OK && same_handle == D && zeros == want_zeros && c.live() == live_before && whole_scalars_equal(c, D, want),
         "scalars_inverse in place over a whole set: status %d, zeros %llu (want %llu)", st, ull(zeros), ull(want_zeros));
    CASE(me->free_handle(D) == MSMZ_OK, "free the copy");
  }

  // check_points: counts, first_bad as a set index and verdict bytes, with and without verdicts
  {
    int k = 0;
    for (auto [first, count] : ranges) {
      const uint32_t what = k++ & 1 ? MSMZ_CHECK_CURVE : MSMZ_CHECK_CURVE | MSMZ_CHECK_SUBGROUP;
      msmz_check_result want{0, 0, UINT64_MAX};
      std::vector<uint8_t> wv(count);
      for (uint64_t i = 0; i < count; i++) {
        const int v = verdict_of(P.val(first + i), P.inf[first + i], what);
        wv[i] = (uint8_t)v;
        want.off_curve += v == 1, want.off_subgroup += v == 2;
        if (v && want.first_bad == UINT64_MAX) want.first_bad = first + i;
      }
      for (int with = 0; with < 2; with++) {
        msmz_check_result got{9, 9, 9};
        std::vector<uint8_t> gv(count, 0xCC);
        const int st = me->check_points(PU, first, count, what, &got, with ? gv.data() : nullptr);
        CASE(st == MSMZ_OK && got.off_curve == want.off_curve && got.off_subgroup == want.off_subgroup &&
                 got.first_bad == want.first_bad && (!with || gv == wv),
             "check_points (%llu, %llu) what %u verdicts %d: status %d, %llu / %llu / %llu, want %llu / %llu / %llu", ull(first),
             ull(count), what, with, st, ull(got.off_curve), ull(got.off_subgroup), ull(got.first_bad), ull(want.off_curve),
             ull(want.off_subgroup), ull(want.first_bad));
      }
    }
    msmz_check_result all;
    CASE(me->check_points(PU, 0, n, 3, &all, nullptr) == MSMZ_OK && all.off_curve >= 2 && all.off_subgroup >= 1 &&
             all.first_bad <= planted[0],
         "the planted points of the first, a middle and the last block are found");
  }

  // out_inf: every share infinity; the first used share infinity and the others not; the shares cancel to infinity
  {
    const std::vector<uint32_t> u = c.used(n);
    Points PX = P;
    Scalars V(3 * n);   // vector 0: all zero
    uint64_t a = 5 % n, b = 0;
    PX.set(a, 0x1234567ull, 0);
    if (u.size() > 1) {
      b = BLK + 2;   // (block 1: the second engine's)
      PX.set(b, 0 - 0x1234567ull, 0);
      for (uint64_t i = 0; i < n; i++) V.set(n + i, c.owner(i) == 0 ? 0 : gen_scalar(33, i) | 1);
      V.set(2 * n + a, 1), V.set(2 * n + b, 1);
    }
    const std::vector<uint8_t> Vw = V.wire();
    uint64_t PXh = 0, Vh = 0;
    CASE(me->upload_points(PX.rec.data(), PX.inf.data(), n, &PXh) == MSMZ_OK, "upload_points");
    uint8_t out[24];
    int inf[3] = {-1, -1, -1};
    int st = me->msm_batch(PXh, Vw.data(), 0, n, 3, nullptr, out, inf, nullptr);
    CASE(st == MSMZ_OK && inf[0] == 1, "out_inf, every share infinity: status %d, flag %d", st, inf[0]);
    if (u.size() > 1) {
      uint64_t want;
      int want_inf;
      model_msm(PX, &V.v[n], n, &want, &want_inf);
      CASE(!want_inf && same_point(out + 8, inf[1], want, 0), "out_inf, the first share infinity and the others not: flag %d", inf[1]);
      CASE(inf[2] == 1, "out_inf, the shares cancel: flag %d", inf[2]);
    }
    for (uint32_t k = 0; k < (u.size() > 1 ? 3u : 1u); k++) {   // the same three through resident scalars, batch 1
      uint64_t want;
      int want_inf, got_inf = -1;
      model_msm(PX, &V.v[k * n], n, &want, &want_inf);
      CASE(me->upload_scalars(&Vw[k * n * 32], n, &Vh) == MSMZ_OK, "upload_scalars");
      st = me->msm_batch(PXh, nullptr, Vh, n, 1, nullptr, out, &got_inf, nullptr);
      CASE(st == MSMZ_OK && want_inf == (k != 1) && same_point(out, got_inf, want, want_inf),
           "out_inf case %u, resident scalars: status %d, flag %d", k, st, got_inf);
      CASE(me->free_handle(Vh) == MSMZ_OK, "free the vector");
    }
    CASE(me->free_handle(PXh) == MSMZ_OK, "free the points");
  }

  // ---- refusals, in the order the header promises: argument errors first, then UNSUPPORTED; no engine is called
  if (n > 2) {
    const uint64_t before = c.total_calls();
    const std::vector<size_t> live_before = c.live();
    uint64_t h = 0, dst = SP;
    uint8_t buf[32];
    msmz_mul m{};
    m.points_handle = PU, m.scalars_handle = SG, m.addend_handle = PG;
    for (int which = 0; which < 3; which++) {
      msmz_mul s = m;
      (which == 0 ? s.first_p : which == 1 ? s.first_s : s.first_q) = 1;
      CASE(me->points_mul(s, msmz_mul_opts{}, n, &h) == MSMZ_ERR_ARG && !h, "points_mul, shifted range %d beyond its set", which);
      CASE(me->points_mul(s, msmz_mul_opts{}, n - 1, &h) == MSMZ_ERR_UNSUPPORTED && !h, "points_mul, shifted range %d", which);
    }
    m.scalars_handle = 0;
    CASE(me->points_mul(m, msmz_mul_opts{}, n, &h) == MSMZ_ERR_ARG, "points_mul without a scalar");
    m.scalars_handle = PU;
    CASE(me->points_mul(m, msmz_mul_opts{}, n, &h) == MSMZ_ERR_ARG, "points_mul with a point set as scalars");

    msmz_scalar_term x{}, y{};
    x.handle = SG, y.handle = SI, y.coeff_handle = SP;
    for (int which = 0; which < 4; which++) {
      msmz_scalar_term xs = x, ys = y;
      uint64_t first_out = 0, out = which == 3 ? dst : 0;
      (which == 0 ? xs.first : which == 1 ? ys.first : which == 2 ? ys.coeff_first : first_out) = 1;
      CASE(me->scalars_combine(xs, &ys, n, first_out, &out) == MSMZ_ERR_ARG, "scalars_combine, shifted range %d beyond its set", which);
      CASE(me->scalars_combine(xs, &ys, n - 1, first_out, &out) == MSMZ_ERR_UNSUPPORTED, "scalars_combine, shifted range %d", which);
    }
    CASE(me->scalars_combine(x, &y, n - 1, 1, &h) == MSMZ_ERR_ARG && !h, "scalars_combine, first_out with a new handle");
    CASE(me->scalars_combine(x, &y, n - 1, 0, &dst) == MSMZ_ERR_UNSUPPORTED && dst == SP, "scalars_combine, a destination not written whole");
    CASE(me->scalars_combine(x, &y, n + 1, 0, &dst) == MSMZ_ERR_ARG, "scalars_combine beyond the sets");
    dst = PU;
    CASE(me->scalars_combine(x, &y, n, 0, &dst) == MSMZ_ERR_ARG, "scalars_combine into a point set");
    dst = SP;

    CASE(me->scalars_dot(SG, 1, SI, 0, n, buf) == MSMZ_ERR_ARG, "scalars_dot, shifted x beyond its set");
    CASE(me->scalars_dot(SG, 1, SI, 0, n - 1, buf) == MSMZ_ERR_UNSUPPORTED, "scalars_dot, shifted x");
    CASE(me->scalars_dot(SG, 0, SI, 1, n, buf) == MSMZ_ERR_ARG, "scalars_dot, shifted y beyond its set");
    CASE(me->scalars_dot(SG, 0, SI, 1, n - 1, buf) == MSMZ_ERR_UNSUPPORTED, "scalars_dot, shifted y");
    CASE(me->scalars_dot(SG, 0, 0, 1, n - 1, buf) == MSMZ_ERR_ARG, "scalars_dot, first_y without y");
    CASE(me->scalars_dot(SG, 0, PU, 0, n, buf) == MSMZ_ERR_ARG, "scalars_dot with a point set");

    uint64_t zeros = 4242;
    CASE(me->scalars_inverse(SG, 1, n, 0, &h, &zeros) == MSMZ_ERR_ARG && !h, "scalars_inverse, shifted range beyond its set");
    CASE(me->scalars_inverse(SG, 1, n - 1, 0, &h, &zeros) == MSMZ_ERR_UNSUPPORTED && !h, "scalars_inverse, shifted range");
    CASE(me->scalars_inverse(SG, 0, n - 1, 1, &h, &zeros) == MSMZ_ERR_ARG, "scalars_inverse, first_out with a new handle");
    CASE(me->scalars_inverse(SG, 0, n - 1, 1, &dst, &zeros) == MSMZ_ERR_UNSUPPORTED, "scalars_inverse, shifted destination");
    CASE(me->scalars_inverse(SG, 0, n, 1, &dst, &zeros) == MSMZ_ERR_ARG, "scalars_inverse, shifted destination beyond its set");
    CASE(me->scalars_inverse(SG, 0, n - 1, 0, &dst, &zeros) == MSMZ_ERR_UNSUPPORTED, "scalars_inverse, a destination not written whole");
    CASE(me->scalars_inverse(SP, 0, n - 1, 1, &dst, &zeros) == MSMZ_ERR_ARG, "scalars_inverse, partial overlap: ARG before UNSUPPORTED");
    CASE(zeros == 4242 && dst == SP, "a refused scalars_inverse writes nothing");

    msmz_segment seg{0, 0, n};
    int one_inf;
    CASE(me->msm_segments(PU, SG, &seg, 1, nullptr, buf, &one_inf, nullptr) == MSMZ_ERR_UNSUPPORTED, "msm_segments");
    src = msmz_src{};
    src.ptr = narrow.data(), src.width = 4;
    CASE(me->import_scalars_into(SG, 0, src, 1) == MSMZ_ERR_UNSUPPORTED, "import_scalars_into");
    CASE(me->alloc_scalars(n, &h) == MSMZ_ERR_UNSUPPORTED, "alloc_scalars");
    msmz_scalar_rec r{};
    r.b_handle = SG;
    CASE(me->scalars_recurrence(r, n, 0, &h, nullptr) == MSMZ_ERR_UNSUPPORTED, "scalars_recurrence");
    CASE(me->scalars_recurrence(r, 0, 0, &h, nullptr) == MSMZ_ERR_ARG, "scalars_recurrence, n = 0");
    CASE(me->scalars_recurrence(r, n, 0, nullptr, nullptr) == MSMZ_ERR_ARG, "scalars_recurrence, no handle pointer");
    r.flags = 4;
    CASE(me->scalars_recurrence(r, n, 0, &h, nullptr) == MSMZ_ERR_ARG, "scalars_recurrence, unknown flag");
    r = msmz_scalar_rec{};
    CASE(me->scalars_recurrence(r, n, 0, &h, nullptr) == MSMZ_ERR_ARG, "scalars_recurrence, neither multiplier nor addend");
    msmz_ntt t{};
    t.handle = SG, t.log_n = 1, t.count = 1;
    CASE(me->scalars_ntt(t, 0, &h) == MSMZ_ERR_UNSUPPORTED, "scalars_ntt");
    t.count = 0;
    CASE(me->scalars_ntt(t, 0, &h) == MSMZ_ERR_ARG, "scalars_ntt, count = 0");
    t.count = 1, t.flags = 8;
    CASE(me->scalars_ntt(t, 0, &h) == MSMZ_ERR_ARG, "scalars_ntt, unknown flag");
    t.flags = MSMZ_NTT_COSET;
    CASE(me->scalars_ntt(t, 0, &h) == MSMZ_ERR_ARG, "scalars_ntt, coset without a shift");
    t.flags = 0, t.shift = buf;
    CASE(me->scalars_ntt(t, 0, &h) == MSMZ_ERR_ARG, "scalars_ntt, a shift without coset");

    // the plain argument errors
    int inf1;
    msmz_check_result cr;
    CASE(me->upload_points(nullptr, nullptr, n, &h) == MSMZ_ERR_ARG && me->upload_points(P.rec.data(), nullptr, 0, &h) == MSMZ_ERR_ARG &&
             me->upload_points(P.rec.data(), nullptr, n, nullptr) == MSMZ_ERR_ARG && me->upload_scalars(nullptr, n, &h) == MSMZ_ERR_ARG &&
             me->random_points(0, 1, GenMap{}, &h) == MSMZ_ERR_ARG && me->random_scalars(n, 1, GenMap{}, nullptr) == MSMZ_ERR_ARG &&
             me->scalars_powers(nullptr, nullptr, n, GenMap{}, &h) == MSMZ_ERR_ARG,
         "null pointers and n = 0 in the set makers");
    CASE(me->download_points(PU, 1, n, buf, nullptr) == MSMZ_ERR_ARG && me->download_points(SG, 0, 1, buf, nullptr) == MSMZ_ERR_ARG &&
             me->download_scalars(PU, 0, 1, buf) == MSMZ_ERR_ARG && me->download_scalars(SG, n, 1, buf) == MSMZ_ERR_ARG &&
             me->download_scalars(987654, 0, 1, buf) == MSMZ_ERR_ARG && me->download_points_compressed(PU, 0, 1, buf, nullptr, 1) == MSMZ_ERR_ARG &&
             me->download_points_compressed(PU, n, 1, buf, nullptr, 0) == MSMZ_ERR_ARG && me->free_handle(987654) == MSMZ_ERR_ARG,
         "downloads: beyond the set, wrong kind, unknown handle, unknown flag");
    CASE(me->msm_batch(PU, nullptr, SG, n + 1, 1, nullptr, buf, &inf1, nullptr) == MSMZ_ERR_ARG &&
             me->msm_batch(PU, nullptr, SG, n / 2 + 1, 2, nullptr, buf, &inf1, nullptr) == MSMZ_ERR_ARG &&
             me->msm_batch(PU, nullptr, PG, n, 1, nullptr, buf, &inf1, nullptr) == MSMZ_ERR_ARG &&
             me->msm_batch(SG, nullptr, SG, n, 1, nullptr, buf, &inf1, nullptr) == MSMZ_ERR_ARG &&
             me->msm_batch(PU, nullptr, SG, n, 0, nullptr, buf, &inf1, nullptr) == MSMZ_ERR_ARG &&
             me->msm_batch(PU, nullptr, SG, 0, 1, nullptr, buf, &inf1, nullptr) == MSMZ_ERR_ARG &&
             me->msm_batch(PU, nullptr, SG, n, 1, nullptr, nullptr, &inf1, nullptr) == MSMZ_ERR_ARG,
         "msm_batch: beyond either set, wrong kinds, batch = 0, n = 0, no output");
    CASE(me->check_points(PU, 0, n, 0, &cr, nullptr) == MSMZ_ERR_ARG && me->check_points(PU, 0, n, 4, &cr, nullptr) == MSMZ_ERR_ARG &&
             me->check_points(PU, 1, n, 1, &cr, nullptr) == MSMZ_ERR_ARG && me->check_points(PU, 0, 0, 1, &cr, nullptr) == MSMZ_ERR_ARG &&
             me->check_points(SG, 0, n, 1, &cr, nullptr) == MSMZ_ERR_ARG && me->check_points(PU, 0, n, 1, nullptr, nullptr) == MSMZ_ERR_ARG,
         "check_points: what, range, kind, no result");
    CASE(c.total_calls() == before && c.live() == live_before && c.sh.forbidden == 0, "a refused call reaches no engine");
  }

  // ---- the scheduler
  const std::vector<uint32_t> u = c.used(n);
  if (u.size() > 1) {
    // (b) the engines run side by side: every mock waits inside msm_batch until all engines with a share are in
    c.sh.barrier.arm((uint32_t)u.size());
    uint64_t want;
    int want_inf, inf1 = -1;
    uint8_t out1[8];
    model_msm(P, SGf.v.data(), n, &want, &want_inf);
    const int st = me->msm_batch(PU, nullptr, SG, n, 1, nullptr, out1, &inf1, nullptr);
    CASE(c.sh.barrier.met(), "the %zu engines with a share were inside msm_batch at the same time", u.size());
    CASE(st == MSMZ_OK && same_point(out1, inf1, want, want_inf), "msm_batch behind the barrier: status %d", st);
    c.sh.barrier.arm(0);
  }
  if (scheduler_cases) {
    // (c) error precedence and (d) cleanup, on every kind of call; every engine holds a share of n here
    const uint32_t mid = G / 2, last = G - 1;
    struct Inject {
      uint32_t g0;
      int s0;
      uint32_t g1;
      int s1;
      int want;
    };
    std::vector<Inject> patterns{{0, MSMZ_ERR_HIP, 0, 0, MSMZ_ERR_HIP},
                                 {mid, MSMZ_ERR_DEGENERATE, 0, 0, MSMZ_ERR_DEGENERATE},
                                 {last, MSMZ_ERR_RANGE, 0, 0, MSMZ_ERR_RANGE}};
    if (G > 1) {
      patterns.push_back({0, MSMZ_ERR_HIP, last, MSMZ_ERR_RANGE, MSMZ_ERR_HIP});        // the first in device order
      patterns.push_back({0, MSMZ_ERR_POINT, last, MSMZ_ERR_RANGE, MSMZ_ERR_RANGE});    // RANGE beats POINT
      patterns.push_back({0, MSMZ_ERR_RANGE, last, MSMZ_ERR_POINT, MSMZ_ERR_RANGE});
      patterns.push_back({0, MSMZ_ERR_POINT, last, MSMZ_ERR_HIP, MSMZ_ERR_POINT});      // and nothing else does
      patterns.push_back({mid, MSMZ_ERR_POINT, last, MSMZ_ERR_POINT, MSMZ_ERR_POINT});
    }
    const uint64_t SENTINEL = 0xABCDEF;
    uint64_t D = 0;
    msmz_scalar_term copy{};
    copy.handle = SG;
    CASE(me->scalars_combine(copy, nullptr, n, 0, &D) == MSMZ_OK, "a destination for the in-place calls");
    struct Op {
      const char* name;
      bool makes_set, fresh_by_zero, every_pattern;
      std::function<int(uint64_t*)> run;
    };
    uint8_t out[32];
    int one_inf;
    msmz_check_result cr;
    uint64_t zeros;
    msmz_mul m{};
    m.points_handle = PU, m.scalars_handle = SG;
    msmz_scalar_term x{}, xd{};
    x.handle = SG, xd.handle = D;
    src = msmz_src{};
    src.ptr = narrow.data(), src.stride = 8, src.width = 4;
    const std::vector<Op> ops{
        {"upload_points", true, false, false, [&](uint64_t* h) { return me->upload_points(P.rec.data(), P.inf.data(), n, h); }},
        {"upload_scalars", true, false, false, [&](uint64_t* h) { return me->upload_scalars(S3w.data(), n, h); }},
        {"import_scalars", true, false, false, [&](uint64_t* h) { return me->import_scalars(src, n, h); }},
        {"random_points", true, false, true, [&](uint64_t* h) { return me->random_points(n, 3, GenMap{}, h); }},
        {"scalars_powers", true, false, false, [&](uint64_t* h) { return me->scalars_powers(nullptr, (const uint8_t*)&ratio, n, GenMap{}, h); }},
        {"points_mul", true, false, false, [&](uint64_t* h) { return me->points_mul(m, msmz_mul_opts{}, n, h); }},
        {"scalars_combine", true, true, false, [&](uint64_t* h) { return me->scalars_combine(x, nullptr, n, 0, h); }},
        {"scalars_inverse", true, true, false, [&](uint64_t* h) { return me->scalars_inverse(SG, 0, n, 0, h, &zeros); }},
        {"precompute_points", true, false, false, [&](uint64_t* h) { return me->precompute_points(PU, n, 5, 1, 2, 0, h); }},
        {"scalars_combine in place", false, false, false, [&](uint64_t*) { uint64_t d = D; return me->scalars_combine(xd, nullptr, n, 0, &d); }},
        {"scalars_inverse in place", false, false, false, [&](uint64_t*) { uint64_t d = D; return me->scalars_inverse(SG, 0, n, 0, &d, nullptr); }},
        {"msm_batch", false, false, true, [&](uint64_t*) { return me->msm_batch(PU, nullptr, SG, n, 1, nullptr, out, &one_inf, nullptr); }},
        {"msm_batch, host scalars", false, false, false, [&](uint64_t*) { return me->msm_batch(PU, S3w.data(), 0, n, 1, nullptr, out, &one_inf, nullptr); }},
        {"check_points", false, false, true, [&](uint64_t*) { return me->check_points(PU, 0, n, 3, &cr, nullptr); }},
        {"scalars_dot", false, false, false, [&](uint64_t*) { return me->scalars_dot(SG, 0, SI, 0, n, out); }},
    };
    for (const Op& op : ops) {
      for (const Inject& p : patterns) {
        // every pattern for three kinds of call; the others fail once, the engine taking turns
        if (!op.every_pattern && (size_t)(&p - patterns.data()) != (size_t)(&op - ops.data()) % 3) continue;
        const std::vector<size_t> live_before = c.live();
        c.inject(p.g0, p.s0);
        if (p.s1) c.inject(p.g1, p.s1);
        uint64_t h = op.fresh_by_zero ? 0 : SENTINEL;   // (combine and inverse make a new set only for *out_handle == 0)
        const uint64_t h_in = h;
        const int st = op.run(&h);
        const bool consumed = c.injections_consumed();
        CASE(st == p.want && consumed, "%s with status %d on engine %u and %d on engine %u: status %d, want %d", op.name, p.s0, p.g0,
             p.s1, p.g1, st, p.want);
        CASE(h == h_in && c.live() == live_before, "%s after a failure: no engine keeps a share and no handle was given out", op.name);
        // the very next call on the same context succeeds
        h = 0;
        const int st2 = op.run(&h);
        const bool grown = c.live_is(live_before, op.makes_set ? 1 : 0);
        CASE(st2 == MSMZ_OK && grown && (h != 0) == op.makes_set, "%s right after a failure: status %d", op.name, st2);
        if (op.makes_set) CASE(me->free_handle(h) == MSMZ_OK && c.live() == live_before, "free what the retry made");
      }
    }
    {
      uint64_t h = 0;
      CASE(me->upload_points(P.rec.data(), P.inf.data(), n, &h) == MSMZ_OK && whole_points_equal(c, h, P) &&
               me->free_handle(h) == MSMZ_OK,
           "an upload after all the failures holds the caller's points");
      uint64_t want;
      int want_inf;
      model_msm(P, SGf.v.data(), n, &want, &want_inf);
      CASE(me->msm_batch(PU, nullptr, SG, n, 1, nullptr, out, &one_inf, nullptr) == MSMZ_OK && same_point(out, one_inf, want, want_inf),
           "an MSM after all the failures is right");
    }
    CASE(me->free_handle(D) == MSMZ_OK, "free the destination");
  }

  // an engine without a share of these sets received no call at all (its sub-handles are 0: nothing to free either)
  {
    const std::vector<uint64_t> now = c.calls();
    bool idle = true, busy = true;
    for (uint32_t g = 0; g < G; g++) {
      if (g * BLK < n) busy = busy && now[g] > calls0[g];
      else idle = idle && now[g] == calls0[g];
    }
    CASE(idle && busy, "engines without a share of n entries receive no call; the others do");
  }

  // ---- B. a scalar set of 3 n entries: batch 3 over resident scalars goes through the host (vector k starts at k n')
  uint64_t SU = 0;
  CASE(me->upload_scalars(S3w.data(), 3 * n, &SU) == MSMZ_OK && SU, "upload_scalars, 3 n");
  check_scalar_set(c, "uploaded scalars", SU, S3, make_ranges(3 * n, G, rng));
  for (uint64_t np : prefixes) {
    if (np != n && np != BLK + 1) continue;   // (3 n' records come to the host each time)
    uint8_t out3[24];
    int inf3[3] = {-1, -1, -1};
    msmz_log log{};
    const int st = me->msm_batch(PG, nullptr, SU, np, 3, &opts, out3, inf3, &log);
    bool same = st == MSMZ_OK;
    for (uint32_t k = 0; k < 3 && same; k++) {
      uint64_t want;
      int want_inf;
      model_msm(PGf, &S3.v[k * np], np, &want, &want_inf);
      same = same_point(out3 + 8 * k, inf3[k], want, want_inf);
    }
    CASE(same, "msm resident scalars batch 3, n' = %llu: status %d", ull(np), st);
    check_parallel_log(c, "msm resident batch 3", log, np, 3, &opts);
  }
  {
    uint8_t out3[24];
    int inf3[3];
    CASE(me->msm_batch(PG, nullptr, SU, n, 4, nullptr, out3, inf3, nullptr) == MSMZ_ERR_ARG, "batch 4 of n over 3 n scalars");
  }

  // ---- free everything: every engine is back where it was
  for (uint64_t h : {PU, PI, PC, PG, SG, SI, SP, SU}) CASE(me->free_handle(h) == MSMZ_OK, "free_handle");
  CASE(me->free_handle(PU) == MSMZ_ERR_ARG, "a freed handle is unknown");
  CASE(c.live() == live0, "every share is freed");
  {
    const std::vector<uint64_t> now = c.calls();
    bool idle = true;
    for (uint32_t g = 0; g < G; g++) idle = idle && (g * BLK < 3 * n || now[g] == calls0[g]);
    CASE(idle, "engines without a share of 3 n entries receive no call, frees included");
  }
}

void run_context(uint32_t G) {
  {
    Ctx* c = new Ctx(G);
    for (uint64_t n : {(uint64_t)100, BLK + 5, (uint64_t)G * BLK, (uint64_t)(2 * G + 1) * BLK + 777})
      run_size(*c, n, n == (uint64_t)G * BLK);

    snprintf(g_where, sizeof g_where, "G=%u", G);
    // the test hooks: settings go to every engine, counters add up, the stage hooks are the first engine's
    CASE(c->me->test_set_glv_bits(100) == MSMZ_OK && c->me->test_set_limits(7, 9) == MSMZ_OK, "test_set_glv_bits / test_set_limits");
    bool all = true;
    for (Mock* m : c->mocks) all = all && m->glv_bits == 100 && m->limits[0] == 7 && m->limits[1] == 9;
    CASE(all, "the test settings reach every engine");
    uint64_t rp = 0, sb = 0;
    c->me->test_passes(&rp, &sb);
    CASE(c->me->test_retries() == (int)(G * (G + 1) / 2) && rp == (uint64_t)G * (G + 1) / 2 && sb == (uint64_t)G * G,
         "test_retries / test_passes are summed over the engines");
    CASE(c->me->test_hooks() == reinterpret_cast<ITestHooks*>(c->mocks[0]), "the stage hooks are the first engine's");
    c->mocks[G - 1]->hook_status = MSMZ_ERR_HIP, c->mocks[0]->hook_status = G > 1 ? MSMZ_ERR_ARG : MSMZ_ERR_HIP;
    CASE(c->me->test_set_glv_bits(0) == (G > 1 ? MSMZ_ERR_ARG : MSMZ_ERR_HIP) && c->mocks[G - 1]->glv_bits == 0,
         "a failing test setting: every engine is still asked, the first status is returned");

    // (a) one thread per engine for the life of the context, all distinct, none the caller's
    std::set<std::thread::id> tids;
    bool worked = true;
    for (Mock* m : c->mocks) worked = worked && m->has_tid && m->worker_calls > 0, tids.insert(m->tid);
    CASE(worked && c->sh.thread_violations == 0, "every call posted for an engine arrives on one and the same thread");
    CASE(tids.size() == G && !tids.count(std::this_thread::get_id()), "the %u engine threads are distinct and not the caller's", G);
    CASE(c->sh.forbidden == 0, "no refused operation was forwarded to an engine");

    // (e) teardown with sets still resident: the workers are joined and all G engines deleted
    uint64_t h = 0;
    const uint32_t ratio = 3;
    CASE(c->me->scalars_powers(nullptr, (const uint8_t*)&ratio, (uint64_t)G * BLK, GenMap{}, &h) == MSMZ_OK, "a set left behind");
    MultiEngine* me = c->me;
    CASE(c->sh.destroyed == 0, "no engine is deleted while the context lives");
    delete me;
    CASE(c->sh.destroyed == (int)G, "destroying the context deletes all %u engines (%d deleted)", G, (int)c->sh.destroyed);
    delete c;
  }
}

// ---------------------------------------------------------------------------------------------- free functions
template <class Fr>
void q_minus(uint32_t k, uint32_t* out) {   // q - k, word by word
  uint64_t borrow = k;
  for (int j = 0; j < 8; j++) {
    const uint64_t w = Fr::Q[j];
    out[j] = (uint32_t)(w - borrow);
    borrow = w < borrow ? 1 : 0;
  }
}

void fold_scalar_cases() {
  snprintf(g_where, sizeof g_where, "fold_scalar");
  for (int curve = 0; curve < 4; curve++) {
    for (uint32_t G : {2u, 8u}) {
      uint32_t part[8], want[8], acc[8] = {};
      switch (curve) {
        case MSMZ_BLS12_377_G1: q_minus<Bls377Fr>(1, part), q_minus<Bls377Fr>(G, want); break;
        case MSMZ_PALLAS: q_minus<PallasFr>(1, part), q_minus<PallasFr>(G, want); break;
        case MSMZ_BLS12_381_G1: q_minus<Bls381Fr>(1, part), q_minus<Bls381Fr>(G, want); break;
        default: q_minus<Ed377Fr>(1, part), q_minus<Ed377Fr>(G, want); break;
      }
      int st = MSMZ_OK;
      for (uint32_t g = 0; g < G && !st; g++) st = fold_scalar(curve, acc, part);
      CASE(st == MSMZ_OK && !memcmp(acc, want, 32), "curve %d: %u parts of q - 1 give q - %u", curve, G, G);
    }
  }
  uint32_t acc[8] = {}, part[8] = {1};
  CASE(fold_scalar(4, acc, part) == MSMZ_ERR_UNSUPPORTED && acc[0] == 0, "an unknown curve");
}

void merge_log_sequential_case() {
  snprintf(g_where, sizeof g_where, "merge_log");
  msmz_log total{};
  total.c = 99;
  const msmz_log a = toy_log(4, 1000, 1, nullptr), b = toy_log(1, 500, 2, nullptr), d = toy_log(6, 10, 1, nullptr);
  merge_log(&total, a, true, LogMerge::SEQUENTIAL);
  merge_log(&total, b, false, LogMerge::SEQUENTIAL);
  merge_log(&total, d, false, LogMerge::SEQUENTIAL);
  bool same = total.c == a.c && total.K == a.K && total.glv == a.glv && total.n_entries == 1000 + 1000 + 10 &&
              total.n_pairs == a.n_pairs + b.n_pairs + d.n_pairs &&
              total.scatter_launches == a.scatter_launches + b.scatter_launches + d.scatter_launches &&
              total.max_bucket == std::max({a.max_bucket, b.max_bucket, d.max_bucket}) &&
              total.rounds == std::max({a.rounds, b.rounds, d.rounds}) &&
              total.scatter_kernel_ms == a.scatter_kernel_ms + b.scatter_kernel_ms + d.scatter_kernel_ms;
  for (int i = 0; i < MSMZ_N_STAGES; i++) same = same && total.stage_ms[i] == a.stage_ms[i] + b.stage_ms[i] + d.stage_ms[i];
  for (int i = 0; i < 32; i++) same = same && total.batch_add_ms[i] == a.batch_add_ms[i] + b.batch_add_ms[i] + d.batch_add_ms[i];
  CASE(same, "SEQUENTIAL: times and counts add, max_bucket and rounds take the maximum, c / K / glv are the first part's");
}

}  // namespace

int main() {
  fold_scalar_cases();
  merge_log_sequential_case();
  for (uint32_t G : {1u, 2u, 3u, 5u, 7u, 8u}) run_context(G);
  printf("cases %ld\n", g_cases);
  if (g_fails) printf("failures %d\n", g_fails);
  return g_fails ? 1 : 0;
}

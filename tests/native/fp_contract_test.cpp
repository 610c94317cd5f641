// Contract checker for the lazy-limb arithmetic of msm_zprize_amd/csrc/fp.h and curve.h, compiled for the host.
//
// Every field type F is wrapped in Traced<F>, and fe_mul / fe_sqr / fe_reduce_small / fe_store / fe_store_mulout /
// fe_is_zero get explicit specialisations for the wrapped types.  Each specialisation checks its operands against the
// bounds documented in fp.h, calls the real routine of the base field on a copy of the limbs, and checks the output
// range the routine claims.  The curve formulas of curve.h then run unchanged on the traced types, so every call
// inside them is checked.  Driven by tests/test_fp_contract.py through stdin / stdout (one output line per command);
// at the end the worst value / limb magnitude seen at each call site goes to stderr, and the exit code is 1 if any
// bound was broken.
//
// Elements on the command line: hex = memory words (fe_unpack, as the kernels load them), or "L" followed by N
// comma-separated signed limbs = raw register limbs.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <type_traits>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/test_ops.h"

namespace msmz {

template <class B>
struct Traced : B {
  using Base = B;
};

// ------------------------------------------------------------------------------------------------ exact bound checks
// sign of den * v - num * p  for the value v of lazy limbs (exact: 64-bit limb arithmetic, full carry)
template <class F>
static int cmp_kp(const Fe<F>& a, int64_t num, int64_t den) {
  constexpr int N = F::N, W = F::W;
  constexpr int64_t MASK = ((int64_t)1 << W) - 1;
  int64_t t[N], c = 0;
  for (int j = 0; j < N; j++) t[j] = den * a.l[j] - num * F::PL[j];
  bool low = false;
  for (int j = 0; j < N - 1; j++) {
    t[j] += c;
    c = t[j] >> W;
    t[j] &= MASK;
    low |= t[j] != 0;
  }
  t[N - 1] += c;
  if (t[N - 1] != 0) return t[N - 1] > 0 ? 1 : -1;
  return low ? 1 : 0;
}

// v = k p for some |k| <= kmax ?
template <class F>
static bool is_multiple(const Fe<F>& a, int kmax) {
  for (int k = -kmax; k <= kmax; k++)
    if (cmp_kp(a, k, 1) == 0) return true;
  return false;
}

template <class F>
static bool within(const Fe<F>& a, int64_t num, int64_t den) {   // |v| < num/den * p
  return cmp_kp(a, num, den) < 0 && cmp_kp(a, -num, den) > 0;
}

template <class F>
static long double value_over_p(const Fe<F>& a) {
  long double v = 0, p = 0;
  for (int j = F::N - 1; j >= 0; j--) {
    v = v * (long double)(1 << F::W) + a.l[j];
    p = p * (long double)(1 << F::W) + F::PL[j];
  }
  return v / p;
}

template <class F>
static int64_t max_limb(const Fe<F>& a) {
  int64_t m = 0;
  for (int j = 0; j < F::N; j++) m = std::max<int64_t>(m, std::llabs((int64_t)a.l[j]));
  return m;
}

template <class F>
static bool low_limbs_normalized(const Fe<F>& a) {
  for (int j = 0; j < F::N - 1; j++)
    if (a.l[j] < 0 || a.l[j] >= (1 << F::W)) return false;
  return true;
}

// ------------------------------------------------------------------------------------------------ per-site statistics
struct Site {
  long calls = 0, viol = 0;
  double v_in = 0;          // worst |input value| / p
  double limb_in = 0;       // worst input limb magnitude (log2)
  double prod = 0;          // worst log2(N A B + N 2^(2W)) (mul / sqr)
  double out_lo = 1e9, out_hi = -1e9;   // output value / p range
  double v_bound = 0;       // the documented input bound / p
};
static std::map<std::string, Site> g_sites;
static std::string g_field, g_scope;
static std::map<std::string, int> g_ordinal;   // per routine, reset when the scope changes
static long g_violations = 0;

static void set_scope(const char* s) {
  g_scope = s;
  g_ordinal.clear();
}

static Site& site(const char* routine, double bound) {
  const int k = g_ordinal[routine]++;
  Site& s = g_sites[g_field + " " + g_scope + ":" + routine + "#" + std::to_string(k)];
  s.calls++;
  s.v_bound = bound;
  return s;
}

static void violation(Site& s, const char* routine, const char* what, double v) {
  s.viol++;
  if (g_violations++ < 20)
    fprintf(stderr, "VIOLATION %s %s:%s: %s (value/p = %.6f)\n", g_field.c_str(), g_scope.c_str(), routine, what, v);
}

template <class F>
static void note_in(Site& s, const Fe<F>& a) {
  s.v_in = std::max(s.v_in, (double)fabsl(value_over_p(a)));
  s.limb_in = std::max(s.limb_in, log2((double)max_limb(a) + 1));
}
template <class F>
static void note_out(Site& s, const Fe<F>& r) {
  const double v = (double)value_over_p(r);
  s.out_lo = std::min(s.out_lo, v);
  s.out_hi = std::max(s.out_hi, v);
}

// mul / sqr: |v| < 2^5 p (2^3 p for the 255-bit fields), N A B + N 2^(2W) < 2^63; out in (-1.5p, 0.5p) with
// normalized limbs 0..N-2
template <class F>
static constexpr int64_t mul_bound() { return F::N == 14 ? 32 : 8; }

template <class T>
static void check_mul_in(Site& s, const char* rt, const Fe<T>& a, const Fe<T>& b) {
  note_in(s, a);
  note_in(s, b);
  if (!within(a, mul_bound<T>(), 1)) violation(s, rt, "input a out of the value bound", (double)value_over_p(a));
  if (!within(b, mul_bound<T>(), 1)) violation(s, rt, "input b out of the value bound", (double)value_over_p(b));
  const __int128 N = T::N;
  const __int128 lhs = N * max_limb(a) * max_limb(b) + N * ((__int128)1 << (2 * T::W));
  s.prod = std::max(s.prod, log2((double)lhs));
  if (lhs >= ((__int128)1 << 63)) violation(s, rt, "limb products: N*A*B + N*2^(2W) >= 2^63", log2((double)lhs));
}
template <class T>
static void check_mul_out(Site& s, const char* rt, const Fe<T>& r) {
  note_out(s, r);
  if (!(cmp_kp(r, 1, 2) < 0 && cmp_kp(r, -3, 2) > 0)) violation(s, rt, "output not in (-1.5p, 0.5p)", (double)value_over_p(r));
  if (!low_limbs_normalized(r)) violation(s, rt, "output limbs not normalized", 0);
}

// reduced value: [0, 3p), normalized limbs, same class as the input
template <class T>
static void check_reduced(Site& s, const char* rt, const Fe<T>& in, const Fe<T>& r) {
  note_out(s, r);
  if (!(cmp_kp(r, 0, 1) >= 0 && cmp_kp(r, 3, 1) < 0)) violation(s, rt, "output not in [0, 3p)", (double)value_over_p(r));
  if (!low_limbs_normalized(r) || r.l[T::N - 1] < 0) violation(s, rt, "output limbs not normalized", 0);
  Fe<T> d;
  fe_sub(d, in, r);
  if (!is_multiple(d, 20)) violation(s, rt, "output not congruent to the input", (double)value_over_p(r));
}

template <class T>
static Fe<typename T::Base> down(const Fe<T>& a) {
  Fe<typename T::Base> r;
  memcpy(r.l, a.l, sizeof(r.l));
  return r;
}
template <class T>
static Fe<T> up(const Fe<typename T::Base>& a) {
  Fe<T> r;
  memcpy(r.l, a.l, sizeof(r.l));
  return r;
}

template <class T>
static void t_mul(Fe<T>& r, const Fe<T>& a, const Fe<T>& b) {
  Site& s = site("mul", mul_bound<T>());
  check_mul_in(s, "mul", a, b);
  Fe<typename T::Base> rb;
  fe_mul<typename T::Base>(rb, down(a), down(b));
  r = up<T>(rb);
  check_mul_out(s, "mul", r);
}
template <class T>
static void t_sqr(Fe<T>& r, const Fe<T>& a) {
  Site& s = site("sqr", mul_bound<T>());
  check_mul_in(s, "sqr", a, a);
  Fe<typename T::Base> rb;
  fe_sqr<typename T::Base>(rb, down(a));
  r = up<T>(rb);
  check_mul_out(s, "sqr", r);
}
template <class T>
static void t_reduce_small(Fe<T>& a) {
  Site& s = site("reduce_small", 16);
  note_in(s, a);
  if (!within(a, 16, 1)) violation(s, "reduce_small", "input not in |v| < 16p", (double)value_over_p(a));
  const Fe<T> in = a;
  Fe<typename T::Base> b = down(a);
  fe_reduce_small<typename T::Base>(b);
  a = up<T>(b);
  check_reduced(s, "reduce_small", in, a);
}
template <class T>
static void t_store(uint32_t* w, const Fe<T>& a) {
  Site& s = site("store", 16);
  note_in(s, a);
  if (!within(a, 16, 1)) violation(s, "store", "input not in |v| < 16p", (double)value_over_p(a));
  fe_store<typename T::Base>(w, down(a));
  Fe<T> r;
  fe_unpack<T>(r, w);
  check_reduced(s, "store", a, r);
}
template <class T>
static void t_store_mulout(uint32_t* w, const Fe<T>& a) {
  Site& s = site("store_mulout", 1.5);
  note_in(s, a);
  if (!(cmp_kp(a, 1, 2) < 0 && cmp_kp(a, -3, 2) > 0))
    violation(s, "store_mulout", "input not a mul output: (-1.5p, 0.5p)", (double)value_over_p(a));
  fe_store_mulout<typename T::Base>(w, down(a));
  Fe<T> r;
  fe_unpack<T>(r, w);
  check_reduced(s, "store_mulout", a, r);
}
template <class T>
static bool t_is_zero(const Fe<T>& a) {
  Site& s = site("is_zero", 16);
  note_in(s, a);
  if (!within(a, 16, 1)) violation(s, "is_zero", "input not in |v| < 16p", (double)value_over_p(a));
  const bool z = fe_is_zero<typename T::Base>(down(a));
  if (z != is_multiple(a, 15)) violation(s, "is_zero", "wrong answer", (double)value_over_p(a));
  return z;
}

#define MSMZ_TRACE_FIELD(T)                                                                                  \
  template <> inline void fe_mul<T>(Fe<T> & r, const Fe<T>& a, const Fe<T>& b) { t_mul<T>(r, a, b); }    \
  template <> inline void fe_sqr<T>(Fe<T> & r, const Fe<T>& a) { t_sqr<T>(r, a); }                        \
  template <> inline void fe_reduce_small<T>(Fe<T> & a) { t_reduce_small<T>(a); }                         \
  template <> inline void fe_store<T>(uint32_t * w, const Fe<T>& a) { t_store<T>(w, a); }                 \
  template <> inline void fe_store_mulout<T>(uint32_t * w, const Fe<T>& a) { t_store_mulout<T>(w, a); }   \
  template <> inline bool fe_is_zero<T>(const Fe<T>& a) { return t_is_zero<T>(a); }

using TBls377 = Traced<Bls377Fp>;
using TBls381 = Traced<Bls381Fp>;
using TPallas = Traced<PallasFp>;
using TEd377 = Traced<Ed377Fp>;
MSMZ_TRACE_FIELD(TBls377)
MSMZ_TRACE_FIELD(TBls381)
MSMZ_TRACE_FIELD(TPallas)
MSMZ_TRACE_FIELD(TEd377)

}  // namespace msmz

using namespace msmz;

// ------------------------------------------------------------------------------------------------ I/O
template <class F>
static void read_fe(Fe<F>& r, std::istream& in) {
  std::string t;
  in >> t;
  if (!t.empty() && t[0] == 'L') {
    size_t pos = 1;
    for (int j = 0; j < F::N; j++) {
      size_t used = 0;
      r.l[j] = (int32_t)std::stol(t.substr(pos), &used);
      pos += used + 1;
    }
    return;
  }
  uint32_t w[F::NW];
  std::string s(F::NW * 8 > t.size() ? F::NW * 8 - t.size() : 0, '0');
  s += t;
  for (int i = 0; i < F::NW; i++) w[i] = (uint32_t)strtoul(s.substr((F::NW - 1 - i) * 8, 8).c_str(), nullptr, 16);
  fe_unpack<F>(r, w);
}

static std::string hex_words(const uint32_t* w, int nw) {
  std::string s;
  char b[9];
  for (int i = nw - 1; i >= 0; i--) {
    snprintf(b, sizeof b, "%08x", w[i]);
    s += b;
  }
  return s;
}

template <class F>
static std::string affine_w(const Xyzz<F>& p) {
  set_scope("xyzz_to_affine_canon");
  uint32_t w[2 * F::NW];
  if (xyzz_to_affine_canon<F>(w, p)) return "INF";
  return hex_words(w, F::NW) + ":" + hex_words(w + F::NW, F::NW);
}
template <class F>
static std::string affine_te(const TeExt<F>& p) {
  set_scope("te_to_affine_canon");
  uint32_t w[2 * F::NW];
  te_to_affine_canon<F>(w, p);
  return hex_words(w, F::NW) + ":" + hex_words(w + F::NW, F::NW);
}

template <class F>
static void read_xyzz(Xyzz<F>& p, std::istream& in) {
  read_fe(p.X, in);
  read_fe(p.Y, in);
  read_fe(p.ZZ, in);
  read_fe(p.ZZZ, in);
}
template <class F>
static void read_te(TeExt<F>& p, std::istream& in) {
  read_fe(p.X, in);
  read_fe(p.Y, in);
  read_fe(p.Z, in);
  read_fe(p.T, in);
}
// an affine record as load_affine hands it to the formulas: y negated in registers when `neg`
template <class F>
static void read_affine(Affine<F>& a, uint32_t neg, std::istream& in) {
  Fe<F> y;
  read_fe(a.x, in);
  read_fe(y, in);
  fe_cneg(a.y, y, neg);
}
template <class F>
static void read_niels(TeNiels<F>& n, std::istream& in) {
  read_fe(n.ym, in);
  read_fe(n.yp, in);
  read_fe(n.kt, in);
}

// a memory round trip of every coordinate (what the kernels do between launches)
template <class F, class P>
static void store_load(P& p) {
  set_scope("store_accumulator");
  Fe<F>* c = reinterpret_cast<Fe<F>*>(&p);
  for (int i = 0; i < 4; i++) {
    uint32_t w[F::NW];
    fe_store<F>(w, c[i]);
    fe_unpack<F>(c[i], w);
  }
}

// ------------------------------------------------------------------------------------------------ commands
template <class F>
constexpr bool kTe = std::is_same<typename F::Base, Ed377Fp>::value;   // the twisted-Edwards curve's field

template <class F>
static std::string run(const std::string& op, std::istream& in) {
  constexpr int N = F::N, NW = F::NW;
  if (op == "fl") {   // fl OP a b : field_limbs_op (the device hook's code) -> raw limbs, canonical value
    int fop;
    Fe<F> a, b;
    in >> fop;
    read_fe(a, in);
    read_fe(b, in);
    set_scope("field_limbs");
    int32_t raw[N];
    uint32_t canon[NW];
    if (fop == TFL_INVERSE_WAVE) fop = TFL_INVERSE;   // same result as the per-lane routine
    if (!field_limbs_op<F>(fop, a, b, raw, canon)) return "ERR";
    std::string s;
    for (int j = 0; j < N; j++) s += (j ? "," : "") + std::to_string(raw[j]);
    return s + " " + hex_words(canon, NW);
  }
  if (op == "wadd" || op == "wdbl") {
    Xyzz<F> p, q, r;
    read_xyzz(p, in);
    if (op == "wadd") {
      read_xyzz(q, in);
      set_scope("xyzz_add");
      xyzz_add(r, p, q);
    } else {
      set_scope("xyzz_dbl");
      xyzz_dbl(r, p);
    }
    return affine_w(r);
  }
  if (op == "wmadd") {   // wmadd X Y ZZ ZZZ ax ay neg inf
    Xyzz<F> p, r;
    Affine<F> a;
    uint32_t neg, inf;
    read_xyzz(p, in);
    Fe<F> x, y;
    read_fe(x, in);
    read_fe(y, in);
    in >> neg >> inf;
    a.x = x;
    fe_cneg(a.y, y, neg);
    set_scope("xyzz_madd");
    xyzz_madd(r, p, a, inf != 0);
    return affine_w(r);
  }
  if (op == "wmdbl") {   // wmdbl ax ay neg
    Affine<F> a;
    Fe<F> x, y;
    uint32_t neg;
    read_fe(x, in);
    read_fe(y, in);
    in >> neg;
    a.x = x;
    fe_cneg(a.y, y, neg);
    Xyzz<F> r;
    set_scope("xyzz_mdbl");
    xyzz_mdbl(r, a);
    return affine_w(r);
  }
  if constexpr (kTe<F>) {
  if (op == "tadd") {
    TeExt<F> p, q, r;
    read_te(p, in);
    read_te(q, in);
    set_scope("te_add");
    te_add(r, p, q);
    return affine_te(r);
  }
  if (op == "tmadd") {   // tmadd X Y Z T ym yp kt neg
    TeExt<F> p, r;
    TeNiels<F> n;
    uint32_t neg;
    read_te(p, in);
    read_niels(n, in);
    in >> neg;
    set_scope("te_madd");
    te_madd(r, p, n, neg);
    return affine_te(r);
  }
  }
  if (op == "inv") {
    Fe<F> a, r;
    read_fe(a, in);
    set_scope("fe_inverse");
    if (!fe_inverse(r, a)) return "ZERO";
    uint32_t w[NW];
    fe_to_canon_words<F>(w, r);
    return hex_words(w, NW);
  }
  // chains: ops string over two accumulators A, B and nb input points; output = A at every 'p'
  //   m / n : A = A + (+-)point[j], j cycling      a : A = A + B      b : B = B + A
  //   d : A = 2A (xyzz_dbl / te_add(A, A))          e : A = A + A through the addition formula
  //   s : A through memory (fe_store + fe_unpack of every coordinate)
  if (op == "wchain" || op == "tchain") {
    const bool te = op == "tchain";
    std::string ops;
    int nb;
    in >> ops;
    Xyzz<F> A, B, R;
    TeExt<F> TA, TB, TR;
    if (te != kTe<F>) return "ERR";
    if (te) {
      read_te(TA, in);
      read_te(TB, in);
    } else {
      read_xyzz(A, in);
      read_xyzz(B, in);
    }
    in >> nb;
    std::vector<Affine<F>> pts(nb);
    std::vector<TeNiels<F>> niels(nb);
    for (int i = 0; i < nb; i++) {
      if (te) read_niels(niels[i], in); else read_affine(pts[i], 0, in);
    }
    std::string out;
    int j = 0;
    for (char c : ops) {
      if constexpr (kTe<F>) {
        switch (c) {
          case 'm': case 'n': set_scope("te_madd"); te_madd(TR, TA, niels[j++ % nb], c == 'n'); TA = TR; break;
          case 'a': set_scope("te_add"); te_add(TR, TA, TB); TA = TR; break;
          case 'b': set_scope("te_add"); te_add(TR, TB, TA); TB = TR; break;
          case 'd': case 'e': set_scope("te_add"); te_add(TR, TA, TA); TA = TR; break;
          case 's': store_load<F>(TA); break;
          case 'p': out += (out.empty() ? "" : " ") + affine_te(TA); break;
          default: return "ERR";
        }
      } else {
        switch (c) {
          case 'm': case 'n': {
            Affine<F> a = pts[j++ % nb];
            fe_cneg(a.y, a.y, c == 'n');
            set_scope("xyzz_madd");
            xyzz_madd(R, A, a, false);
            A = R;
            break;
          }
          case 'a': set_scope("xyzz_add"); xyzz_add(R, A, B); A = R; break;
          case 'b': set_scope("xyzz_add"); xyzz_add(R, B, A); B = R; break;
          case 'd': set_scope("xyzz_dbl"); xyzz_dbl(R, A); A = R; break;
          case 'e': set_scope("xyzz_add"); xyzz_add(R, A, A); A = R; break;
          case 's': store_load<F>(A); break;
          case 'p': out += (out.empty() ? "" : " ") + affine_w(A); break;
          default: return "ERR";
        }
      }
    }
    return out;
  }
  return "ERR";
}

static void report() {
  fprintf(stderr, "%-8s %-44s %9s %10s %7s %10s %9s %21s %5s\n", "field", "call site", "calls", "max|v|/p", "bound",
          "max limb", "prod", "output/p", "viol");
  for (auto& kv : g_sites) {
    const Site& s = kv.second;
    const size_t sp = kv.first.find(' ');
    fprintf(stderr, "%-8s %-44s %9ld %10.4f %7.1f %8.2f b %7.2f b [%+9.4f, %+9.4f] %5ld\n", kv.first.substr(0, sp).c_str(),
            kv.first.substr(sp + 1).c_str(), s.calls, s.v_in, s.v_bound, s.limb_in, s.prod, s.out_lo, s.out_hi, s.viol);
  }
  fprintf(stderr, "MSMZ_FE_ILP=%d VIOLATIONS %ld\n", MSMZ_FE_ILP, g_violations);
}

int main() {
  std::string field, op;
  while (std::cin >> field >> op) {
    g_field = field;
    std::string r;
    if (field == "bls377") r = run<TBls377>(op, std::cin);
    else if (field == "bls381") r = run<TBls381>(op, std::cin);
    else if (field == "pallas") r = run<TPallas>(op, std::cin);
    else if (field == "ed377") r = run<TEd377>(op, std::cin);
    else r = "ERR";
    printf("%s\n", r.c_str());
  }
  report();
  return g_violations ? 1 : 0;
}

// The regime of every case of the MSM sweep (tests/msm_sweep_util.py), predicted on a CPU: this program includes the
// planner (msm_zprize_amd/csrc/plan.h) and nothing else of the engine, replays the few host decisions engine.h takes
// around it (which n the plan is made for, the GLV default, batch or problem by problem, the first index-range pass, the
// length classes of a segmented call, the parameters of a precomputed set) and prints what the planner decides.
//
// stdin: one case per line, 20 integers
//   id curve n pts_n pre_n glv c sbits shape B factor basic reduce_affine pass_entries want_sub glv_bits len0 len1 len2 has_endo
//   shape 0 = one MSM, 1 = a batch of B, 2 = three segments of len0..2, 3 = a precomputed set of `factor` over pre_n
//   points (n, pts_n: the share of the engine whose plan the call's log reports; one engine: n, the set's size)
//   want_sub 1 = pick the lowered batch limit that cuts the batch into sub-batches of two
// stdout: one line of key=value words per case.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../msm_zprize_amd/csrc/constants_gen.h"
#include "../../msm_zprize_amd/csrc/plan.h"
using namespace msmz;

struct Case {
  long long id, curve, n, pts_n, pre_n, glv, c, sbits, shape, B, factor, basic, reduce_affine, pass_entries, want_sub,
      glv_bits, len[3], has_endo;
};

// which branch of Planner::choose_window gives the window size (a label; the size itself is the planner's)
template <class Fr>
static const char* window_rule(const Planner<Fr>& pr, bool glv, uint32_t M, int b, bool tree_rounds, int c_user) {
  if (c_user > 0) return "user";
  if (M < (1u << 18)) return "model";
  if (tree_rounds && !glv && b < Fr::BITS) return "bounded17";
  const int c0 = tree_rounds ? (glv ? 16 : 17) : default_window(M);
  Planner<Fr> p2 = pr;
  return p2.choose_window(glv, M, b, tree_rounds) < c0 ? "stepped" : "fixed";
}

template <class Fr>
static void predict(const Case& cs) {
  Planner<Fr> pr;
  pr.k.glv_bits_assumed = (int)cs.glv_bits;
  msmz_opts opt;
  memset(&opt, 0, sizeof(opt));
  opt.c = (int)cs.c;
  opt.glv = (int)cs.glv;
  opt.reserved[0] = (int)cs.reduce_affine;
  opt.reserved[1] = pr.bound((int)cs.sbits);
  printf("id=%lld", cs.id);
  uint32_t fac = 1;
  const char* rule = nullptr;
  if (cs.shape == 3) {
    int pc = 0, pglv = 0, pk = 0, psb = 0;
    uint32_t copies = 0;
    msmz_opts po = opt;
    po.reserved[0] = 0;
    const int st = pr.precompute_params((uint64_t)cs.pre_n, &po, (uint32_t)cs.factor, &pc, &pglv, &copies, &pk, &psb);
    printf(" pre_status=%d", st);
    if (st) {
      printf(" status=%d\n", st);
      return;
    }
    printf(" pre_c=%d pre_glv=%d pre_copies=%u pre_K=%d pre_sbits=%d", pc, pglv, copies, pk, psb);
    if (cs.c > 0) rule = "user";
    else {
      const uint32_t M = (uint32_t)(pglv ? 2 * cs.pre_n : cs.pre_n);
      const uint32_t F = cs.factor == 0 ? 1024u : (uint32_t)cs.factor;
      const int b0 = pr.scalar_bits(pglv != 0, 0, psb);
      const bool b17 = !pglv && M >= (1u << 16) && F >= (uint32_t)pr.geometry(17, false, M, b0, F).K && pr.pre_fits(17, false, M, b0, F);
      rule = b17 ? "pre17" : "pre_model";
    }
    opt.c = pc;
    opt.glv = pglv;
    opt.reserved[1] = psb;
    fac = copies;
  }
  // the problems the first pipeline is decided for: a batch, or the first length class of a segmented call
  uint64_t n = (uint64_t)cs.n;
  uint32_t cand = cs.shape == 1 ? (uint32_t)cs.B : 1;
  if (cs.shape == 2) {
    const uint64_t lens[3] = {(uint64_t)cs.len[0], (uint64_t)cs.len[1], (uint64_t)cs.len[2]};
    std::vector<uint32_t> order, starts;
    segment_classes(lens, 3, &order, &starts);
    n = 0;
    for (uint32_t j = starts[0]; j < starts[1]; j++) n = lens[order[j]] > n ? lens[order[j]] : n;
    cand = starts[1] - starts[0];
    printf(" classes=%zu first_class=%u", starts.size() - 1, cand);
    if (cand == 1) n = lens[order[0]];
  }
  if (opt.glv < 0) opt.glv = cs.has_endo && pr.default_glv(n, opt.reserved[1]) ? 1 : 0;
  const bool glv = opt.glv != 0;
  const bool basic = cs.basic != 0;
  const uint64_t pass = cs.pass_entries ? (uint64_t)cs.pass_entries : kMaxEntriesPerPass;
  const uint64_t per_pass = (glv && !basic) ? pass / 2 : pass;   // (engine.h shape(): twisted Edwards never splits)
  const bool want_2d = opt.reserved[0] != 1;
  const bool may_batch = !basic && want_2d && n <= per_pass && cand > 1;
  uint64_t cap = 0;
  if (cs.want_sub && may_batch) {
    // entries of two problems planned as a pair, and one problem's short of a third
    Plan p2;
    if (pr.make_plan(p2, n, glv, opt, (uint32_t)cs.pts_n, true, 0, true, 2, fac) == MSMZ_OK) {
      cap = 3ull * p2.K * p2.M - 1;
      pr.k.batch_entries = cap;
    }
  }
  uint32_t bs = may_batch ? pr.batch_size(n, opt, (uint32_t)cs.pts_n, fac, cand) : 1;
  Plan pl;
  int st = MSMZ_OK;
  bool per_problem = cand > 1 && bs <= 1;
  if (bs > 1) {
    st = pr.make_plan(pl, n, glv, opt, (uint32_t)cs.pts_n, true, 0, want_2d, bs, fac);
    if (st == MSMZ_OK && !pr.sort_layout(pl).two_level) {
      per_problem = true;
      bs = 1;
    }
  }
  uint64_t passes = 0;
  if (bs <= 1) {
    const uint64_t cnt = n < per_pass ? n : per_pass;
    passes = (n + per_pass - 1) / per_pass;
    if (basic) st = glv ? MSMZ_ERR_UNSUPPORTED : pr.make_plan(pl, cnt, false, opt, (uint32_t)cs.pts_n, false);
    else st = pr.make_plan(pl, cnt, glv, opt, (uint32_t)cs.pts_n, true, 0, want_2d, 1, fac);
  }
  printf(" status=%d", st);
  if (st) {
    printf("\n");
    return;
  }
  const SortLayout sl = pr.sort_layout(pl);
  const PlanChunks pc = pr.plan_chunks(pl);
  if (!rule) rule = window_rule(pr, glv, pl.M, pl.b, !basic, (int)cs.c);
  printf(" n_plan=%u c=%d K=%d Keff=%d spread=%d fold_shift=%d F=%u b=%d glv=%d M=%u L=%u two_level=%d cspec=%d fb=%d fbt=%d"
         " chunk=%u top_split=%d bs=%u per_problem=%d passes=%llu cap=%llu rule=%s top_range=%u",
         pl.n, pl.c, pl.K, pl.Keff, pl.spread, pl.fold_shift, Planner<Fr>::set_windows(pl), pl.b, pl.glv ? 1 : 0, pl.M, pl.L,
         sl.two_level ? 1 : 0, sl.cspec, sl.fits ? sl.geom.fb : -1, sl.fits ? sl.geom.fbt : -1, pc.chunk,
         pc.nb_main != pl.nb * pl.nprob ? 1 : 0, bs, per_problem ? 1 : 0, (unsigned long long)passes, (unsigned long long)cap,
         rule, pl.top_range);
  // the plan of the redo, when a GLV half is longer than the assumed length (msmz_test_set_glv_bits)
  if (glv && cs.glv_bits) {
    Plan r;
    if (pr.make_plan(r, pl.n, true, opt, (uint32_t)cs.pts_n, true, 1, want_2d, pl.nprob, fac) == MSMZ_OK)
      printf(" redo_c=%d redo_K=%d", r.c, r.K);
  }
  printf("\n");
}

int main() {
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    Case c;
    if (sscanf(line, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &c.id,
               &c.curve, &c.n, &c.pts_n, &c.pre_n, &c.glv, &c.c, &c.sbits, &c.shape, &c.B, &c.factor, &c.basic,
               &c.reduce_affine, &c.pass_entries, &c.want_sub, &c.glv_bits, &c.len[0], &c.len[1], &c.len[2], &c.has_endo) != 20) {
      fprintf(stderr, "bad line: %s", line);
      return 2;
    }
    switch (c.curve) {
      case MSMZ_BLS12_377_G1: predict<Bls377Fr>(c); break;
      case MSMZ_PALLAS: predict<PallasFr>(c); break;
      case MSMZ_BLS12_381_G1: predict<Bls381Fr>(c); break;
      case MSMZ_ED_ON_BLS12_377: predict<Ed377Fr>(c); break;
      default: return 2;
    }
  }
  return 0;
}

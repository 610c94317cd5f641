// The bucket reduction as one host-side stage: the buckets an MSM's accumulation left -> one result per window (2-D: two
// per bucket set).  BucketReduce owns what only the reduction touches -- the two pairs of level buffers it ping-pongs
// between, the window results, the per-bucket sums and the descriptors of the batched-affine first level -- and which
// kernel a level runs; its callers (engine.h, test_hooks.h) hand it the stream and a description of the buckets, and
// read final().  It holds nothing of the engine.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/msmz.h"
#include "batch_add.h"
#include "kernels.h"
#include "plan.h"
#include "store.h"

namespace msmz {

// Which kernel a level of the bucket reduction runs; none changes a result.  The engine holds one, constant, which the
// MSM paths pass to the reduction; a test hook passes a copy with its caller's values.
struct ReduceKnobs {
  uint32_t tail_n = (uint32_t)env_int("MSMZ_TAIL_N", REDUCE_TAIL_N);   // entries per window at which k_reduce_tail takes over
  uint32_t quad16_max = (uint32_t)env_int("MSMZ_QUAD16", 8192);        // levels of at most this many groups: k_reduce_quad16
  uint32_t pairsum_x4_max = (uint32_t)env_int("MSMZ_PAIRSUM_X4", 16384);   // pair-sum levels of at most this many
                                                                           // additions use DPP quads
  // levels of at most this many groups (and within quad16_max) run the row form, k_reduce_rows: one wave per addition.
  // It wins while its waves stand alone on their SIMDs -- 16-20 us a level up to 480 groups against 45-47 us for
  // k_reduce_quad16, 55 against 47 us at 1920 (profiles/reduce_rows_ab.txt) -- and a launch per level is then shorter
  // than a level inside k_reduce_tail, so such levels run as launches below tail_n too, down to one entry.
  uint32_t rows_max = (uint32_t)env_int("MSMZ_ROWS_MAX", 512);
};

// The buckets the 2-D reduction sums, in the three forms an accumulation leaves them in.  The memory stays the caller's.
struct BucketSource {
  const uint32_t* recs;     // slot records (locations) or accumulator records
  const uint32_t* points;   // locations: the resident point set their LOC_ORIG words name
  const uint4* bfin;        // locations: what the tree rounds left of each bucket (plan_kernels.h); else null
  const uint32_t* cscan;    // chunk accumulators: bucket g = recs[cscan[g] .. cscan[g + 1]); null: recs[g]

  // the affine bucket sums of the tree rounds (Weierstrass only)
  static BucketSource locations(const uint32_t* slots, const uint32_t* pts, const uint4* bfin) { return {slots, pts, bfin, nullptr}; }
  // msmBasic: the chunk accumulators of k_bucket_accumulate and their ranges per bucket
  static BucketSource chunks(const uint32_t* accs, const uint32_t* cscan) { return {accs, nullptr, nullptr, cscan}; }
  // one accumulator per bucket, in bucket order (BucketReduce::bucket_sums)
  static BucketSource per_bucket(const uint32_t* accs) { return {accs, nullptr, nullptr, nullptr}; }
};

template <class Cfg>
class BucketReduce {
  using F = typename Cfg::F;
  using P = typename Cfg::P;
  static constexpr int AW = P::ACC_WORDS;

 public:
  // Two-dimensional bucket reduction (reduce2d_kernels.h): line sums, then the weighted sums over H lines of g.nprob
  // problems with the upper-level kernels.  Leaves result 2 kw (rows) / 2 kw + 1 (columns) of bucket set kw in final().
  // g: the planner's geometry (Planner::r2_geom); rk: which kernel a level runs.
  int run_2d(const R2Geom& g, const ReduceKnobs& rk, const BucketSource& src, hipStream_t stream) {
    const uint32_t* lines;
    if (int st = line_sums(g, rk, src, stream, &lines)) return st;
    return weighted_sums(g, rk, stream);
  }

  // first half: the partial sums of every line's chunks, then their pair sums; *lines = the g.nprob * g.H line sums
  // (until weighted_sums reuses them)
  int line_sums(const R2Geom& g, const ReduceKnobs& rk, const BucketSource& src, hipStream_t stream,
                const uint32_t** lines) {
    const uint32_t n_lines = g.nprob * g.H;
    const uint32_t total = n_lines * g.NC;
    int st;
    // ping-pong between the rows of the two level pairs; the C inputs of the first level are filled by weighted_sums
    if ((st = rows_room(0, total)) || (st = rows_room(1, total))) return st;
    if (src.bfin) {
      if constexpr (!Cfg::TE)
        hipLaunchKernelGGL((k_reduce2d_partial<F>), dim3((total + 127) / 128), dim3(128), 0, stream, rows(0), src.recs,
                           src.points, src.bfin, g, total);
    } else {
      hipLaunchKernelGGL((k_reduce2d_partial_acc<P>), dim3((total + 127) / 128), dim3(128), 0, stream, rows(0), src.recs,
                         src.cscan, g, total);
    }
    cur_ = 0;
    for (uint32_t n = total / 2; n >= n_lines && g.NC > 1; n /= 2) {
      if (n <= rk.pairsum_x4_max) {
        hipLaunchKernelGGL((k_pairsum_x4<P>), dim3((n * 4 + 63) / 64), dim3(64), 0, stream, rows(cur_ ^ 1), rows(cur_), n);
      } else {
        hipLaunchKernelGGL((k_pairsum<P>), dim3((n + 127) / 128), dim3(128), 0, stream, rows(cur_ ^ 1), rows(cur_), n);
      }
      cur_ ^= 1;
      if (n == n_lines) break;
    }
    *lines = rows(cur_);
    return MSMZ_OK;
  }

  // second half, the upper levels: rows = the line sums line_sums left (weight unit 1), C = neutral
  int weighted_sums(const R2Geom& g, const ReduceKnobs& rk, hipStream_t stream) {
    const uint32_t n_lines = g.nprob * g.H;
    if (int st = carry_room(cur_, n_lines)) return st;
    hipLaunchKernelGGL((k_fill_neutral<P>), dim3((n_lines + 255) / 256), dim3(256), 0, stream, carry(cur_), n_lines);
    if (int st = levels(rk, g.H, g.nprob, stream)) return st;
    MSMZ_HIP(hipGetLastError());
    return MSMZ_OK;
  }

  // The inputs of levels() for callers that fill them themselves: room for n accumulator records each, rows and C.
  int level_inputs(size_t n, uint32_t** rows_out, uint32_t** c_out) {
    int st;
    if ((st = rows_room(0, n)) || (st = carry_room(0, n))) return st;
    cur_ = 0;
    *rows_out = rows(0);
    *c_out = carry(0);
    return MSMZ_OK;
  }

  // reduce levels on the accumulator records of the current level pair (rows, C): nprob problems of n_in entries; ends
  // with one entry per problem in final()
  int levels(const ReduceKnobs& rk, uint32_t n_in, uint32_t nprob, hipStream_t stream) {
    int st;
    const uint32_t rows_max = rk.rows_max < rk.quad16_max ? rk.rows_max : rk.quad16_max;
    while (n_in > rk.tail_n || (n_in > 1 && (uint64_t)nprob * ((n_in + 3) / 4) <= rows_max)) {
      const uint32_t S = 4;   // quads handle short tails too
      const uint32_t g2 = (n_in + S - 1) / S;
      const int nxt = cur_ ^ 1;
      if ((st = rows_room(nxt, (size_t)nprob * g2)) || (st = carry_room(nxt, (size_t)nprob * g2))) return st;
      const uint32_t total = nprob * g2;
      if (total <= rows_max) {
        // smallest levels: every wave alone on its SIMD, one wave per addition
        hipLaunchKernelGGL((k_reduce_rows<P>), dim3(total), dim3(256), 0, stream, rows(nxt), carry(nxt), rows(cur_),
                           carry(cur_), n_in, g2, total);
      } else if (total <= rk.quad16_max) {
        // small level: latency-bound, one DPP quad per addition
        hipLaunchKernelGGL((k_reduce_quad16<P>), dim3((total * 16 + 63) / 64), dim3(64), 0, stream, rows(nxt), carry(nxt),
                           rows(cur_), carry(cur_), n_in, g2, total);
      } else {
        hipLaunchKernelGGL((k_reduce_quad<P>), dim3((total * 4 + 63) / 64), dim3(64), 0, stream, rows(nxt), carry(nxt),
                           rows(cur_), carry(cur_), n_in, g2, total);
      }
      n_in = g2;
      cur_ = nxt;
    }
    // the last levels (<= REDUCE_TAIL_N entries per window) in ONE launch, one workgroup per window; leaves the
    // window sums in final_
    const int nxt = cur_ ^ 1;
    if ((st = rows_room(nxt, (size_t)nprob * n_in)) || (st = carry_room(nxt, (size_t)nprob * n_in))) return st;
    if ((st = final_.ensure((size_t)nprob * AW * 4))) return st;
    hipLaunchKernelGGL((k_reduce_tail<P>), dim3(nprob), dim3(REDUCE_TAIL_T), 0, stream, rows(cur_), carry(cur_), rows(nxt),
                       carry(nxt), final_.as<uint32_t>(), n_in, n_in);
    return MSMZ_OK;
  }

  // *sums = one accumulator per bucket g < nb: the sum of the chunk accumulators of `chunks` (BucketSource::chunks)
  int bucket_sums(BucketSource chunks, uint32_t nb, hipStream_t stream, BucketSource* sums) {
    if (int st = bsum_.ensure((size_t)nb * AW * 4)) return st;
    hipLaunchKernelGGL((k_bucket_sums<P>), dim3((nb + 127) / 128), dim3(128), 0, stream, bsum_.as<uint32_t>(), chunks.recs,
                       chunks.cscan, nb);
    *sums = BucketSource::per_bucket(bsum_.as<uint32_t>());
    return MSMZ_OK;
  }

  // Batched-affine first level of the bucket reduction (reduce_affine.h; Weierstrass only): S - 1
  // chain steps and a short pair tree, every launch over Keff * groups (x pairs per group) additions of `adder`, results
  // behind the tree rounds' `tree_pairs` records of its slot array (slot_bytes long: sized for this in advance, its
  // contents must survive).  src: the tree rounds' buckets (BucketSource::locations, one location per bucket).  Leaves
  // the scaled (row, tri) XYZZ records as the inputs of levels(): Keff problems of `groups` entries.
  int first_affine(const Plan& pl, uint32_t S, uint32_t groups, uint64_t tree_pairs, const BatchAdder<Cfg>& adder,
                   size_t slot_bytes, const BucketSource& src, MsmMeta* d_meta) {
    F2Geom g;
    memset(&g, 0, sizeof(g));
    g.L = pl.L;
    g.S = S;
    g.groups = groups;
    g.NG = (uint32_t)pl.Keff * groups;
    g.inf_slot = (uint32_t)((tree_pairs + 63) / 64 * 64);
    g.out0 = g.inf_slot + 64;
    uint32_t n_launch = 0, dsum = 0, osum = 0;
    auto add_launch = [&](uint32_t pairs_per_group) {
      g.ppg[n_launch] = pairs_per_group;
      g.desc_off[n_launch] = dsum;
      g.out_off[n_launch] = osum;
      dsum += g.NG * pairs_per_group;
      osum += g.NG * pairs_per_group;
      n_launch++;
    };
    for (uint32_t step = 1; step < S; step++) add_launch(1);
    for (uint32_t n = S - 1; n > 1; n = n / 2 + (n & 1)) add_launch(n / 2);
    g.n_launches = n_launch;
    g.desc_off[n_launch] = dsum;   // (row, tri) locations of every group
    dsum += g.NG;
    if ((uint64_t)g.out0 + osum + 64 >= (1ull << 30)) return MSMZ_ERR_ARG;
    int st;
    uint32_t *d_rows, *d_tri;
    if ((st = level_inputs((size_t)g.NG, &d_rows, &d_tri)) || (st = f2desc_.ensure((size_t)dsum * 8))) return st;
    if (((size_t)g.out0 + osum + 64) * SlotFmt<F>::WORDS * 4 > slot_bytes) return MSMZ_ERR_HIP;
    MSMZ_HIP(hipMemsetAsync(adder.slots + slot_words<F>(g.inf_slot), 0, (size_t)64 * SlotFmt<F>::WORDS * 4, adder.stream));
    hipLaunchKernelGGL(k_reduce_affine_desc, dim3((g.NG + 255) / 256), dim3(256), 0, adder.stream, f2desc_.as<uint2>(),
                       src.bfin, g);
    for (uint32_t i = 0; i < n_launch; i++)
      adder.launch(g.NG * g.ppg[i], true, src.points, f2desc_.as<uint2>() + g.desc_off[i], g.out0 + g.out_off[i], d_meta);
    if constexpr (!Cfg::TE)
      hipLaunchKernelGGL((k_reduce_affine_finish<F>), dim3((g.NG + 127) / 128), dim3(128), 0, adder.stream, d_rows, d_tri,
                         src.recs, src.points, f2desc_.as<uint2>() + g.desc_off[n_launch], src.bfin, g);
    MSMZ_HIP(hipGetLastError());
    return MSMZ_OK;
  }

  // the window results of the last levels() (run_2d, weighted_sums): one accumulator record per problem
  const uint32_t* final() const { return final_.as<uint32_t>(); }

  // f(buffer) for every device buffer of the stage: all scratch, undefined at the start of every reduction
  template <class Fn>
  void each_scratch(Fn f) {
    for (DevBuf& b : red_) f(b);
    f(final_), f(bsum_), f(f2desc_);
  }

 private:
  // level pair p in {0, 1}: the rows and the C (running-sum) records of a level; a level reads one pair and writes the other
  uint32_t* rows(int p) const { return red_[p * 2].as<uint32_t>(); }
  uint32_t* carry(int p) const { return red_[p * 2 + 1].as<uint32_t>(); }
  int rows_room(int p, size_t n) { return red_[p * 2].ensure(n * AW * 4); }   // ... with room for n records
  int carry_room(int p, size_t n) { return red_[p * 2 + 1].ensure(n * AW * 4); }

  DevBuf red_[4], final_, bsum_, f2desc_;
  int cur_ = 0;   // the level pair that holds the inputs of the next level (after line_sums: the line sums)
};

}  // namespace msmz

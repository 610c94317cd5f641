// One MSM call's run state, which the engine's phases (engine.h) and the sort stage (sort.h) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace msmz {

// Named events of an MSM's stages, created once per engine; a timed MSM records them in stream order.
struct StageEvents {
  hipEvent_t sort0, hist_end, scan_end, coarse_end, sort_end;   // sort: digits / histogram, scan, scatter
  hipEvent_t plan0, plan_end;                                    // plan (incl. its host round trip)
  hipEvent_t round_end[32];                                      // tree round r (recorded for non-empty rounds)
  hipEvent_t acc_end, red_end;                                   // accumulation, bucket reduction
  std::vector<hipEvent_t*> all() {
    std::vector<hipEvent_t*> v{&sort0, &hist_end, &scan_end, &coarse_end, &sort_end, &plan0, &plan_end, &acc_end, &red_end};
    for (hipEvent_t& e : round_end) v.push_back(&e);
    return v;
  }
};

// One MSM call's run state, beside its Plan (the planner's output): whether it is timed, its stage events, and the
// device totals fetch_meta reads back.  n_pairs: the additions of the accumulation (the tree rounds' pairs; msmBasic:
// the entries).
struct Run {
  bool timing = false;
  StageEvents ev{};
  uint32_t max_bucket = 0, n_entries = 0, rounds = 0;
  uint32_t round_pairs[32] = {}, round_base[32] = {};
  uint64_t n_pairs = 0;
  void mark(hipEvent_t e, hipStream_t stream) const {
    if (timing) (void)hipEventRecord(e, stream);
  }
};

}  // namespace msmz

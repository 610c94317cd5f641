// Host driver for the sub-batch split of the batched MSM (msm_zprize_amd/csrc/multi.h batch_split).
// stdin: lines "remaining entries_per_problem cap"; stdout: one sub-batch size per line.
#include <cstdio>

#include "../../msm_zprize_amd/csrc/multi.h"

int main() {
  unsigned long long r, e, cap;
  while (scanf("%llu %llu %llu", &r, &e, &cap) == 3) printf("%u\n", msmz::batch_split((uint32_t)r, e, cap));
  return 0;
}

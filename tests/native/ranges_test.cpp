// Host driver for the range predicates of msm_zprize_amd/csrc/ranges.h.
// stdin: lines "in first n len" or "ov a b n" (hex); stdout: 0 or 1 per line.
#include <cstdio>
#include <cstring>

#include "../../msm_zprize_amd/csrc/ranges.h"

int main() {
  char op[8];
  unsigned long long x, y, z;
  while (scanf("%7s %llx %llx %llx", op, &x, &y, &z) == 4) {
    if (!strcmp(op, "in")) printf("%d\n", msmz::in_range(x, y, z) ? 1 : 0);
    else if (!strcmp(op, "ov")) printf("%d\n", msmz::partial_overlap(x, y, z) ? 1 : 0);
    else return 1;
  }
  return 0;
}

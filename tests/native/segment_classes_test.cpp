// Host driver for the length classes of a segmented MSM (msm_zprize_amd/csrc/multi.h segment_classes).
// stdin: one case per line, its segment lengths separated by blanks; stdout per case: the line "order ..." and the line
// "starts ...".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../msm_zprize_amd/csrc/multi.h"

int main() {
  char line[1 << 16];
  while (fgets(line, sizeof line, stdin)) {
    std::vector<uint64_t> n;
    for (char* tok = strtok(line, " \t\n"); tok; tok = strtok(nullptr, " \t\n")) n.push_back(strtoull(tok, nullptr, 10));
    if (n.empty()) continue;
    std::vector<uint32_t> order, starts;
    msmz::segment_classes(n.data(), (uint32_t)n.size(), &order, &starts);
    printf("order");
    for (uint32_t v : order) printf(" %u", v);
    printf("\nstarts");
    for (uint32_t v : starts) printf(" %u", v);
    printf("\n");
  }
  return 0;
}

// node_cuts_check.cpp -- csrc/node_cuts.h on its own (no HIP; g++ -fsanitize=address,undefined): for every line
// "step0 n_steps n_segments form sum_steps" on stdin one line "cuts ... | redCuts ..." (tests/test_node_cuts.py)
#include <cstdio>

#include "../../sipnet_amd/csrc/node_cuts.h"

int main() {
  int step0, nSteps, nSeg, form, sumSteps;
  std::vector<int32_t> cuts, redCuts;
  while (scanf("%d %d %d %d %d", &step0, &nSteps, &nSeg, &form, &sumSteps) == 5) {
    sipnet::segmentCuts(step0, nSteps, nSeg, form, sumSteps, &cuts, &redCuts);
    for (int32_t c : cuts) printf("%d ", c);
    printf("|");
    for (int32_t c : redCuts) printf(" %d", c);
    printf("\n");
  }
  return 0;
}

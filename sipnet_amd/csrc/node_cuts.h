// node_cuts.h -- part of node.cpp: where a gathering run is cut into segments.  No HIP in it: it builds under g++ with the
// sanitizers on a box without a GPU (tests/c/node_cuts_check.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/sipnet_amd.h"

namespace sipnet {

// n_segments segments of the records [step0, step0 + n_steps): segment j is [cuts[j], cuts[j + 1]) relative to step0 and
// rows [redCuts[j], redCuts[j + 1]) of the reduced block (steps, or with SIPNET_GATHER_SUMS groups of sumSteps steps;
// redCuts ends at the number of rows of the run).  The planes are cut at whole 16-step tiles of the site plan where the
// segments are long enough for that, sums at whole groups.  The caller has checked 1 <= n_segments <= n_steps and, for
// sums, sumSteps > 0 and n_segments <= the number of groups.
inline void segmentCuts(int32_t step0, int32_t n_steps, int32_t n_segments, int32_t form, int32_t sumSteps,
                        std::vector<int32_t>* cuts, std::vector<int32_t>* redCuts) {
  const bool sums = form == SIPNET_GATHER_SUMS;
  const int32_t nGroups = sums ? (n_steps + sumSteps - 1) / sumSteps : n_steps;
  std::vector<int32_t>& c = *cuts;
  c.assign(n_segments + 1, 0);
  c[n_segments] = n_steps;
  for (int j = 1; j < n_segments; j++) {
    if (sums) {
      c[j] = (int32_t)((int64_t)nGroups * j / n_segments) * sumSteps;   // whole groups
      continue;
    }
    const int32_t raw = (int32_t)((int64_t)n_steps * j / n_segments);
    const int32_t tile = ((step0 + raw) & ~15) - step0;
    c[j] = tile > c[j - 1] ? tile : raw;
  }
  redCuts->assign(n_segments + 1, 0);
  for (int j = 0; j <= n_segments; j++) (*redCuts)[j] = sums ? (c[j] + sumSteps - 1) / sumSteps : c[j];
}

}  // namespace sipnet

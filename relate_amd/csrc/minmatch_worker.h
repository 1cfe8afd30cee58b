// minmatch_worker.h -- what the GPU tree builder's worker unit (minmatch_worker.hip) offers minmatch_builder.hip
#pragma once
#include <algorithm>
#include <cstdlib>

#include "minmatch_params.h"

namespace rl {
class BuildQueue;  // the workers of one device and tree size (with sample ages: another kernel, workers of their own)
BuildQueue *build_queue_of(int device, int N, bool ages);  // lives as long as the process; nullptr: no pinned memory
// Publishes the tree and returns when ITS worker says it is out (p.host_done, -1 until then): 0, or RL_EHIP.
int build_queue_run(BuildQueue *q, const MMParams &p);
int worker_layout(int N, bool ages);  // the L_* the worker kernel for trees of N leaves keeps its per-cluster state in
inline int env_int(const char *name, int fallback, int lo, int hi) {
  const char *e = getenv(name);
  return e ? std::max(lo, std::min(hi, atoi(e))) : fallback;
}
}  // namespace rl

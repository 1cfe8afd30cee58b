// copying.h -- CopyingMatrix: what copying.cpp, window.cpp and copying_kernels.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"

namespace rl {

struct CopyingParams {
  Layout lay;
  int N, S, waves;
  int nloc;                  // one workgroup per target of the window; the arrays below are indexed by t = n - k0
  const float *topology;     // the window's resident posterior rows (RepaintParams::topology)
  const int64_t *top_off;    // [nloc+1] row offsets into weights
  const int64_t *slab_base;  // [nloc] posterior row j of target t is topology row slab_base[t] + j
  const int32_t *row_lo, *row_hi;  // [nloc] the rows this launch reduces, [lo, hi): resident, and not reduced before
  const double *weights;     // [top_off[nloc]] Wt of every posterior row of the window
  double *C;                 // [nloc][N], added to
  int32_t *bad_row;          // [nloc] 1 + the first row with a weight whose sum is not finite and positive (else untouched)
};
hipError_t launch_copying(const CopyingParams &p, hipStream_t stream);

// Row weights of one target in one window (relate_amd.h, CopyingMatrix step 1): site[D] ascending, the window owns
// the SNPs [s_begin, s_end).  RL_ESTATE when a SNP has no row on one of its sides.
int copying_weights(const int32_t *site, int D, const double *rpos, int s_begin, int s_end, double *wt);
// Steps 2 and 3 on the host: rows [D][N] in donor order; c_row [N] is added to.  *bad_row: as CopyingParams::bad_row.
void copying_rows(const float *rows, const double *wt, int D, int N, double *c_row, int *bad_row);

}  // namespace rl

// copying.cpp -- CopyingMatrix, host side: the Li-Stephens coancestry ("chunk length") matrix of a painted chunk,
// C[n][j] = the number of SNPs recipient n is expected to copy from donor j (include/relate_amd.h has the definition).
//
// This file is the row weights (step 1), the host twin of the device's reduction (steps 2 and 3: the same partial
// sums, the same halving, product and sum rounded one after the other -- equal bits), the walk over the windows of a
// painted context and the stage behind `Relate --mode CopyingMatrix`.  The walk through the parts of ONE window is
// rl_window_copying (window.cpp), the kernel copying_kernels.hip.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "copying.h"

namespace rl {

int copying_weights(const int32_t *site, int D, const double *rpos, int s_begin, int s_end, double *wt) {
  for (int d = 0; d < D; d++) wt[d] = 0.0;
  if (D < 1 || site[0] > s_begin) {
    set_error("the posterior rows begin at SNP %d, behind the window's first SNP %d", D < 1 ? -1 : site[0], s_begin);
    return RL_ESTATE;
  }
  int p = 0;
  for (int s = s_begin; s < s_end; s++) {
    while (p + 1 < D && site[p + 1] <= s) p++;
    if (s == site[p]) {
      wt[p] += 1.0;
      continue;
    }
    if (p + 1 >= D) {
      set_error("SNP %d lies behind the last posterior row (SNP %d)", s, site[p]);
      return RL_ESTATE;
    }
    const double a = rpos[site[p]], b = rpos[site[p + 1]];
    double wl = 0.5, wr = 0.5;  // anc_builder.cpp:146-153
    if (a != b) {
      wl = (b - rpos[s]) / (b - a);
      wr = (rpos[s] - a) / (b - a);
    }
    wt[p] += wl;
    wt[p + 1] += wr;
  }
  return RL_OK;
}

void copying_rows(const float *rows, const double *wt, int D, int N, double *c_row, int *bad_row) {
#pragma clang fp contract(off)
  double x[256];
  for (int p = 0; p < D; p++) {
    if (wt[p] == 0.0) continue;
    const float *row = rows + (size_t)p * N;
    for (int t = 0; t < 256; t++) {  // partial t: the donors t, t + 256, ..., rising
      double s = 0.0;
      for (int j = t; j < N; j += 256) s += (double)row[j];
      x[t] = s;
    }
    for (int h = 128; h >= 1; h >>= 1)
      for (int t = 0; t < h; t++) x[t] += x[t + h];
    const double Z = x[0];
    if (!(Z > 0.0 && Z < __builtin_huge_val())) {
      if (bad_row && !*bad_row) *bad_row = p + 1;
      continue;
    }
    const double c = wt[p] / Z;
    for (int j = 0; j < N; j++) {
      const double prod = c * (double)row[j];
      c_row[j] = c_row[j] + prod;
    }
  }
}

}  // namespace rl

using namespace rl;

extern "C" {

int rl_copying_weights_host(const int *site, int D, const double *rpos, int s_begin, int s_end, double *weights) {
  if (!site || !rpos || !weights || D < 1 || s_begin < 0 || s_end < s_begin) {
    set_error("rl_copying_weights_host: bad arguments (D=%d, SNPs [%d, %d))", D, s_begin, s_end);
    return RL_EINVAL;
  }
  for (int d = 1; d < D; d++)
    if (site[d] <= site[d - 1]) {
      set_error("rl_copying_weights_host: the sites do not rise at row %d", d);
      return RL_EINVAL;
    }
  const int rc = copying_weights(site, D, rpos, s_begin, s_end, weights);
  if (rc) set_error("rl_copying_weights_host: %s", std::string(rl_last_error()).c_str());
  return rc;
}

int rl_copying_rows_host(const float *rows, const double *weights, int D, int N, double *c_row) {
  if (!rows || !weights || !c_row || D < 0 || N < 1) {
    set_error("rl_copying_rows_host: bad arguments (D=%d, N=%d)", D, N);
    return RL_EINVAL;
  }
  int bad = 0;
  copying_rows(rows, weights, D, N, c_row, &bad);
  if (bad) {
    set_error("CopyingMatrix: row %d: the posterior row has a weight and its sum is not finite and positive", bad - 1);
    return RL_ESTATE;
  }
  return RL_OK;
}

int rl_copying_matrix(rl_ctx *ctx, int w_first, int w_last, int sum_mode, double *C_host, long long *W_out) {
  if (!ctx || !ctx->have_chunk || !C_host || !W_out || w_first < 0 || w_last < w_first || w_last >= ctx->W) {
    set_error("rl_copying_matrix: bad arguments (windows %d..%d of %d; a chunk, a matrix and a count are needed)",
              w_first, w_last, ctx ? ctx->W : 0);
    return RL_EINVAL;
  }
  if (!ctx->painted) {
    set_error("rl_copying_matrix: rl_paint has not run");
    return RL_ESTATE;
  }
  if (stone_row(ctx, w_first, "rl_copying_matrix") < 0 || stone_row(ctx, w_last, "rl_copying_matrix") < 0) return RL_ESTATE;
  RL_HIP(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)ctx->nloc * ctx->N * sizeof(double);
  DevBuf d_C;
  int rc = d_C.alloc(bytes);
  if (rc) return rc;
  RL_HIP(hipMemset(d_C.p, 0, bytes));
  const size_t row_bytes = (size_t)ctx->S * 64 * ctx->waves * sizeof(float);
  for (int w = w_first; w <= w_last; w++) {
    // one window at a time, with the posterior rows the free HBM has room for (RELATE_AMD_WINDOW_ROWS: by hand, as
    // in the BuildTopology stage): a window that does not fit is reduced part by part, to the same bits
    long long max_rows = 0;
    if (const char *e = getenv("RELATE_AMD_WINDOW_ROWS")) {
      max_rows = std::max(0LL, atoll(e));
    } else {
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        max_rows = std::max<long long>(1, (long long)(0.6 * (double)(free_b + device_cache_held(ctx->device, row_bytes)) / (double)row_bytes));
    }
    rl_window *win = rl_window_open_bounded(ctx, w, nullptr, -1, sum_mode, max_rows, nullptr);
    if (!win) return RL_ESTATE;
    rc = rl_window_copying(win, d_C.p, nullptr);
    rl_window_close(win);
    if (rc) return rc;
  }
  RL_HIP(hipMemcpy(C_host, d_C.p, bytes, hipMemcpyDeviceToHost));
  *W_out = (long long)ctx->wb[w_last + 1] - ctx->wb[w_first];
  return RL_OK;
}

int rl_stage_copying_matrix(const char *out_dir, int chunk_index, int first_section, int last_section,
                            const rl_stage_opts *opts, const char *out_path) {
  rl_stage_opts o;
  if (int orc = rl_internal_resolve_opts(opts, &o)) return orc;
  if (!out_dir || !out_path || first_section < 0 || last_section < first_section) {
    set_error("rl_stage_copying_matrix: bad arguments (sections %d..%d)", first_section, last_section);
    return RL_EINVAL;
  }
  rl_ctx *ctx = rl_create(o.device);
  if (!ctx) return RL_ENODEVICE;
  int rc = rl_load_chunk(ctx, out_dir, chunk_index);
  if (!rc && o.use_painting) rc = rl_set_painting(ctx, o.theta, o.rho);
  if (!rc && first_section >= ctx->W) {
    set_error("rl_stage_copying_matrix: section %d, the chunk has %d", first_section, ctx->W);
    rc = RL_EINVAL;
  }
  const int w0 = first_section, w1 = rc ? 0 : std::min(last_section, ctx->W - 1);
  if (!rc) rc = rl_set_window_range(ctx, w0, w1);  // Paint keeps (and walks to) the stones of these windows only
  if (!rc) rc = rl_paint(ctx, o.sum_mode, nullptr);
  std::vector<double> C;
  long long W = 0;
  if (!rc) {
    C.assign((size_t)ctx->N * ctx->N, 0.0);
    rc = rl_copying_matrix(ctx, w0, w1, o.sum_mode, C.data(), &W);
  }
  if (!rc) {
    FILE *fp = fopen(out_path, "wb");
    const int32_t head[4] = {ctx->N, chunk_index, ctx->wb[w0], ctx->wb[w1 + 1]};
    const int64_t w = W;
    const bool ok = fp && fwrite(head, 4, 4, fp) == 4 && fwrite(&w, 8, 1, fp) == 1 && fwrite(C.data(), 8, C.size(), fp) == C.size();
    if ((fp && fclose(fp) != 0) || !ok) {
      set_error("writing %s failed", out_path);
      rc = RL_EIO;
    }
  }
  rl_destroy(ctx);
  return rc;
}

}  // extern "C"

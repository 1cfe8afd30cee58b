/* oracle_window_check.c -- the oracle's entries for the K2 / K3 geometry tests (ro_repaint_section_flags,
 * ro_window_open_targets, ro_window_matrix_row) under AddressSanitizer and UBSan, as a program of its own
 * (tools/oracle_window_check.sh builds and runs it on the CPU; it is not loaded into Python):
 *   oracle_window_check DIR
 * A window of some targets gives the rows of the whole window's matrix, the flags entry the bits of the plain one. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "relate_oracle.h"
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: oracle_window_check DIR\n"); return 64; }
  const char *dir = argv[1];
  const int N = 37, L = 60, W = 3;
  int wb[4] = {0, 12, 33, 60};
  char *seq = malloc((size_t)N * L);
  double *r = malloc(sizeof(double) * L), *rpos = malloc(sizeof(double) * (L + 1));
  unsigned s = 12345;
  for (int i = 0; i < N * L; i++) { s = s * 1103515245u + 12345u; seq[i] = ((s >> 16) % 100 < 20) ? '1' : '0'; }
  for (int i = 0; i < 14; i++) { memset(seq + (size_t)(14 + i) * N, '0', N); seq[(size_t)(14 + i) * N + 5] = '1'; }
  rpos[0] = 1e-5; for (int i = 0; i < L; i++) { r[i] = 2.5e-3; rpos[i + 1] = rpos[i] + 1e-6; }
  ro_data d = {N, L, seq, r, rpos, 0.001};
  if (ro_paint_chunk(&d, wb, W, dir, 2, 0, NULL, NULL)) return 1;
  ro_sum_order lanes = {RO_SUM_LANES, 0, 0};
  int targets[3] = {0, 5, 36};
  long flags = 0;
  for (int w = 0; w < W; w++) {
    char pf[256]; snprintf(pf, sizeof pf, "%s/relate_%d.bin", dir, w);
    ro_window *all = ro_window_open(&d, pf, wb[w], 2);
    ro_window *some = ro_window_open_targets(&d, pf, wb[w], 2, NULL, targets, 3);
    ro_window *ln = ro_window_open_targets(&d, pf, wb[w], 2, &lanes, NULL, 0);
    if (!all || !some || !ln) return 2;
    float *M = malloc(sizeof(float) * N * N), *row = malloc(sizeof(float) * N);
    for (int snp = wb[w]; snp < wb[w + 1]; snp++) {
      if (snp > wb[w]) { ro_window_advance(all, snp); ro_window_advance(some, snp); ro_window_advance(ln, snp); }
      ro_window_matrix(all, snp, M);
      for (int i = 0; i < 3; i++) {
        if (ro_window_matrix_row(some, snp, targets[i], row)) return 3;
        if (memcmp(row, M + (size_t)targets[i] * N, sizeof(float) * N)) { printf("row differs w=%d snp=%d\n", w, snp); return 4; }
      }
      if (ro_window_matrix_row(some, snp, 1, row) != -1) return 5;
      ro_window_matrix(ln, snp, M);
    }
    free(M); free(row);
    ro_window_free(all); ro_window_free(some); ro_window_free(ln);
  }
  /* flags entry against the plain one */
  {
    float *ab = calloc(N, sizeof(float)), *be = calloc(N, sizeof(float));
    for (int n = 0; n < N; n++) { ab[n] = 1.0f / N; be[n] = 1.0f; }
    int cap = 33 - 12 + 2;
    float *t1 = malloc(sizeof(float) * cap * N), *t2 = malloc(sizeof(float) * cap * N), l1[64], l2[64];
    unsigned char f[64], b[64];
    int D1 = ro_repaint_section(&d, ab, be, 12, 32, 0.f, 0.f, 5, NULL, t1, l1);
    int D2 = ro_repaint_section_flags(&d, ab, be, 12, 32, 0.f, 0.f, 5, NULL, t2, l2, f, b);
    if (D1 != D2 || memcmp(t1, t2, sizeof(float) * D1 * N) || memcmp(l1, l2, sizeof(float) * D1)) return 6;
    for (int i = 0; i < D1; i++) flags += f[i] + b[i];
    if (ro_repaint_section_flags(&d, ab, be, 12, 32, 0.f, 0.f, 5, &lanes, t2, l2, NULL, NULL) != D1) return 7;
    free(ab); free(be); free(t1); free(t2);
  }
  printf("ok, %ld rescales flagged\n", flags);
  free(seq); free(r); free(rpos);
  return 0;
}

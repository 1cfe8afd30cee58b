// treeseq.h -- the tree-sequence object of treeseq.cpp, for the files that drive it (stage.cpp, shard.cpp).
#pragma once
#include <atomic>
#include <vector>

#include "common.h"
#include "minmatch.h"

namespace rl {

struct SnpInfo {
  int tree = 0;
  std::vector<int> branch;
  bool flipped = false;
};

}  // namespace rl

struct rl_treeseq {
  int N = 0, L = 0;
  double theta = 0.001;
  std::vector<uint32_t> bits_own;  // panel (a copy: rl_treeseq_create), or
  const uint32_t *bits = nullptr;  // ... the caller's, which outlives the object (the stage: its context's panel)
  int row_words = 0;
  std::vector<double> rpos;
  std::vector<int> bp, state;
  int thr = 0;
  std::vector<rl::HostTree> trees;
  std::vector<rl::SnpInfo> info;  // indexed by snp - start
  int start = 0, end = 0;
  std::vector<char> member;  // carriers of the current SNP
  int num_carriers = 0;
  int build_device = -1;  // >= 0: trees are built on that GPU (minmatch_builder.hip), the host builder as fallback
  rl_matrix_dev_fn matrix_dev = nullptr;  // with it the distance matrices never leave the device
  rl_matrix_dev_ex_fn matrix_dev_ex = nullptr;  // ... and arrive with the carrier penalty applied and their row minima
  long long gpu_trees = 0, host_trees = 0;
  std::vector<double> sample_ages;  // N values (--sample_ages) or empty
  // the device builder's buffers (16 N^2 B of woven matrix) outlive a section: the next one of this object reuses them
  rl::DeviceMinMatch *dev_builder = nullptr;
  ~rl_treeseq() { delete dev_builder; }

  bool derived(int snp, int n) const { return (bits[(size_t)snp * row_words + (n >> 5)] >> (n & 31)) & 1u; }
};

namespace rl {

// as rl_treeseq_create, the panel borrowed instead of copied
rl_treeseq *treeseq_borrowing(int N, int L, const uint32_t *bits, int row_words, const double *rpos, const int *bp_pos,
                              const int *state, double theta);

// `--mode OptimizeParameters`: what the sections of one grid point add up (treeseq.cpp optimize_section)
struct OptRun {
  float log_ratio = 0.0f;            // (float) log(theta / ntheta), :852
  std::atomic<long long> count{0};   // SNPs of the sections that did not map
  std::atomic<long long> trees{0}, gpu_trees{0}, host_trees{0};  // built in all, by the device's workers, by the host
};
int optimize_section(rl_treeseq *ts, int start, int end, rl_window *win, OptRun &run);

}  // namespace rl

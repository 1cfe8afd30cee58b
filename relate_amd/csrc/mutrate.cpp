// mutrate.cpp -- AvgMutationRate, host side (include/relate_amd.h has the definition; the reference:
// include/evaluate/mutation_rate/AvgMutationRate.cpp).
//
// The per-tree quantity is the total branch length in every epoch.  HostLengths restates the reference's two functions
// operation by operation -- the std::sort of all 2N-1 node times by (time, label), the count of lineages per group of
// equal times, the serial walk with its epoch cursor and its float and double products -- and is the `device < 0`
// path and the authority the device (mutrate_kernels.hip) is held to, bit for bit.  This file also holds the readers
// of the .mut and of the --dist file, count_bases, the loop over the SNPs (two serial double sums, in the .mut's
// order), the writer of _avg.rate and the C entry points.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "anc_text.h"
#include "common.h"
#include "mut_text.h"
#include "mutrate.h"
#include "tree_host.h"

namespace rl {

namespace {

const char *const kMode = "AvgMutationRate";

// one tree's branch length per epoch as the reference computes it
struct HostLengths : TreeTables {
  std::vector<float> coords;    // coordinates_tree
  std::vector<int> order, lin;  // sorted_indices, num_lineages
  std::vector<int> lin_tmp;
  float root = 0.0f;  // coordinates_tree[root] after run: the last of the sorted float coordinates
  explicit HostLengths(int n) : TreeTables(n), coords(nodes), order(nodes), lin(nodes, 0), lin_tmp(nodes) {}

  // parent must have passed first_bad_node, bl first_bad_length.  out: E doubles, out[E-1] = 0
  void run(const int *parent, const double *bl, const double *epoch, int E, double *out) {
    fill(parent);
    // Tree::GetCoordinates (src/anc.cpp:525-537): the maximum over both children in double, a float at every node
    for (int v = 0; v < N; v++) coords[v] = 0.0f;
    for (int n = N; n < nodes; n++)
      coords[n] = (float)std::max((double)coords[second[n]] + bl[second[n]], (double)coords[first[n]] + bl[first[n]]);
    // GetCoordsAndLineages (:58-95)
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(),
              [this](int a, int b) { return coords[a] == coords[b] ? a < b : coords[a] < coords[b]; });
    int num_lins = 0, start = 0;
    double age = coords[order[0]];
    for (int i = 0; i < nodes; i++) {
      if (coords[order[i]] > age) {
        for (; start != i; start++) lin[order[start]] = num_lins;
        age = coords[order[start]];
      }
      if (order[i] < N) num_lins++;
      else num_lins--;
    }
    // (the group of the root keeps what an earlier tree left: no interval starts there)
    lin_tmp = lin;
    for (int i = 0; i < nodes; i++) lin[i] = lin_tmp[order[i]];
    std::sort(coords.begin(), coords.end());
    root = coords[nodes - 1];
    // GetBranchLengthsInEpoch (:228-291); the caller reads E entries of a vector shrunk to E - 1
    std::fill(out, out + E, 0.0);
    int ep = 0;
    for (ep = 0; ep < E; ep++)
      if (coords[0] < epoch[ep]) break;
    ep--;
    out[ep] = 0;
    for (int i = 1; i < nodes; i++) {
      if (coords[i] > coords[i - 1]) {
        if (coords[i] < epoch[ep + 1]) {
          if (coords[i - 1] >= epoch[ep]) out[ep] += lin[i - 1] * (coords[i] - coords[i - 1]);
          else out[ep] = lin[i - 1] * (coords[i] - epoch[ep]);
        } else {
          if (coords[i - 1] >= epoch[ep]) out[ep] += lin[i - 1] * (epoch[ep + 1] - coords[i - 1]);
          else out[ep] = lin[i - 1] * (epoch[ep + 1] - epoch[ep]);  // (the reference asserts it never gets here)
          ep++;
          if (ep == E - 1) break;
          while (ep < E - 1 && epoch[ep + 1] < coords[i]) {  // (the reference tests ep second, reading epoch[E])
            out[ep] = lin[i - 1] * (epoch[ep + 1] - epoch[ep]);
            ep++;
          }
          if (ep < E - 1) out[ep] = lin[i - 1] * (coords[i] - epoch[ep]);
          else break;
        }
      }
    }
  }
};

// the trees whose flag is not kTreeDone, on the host: checked, then -- unless the device has refused them --
// walked.  roots: null, or [ntrees]
int host_rows(const int *parents, const double *bl, int N, int ntrees, const double *ep, int E, double *out, float *roots,
              const char *where, const int *tree_id, const int *flags, bool refused_by_device) {
  const size_t nodes = (size_t)2 * N - 1;
  const auto tree_name = [&](int t) { return std::string(where) + ": tree " + std::to_string(tree_id ? tree_id[t] : t); };
  HostLengths host(N);
  std::vector<unsigned char> kids;
  for (int t = 0; t < ntrees; t++) {
    if (flags[t] == kTreeDone) continue;
    const int *parent = parents + t * nodes;
    const double *b = bl + t * nodes;
    if (const int rc = check_tree(tree_name(t).c_str(), parent, b, N, 2 * N - 2, refused_by_device, kids)) return rc;
    host.run(parent, b, ep, E, out + (size_t)t * E);
    if (roots) roots[t] = host.root;
  }
  return RL_OK;
}

// out [ntrees][E].  `where` names the trees' origin in a message; tree_id (or null: the index) what a tree is called
int mutrate_rows(const int *parents, const double *bl, int N, int ntrees, const double *ep, int E, int device, double *out,
                 const char *where, const int *tree_id) {
  if (N < 2 || N > kMutrateMaxN) {
    set_error("%s: trees of 2 <= N <= %d leaves (N=%d)", where, kMutrateMaxN, N);
    return RL_EINVAL;
  }
  std::vector<int> flags((size_t)ntrees, kTreeRefused);
  if (device >= 0) {
    if (const int rc = mutrate_device(parents, bl, N, ntrees, ep, E, device, out, flags.data())) return rc;
    if (std::count(flags.begin(), flags.end(), (int)kTreeDone) == ntrees) return RL_OK;
  }
  return host_rows(parents, bl, N, ntrees, ep, E, out, nullptr, where, tree_id, flags.data(), device >= 0);
}

// ------------------------------------------------------------------------------------------------ the file layer

// what AvgMutationRate reads of a SNP (Mutations::Read, src/mutations.cpp:229-430)
struct MutSnp {
  int pos = 0, dist = 0, tree = 0, branches = 0;
  float age_begin = 0.0f, age_end = 0.0f;
};

// `snp;pos;dist;rs_id;tree;branches;is_not_mapping;is_flipped;age_begin;age_end;...`
int read_mut(const std::string &fn, std::vector<MutSnp> &snps) {
  const char *const format = "snp;pos;dist;rs_id;tree;branches;is_not_mapping;is_flipped;age_begin;age_end;...";
  return read_mut_lines(kMode, fn, format, nullptr, snps, [](std::vector<std::string> &col, MutSnp &m, long long) {
    bool ok = col.size() >= 10 && parse_int(col[1], &m.pos) && parse_int(col[2], &m.dist) && parse_int(col[4], &m.tree);
    if (ok) {
      char *end = nullptr;
      m.age_begin = (float)strtod(col[8].c_str(), &end);  // (std::stod into a float)
      ok = end != col[8].c_str();
      m.age_end = (float)strtod(col[9].c_str(), &end);
      ok = ok && end != col[9].c_str();
      std::istringstream br(col[5]);
      for (std::string b; ok && br >> b;) {
        int v = 0;
        ok = parse_int(b, &v);
        m.branches++;
      }
    }
    return ok ? RL_OK : RL_EFORMAT;
  });
}

// :458-494: the scan of the position list for the .mut's positions, in order
int count_bases_of(const std::vector<MutSnp> &mut, const std::vector<int> &pos, const std::vector<int> &dist,
                   const char *list_name, std::vector<double> &count_bases) {
  const double total_num_bases = 1e9;
  const size_t L = mut.size(), M = pos.size();
  count_bases.assign(L, 0.0);
  size_t s = 0, j = 0;
  if (mut[0].pos == pos[0]) {
    count_bases[0] = 0.5 * dist[0] / total_num_bases;
    s++;
  }
  for (j = 1; s < L; j++) {
    if (j >= M) {
      set_error("%s: SNP %zu of the .mut (position %d) is not in %s: the reference reads past the end of its list", kMode, s,
                mut[s].pos, list_name);
      return RL_EINVAL;
    }
    if (mut[s].pos == pos[j]) {
      count_bases[s] = 0.5 * dist[j - 1] / total_num_bases;
      count_bases[s] += 0.5 * dist[j] / total_num_bases;
      s++;
    }
  }
  return RL_OK;
}

}  // namespace

int mutrate_host_rows(const int *parents, const double *bl, int N, int ntrees, const double *ep, int E, double *out,
                      float *roots, const char *where, const int *tree_id, bool refused_by_device) {
  if (N < 2 || N > kMutrateMaxN) {
    set_error("%s: trees of 2 <= N <= %d leaves (N=%d)", where, kMutrateMaxN, N);
    return RL_EINVAL;
  }
  const std::vector<int> flags((size_t)ntrees, kTreeRefused);
  return host_rows(parents, bl, N, ntrees, ep, E, out, roots, where, tree_id, flags.data(), refused_by_device);
}

}  // namespace rl

using namespace rl;

extern "C" int rl_mutrate_batch_trees(int N) { return N < 2 ? 0 : mutrate_batch_trees(N); }

extern "C" int rl_mutrate_epochs(float years_per_gen, const char *bins_or_null, double *epochs, int *nepochs) {
  return make_epochs("rl_mutrate_epochs", years_per_gen, bins_or_null, epochs, nepochs);
}

extern "C" int rl_mutrate_trees(const int *parents, const double *branch_length, int N, int ntrees, const double *epochs,
                                int nepochs, int device, double *out) {
  if (!parents || !branch_length || !epochs || !out || ntrees < 0) {
    set_error("rl_mutrate_trees: bad arguments (ntrees=%d; no null pointers)", ntrees);
    return RL_EINVAL;
  }
  if (const int rc = check_epochs("rl_mutrate_trees", epochs, nepochs, kMutrateMaxEpochs)) return rc;
  return mutrate_rows(parents, branch_length, N, ntrees, epochs, nepochs, device, out, "rl_mutrate_trees", nullptr);
}

extern "C" int rl_mutrate_anc(const char *anc_path, const char *mut_path, const char *dist_path_or_null,
                              const double *epochs, int nepochs, int device, double *mutation, double *opportunity,
                              long long *mapped_snps) {
  if (!anc_path || !mut_path || !epochs || !mutation || !opportunity) return null_args("rl_mutrate_anc");
  if (const int rc = check_epochs("rl_mutrate_anc", epochs, nepochs, kMutrateMaxEpochs)) return rc;
  const int E = nepochs;
  AncText anc(kMode);
  int rc = anc.open(anc_path);
  if (rc) return rc;
  if (anc.has_ages) {
    set_error("%s: %s has sample ages: the coordinates with sample ages are not part of this build", kMode, anc_path);
    return RL_EINVAL;
  }
  const int N = anc.N;
  if (N > kMutrateMaxN) {
    set_error("%s: %s: trees of 2 <= N <= %d leaves (N=%d)", kMode, anc_path, kMutrateMaxN, N);
    return RL_EINVAL;
  }
  std::vector<MutSnp> mut;
  if ((rc = read_mut(mut_path, mut))) return rc;
  if (mut.back().tree >= anc.trees || mut.front().tree < 0) {
    set_error("%s: %s names tree %d, %s holds %d", kMode, mut_path, mut.front().tree < 0 ? mut.front().tree : mut.back().tree, anc_path, anc.trees);
    return RL_EINVAL;
  }
  std::vector<int> pos, dist;
  if (dist_path_or_null) {
    if ((rc = read_dist(kMode, dist_path_or_null, pos, &dist))) return rc;
  } else {
    for (const MutSnp &m : mut) pos.push_back(m.pos), dist.push_back(m.dist);
  }
  std::vector<double> count_bases;
  if ((rc = count_bases_of(mut, pos, dist, dist_path_or_null ? dist_path_or_null : "its own columns", count_bases))) return rc;

  // the trees with a one-branch SNP go up batch by batch; their E doubles come back and the SNPs of the batch are
  // added in the .mut's order (:519-586)
  SnpTreeBatches w(N, mutrate_batch_trees(N));
  std::vector<double> lengths;
  std::vector<size_t> snp_id;  // the mapped SNPs of the batch
  std::vector<int> snp_tree;   // ... and the tree of each, within the batch
  std::fill(mutation, mutation + E, 0.0);
  std::fill(opportunity, opportunity + E, 0.0);
  long long mapped = 0;
  // RELATE_AMD_TIMING=1: where the wall-clock of the mode goes (reading the text, the trees' lengths, the SNP loop)
  typedef std::chrono::steady_clock Clock;
  const auto since = [](Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); };
  const Clock::time_point begun = Clock::now();
  double trees_seconds = 0.0, snps_seconds = 0.0;
  int trees_done = 0;
  const auto flush = [&]() -> int {
    const int held = (int)w.tree_id.size();
    lengths.assign((size_t)held * E, 0.0);
    Clock::time_point t0 = Clock::now();
    if (const int r = mutrate_rows(w.parents.data(), w.bl.data(), N, held, epochs, E, device, lengths.data(), anc_path, w.tree_id.data()))
      return r;
    trees_seconds += since(t0);
    trees_done += held;
    t0 = Clock::now();
    for (size_t i = 0; i < snp_id.size(); i++) {
      const MutSnp &m = mut[snp_id[i]];
      const double *in_epoch = &lengths[(size_t)snp_tree[i] * E];
      int ep = 0;
      while (epochs[ep] <= m.age_begin) {
        ep++;
        if (ep == E) break;
      }
      ep--;
      if (ep < 0) {
        set_error("%s: %s: SNP %zu has age_begin %g below 0: the reference aborts on this input", kMode, mut_path, snp_id[i], (double)m.age_begin);
        return RL_EINVAL;
      }
      mapped++;
      const float age_end = m.age_end;
      const double branch_length = age_end - m.age_begin;  // (a float difference)
      if (ep < E - 1) {
        if (age_end <= epochs[ep + 1]) {
          mutation[ep] += 1.0;
        } else {
          mutation[ep] += (epochs[ep + 1] - m.age_begin) / branch_length;
          ep++;
          while (ep < E - 1 && epochs[ep + 1] <= age_end) {
            mutation[ep] += (epochs[ep + 1] - epochs[ep]) / branch_length;
            ep++;
          }
          if (ep + 1 != E) mutation[ep] += (age_end - epochs[ep]) / branch_length;
        }
      }
      for (int e = 0; e < E; e++) opportunity[e] += in_epoch[e] * count_bases[snp_id[i]];
    }
    snps_seconds += since(t0);
    snp_id.clear(), snp_tree.clear();
    return RL_OK;
  };
  const auto take = [&](size_t s, int slot) {
    if (mut[s].branches == 1) snp_id.push_back(s), snp_tree.push_back(slot);
    return RL_OK;
  };
  if ((rc = w.walk(anc, mut.size(), [&](size_t k) { return mut[k].tree; }, [&](size_t k) { return mut[k].branches == 1; }, take, flush)))
    return rc;
  if (timing_level() >= 1)
    fprintf(stderr, "[mutrate] %d trees of N=%d on %s: %.6f s; SNP loop (%lld mapped): %.6f s; reading the text and the rest: %.6f s\n",
            trees_done, N, device >= 0 ? "the device" : "the host", trees_seconds, mapped, snps_seconds,
            since(begun) - trees_seconds - snps_seconds);
  if (mapped_snps) *mapped_snps = mapped;
  return RL_OK;
}

extern "C" int rl_mutrate_write(const char *path, const double *epochs, int nepochs, const double *mutation,
                                const double *opportunity) {
  if (!path || !epochs || !mutation || !opportunity || nepochs < 0) return null_args("rl_mutrate_write");
  std::ofstream os(path);
  if (os.fail()) {
    set_error("%s: error while opening file %s", kMode, path);
    return RL_EIO;
  }
  const double total_num_bases = 1e9;
  for (int e = 0; e < nepochs; e++) {
    const double rate = (mutation[e] / opportunity[e]) / total_num_bases;
    os << epochs[e] << " " << rate << "\n";
  }
  os.close();
  if (os.fail()) {
    set_error("%s: writing %s failed", kMode, path);
    return RL_EIO;
  }
  return RL_OK;
}

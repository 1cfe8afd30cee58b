// coaltree.cpp -- CoalRateForTree, host side (include/relate_amd.h has the definition; the reference:
// include/evaluate/coalescent_rate/coal_tree.cpp and CoalescenceRateForTree, CoalescentRateForSection.cpp:605-858).
//
// HostCoalTree restates coal_tree::populate operation by operation -- the std::sort of all 2N-1 node times by (time,
// label), the lineage count per group of equal times, the walk over the ranks with its epoch cursor, every term added
// straight onto the accumulators of the current block of trees -- and is the `device < 0` path and the authority the
// device (coaltree_kernels.hip) is held to, bit for bit.  This file also holds the loop over the text .anc with the
// factors of AncMutIterators::NextTree (mut_text.h), the sum of the blocks, the rate rule and the writer of
// coal_tree::Dump, and the C entry points.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <fstream>
#include <numeric>
#include <string>
#include <tuple>
#include <vector>

#include "anc_text.h"
#include "coaltree.h"
#include "common.h"
#include "mut_text.h"
#include "tree_host.h"

namespace rl {

namespace {

const char *const kMode = "CoalRateForTree";

// coal_tree with num_bootstrap = 1: the accumulators of every block and the tree that is being added
struct HostCoalTree : TreeTables {
  std::vector<float> coords;
  std::vector<int> sorted_indices, num_lins;
  int E, block_size, num_blocks, current_block = 0, count_trees = 0;
  std::vector<double> num, denom;  // [num_blocks][E]
  HostCoalTree(int n, int e, long long ntrees, int bs)
      : TreeTables(n), coords(nodes), sorted_indices(nodes), num_lins(nodes), E(e), block_size(bs),
        num_blocks(coaltree_num_blocks(ntrees, bs)), num((size_t)num_blocks * e, 0.0), denom((size_t)num_blocks * e, 0.0) {}

  // coal_tree::populate (coal_tree.cpp:98-199).  parent must have passed first_bad_node, bl first_bad_length.
  // 0, or which of the reference's live asserts fails: 1 `lins >= 1`, 2 `current_block < num_blocks`
  int populate(const int *parent, const double *bl, double num_bases_tree_persists, const double *epochs) {
    fill(parent);
    // Tree::GetCoordinates (src/anc.cpp:525-537): the maximum over both children in double, a float at every node
    for (int v = 0; v < N; v++) coords[v] = 0.0f;
    for (int n = N; n < nodes; n++)
      coords[n] = (float)std::max((double)coords[second[n]] + bl[second[n]], (double)coords[first[n]] + bl[first[n]]);

    std::iota(sorted_indices.begin(), sorted_indices.end(), 0);
    std::sort(sorted_indices.begin(), sorted_indices.end(),
              [&](int i1, int i2) { return std::tie(coords[i1], i1) < std::tie(coords[i2], i2); });
    int lins = 0;
    float age = coords[sorted_indices[0]];
    int prev = 0, w = 0;  // it_sorted_indices_prev, it_num_lins
    for (int i = 0; i < nodes; i++) {
      if (coords[sorted_indices[i]] > age) {
        while (coords[sorted_indices[prev]] == age) {
          num_lins[w] = lins;
          w++;
          prev++;
        }
        age = coords[sorted_indices[prev]];
      }
      if (sorted_indices[i] < N) lins++;
      else lins--;
      if (!(lins >= 1)) return 1;
    }
    while (coords[sorted_indices[prev]] == age) {
      num_lins[w] = lins;
      w++;
      prev++;
      if (w == nodes) break;
    }
    if (count_trees == block_size) {
      current_block++;
      count_trees = 0;
      if (!(current_block < num_blocks)) return 2;
    }
    std::sort(coords.begin(), coords.end());

    double *it2_num = &num[(size_t)current_block * E], *it2_denom = &denom[(size_t)current_block * E];
    int l = 0, r = 1;  // it_num_lins; it_coords_next and it_sorted_indices
    double current_lower_age = epochs[0];
    for (int c = 1; c != E;) {
      while (coords[r] <= epochs[c]) {
        if (sorted_indices[r] >= N) *it2_num += num_bases_tree_persists / 1e9;
        *it2_denom += num_bases_tree_persists * num_lins[l] * (num_lins[l] - 1) / 2.0 * (coords[r] - current_lower_age) / 1e9;
        current_lower_age = coords[r];
        l++;
        r++;
        if (r == nodes) break;
      }
      if (r == nodes) break;
      *it2_denom += num_bases_tree_persists * num_lins[l] * (num_lins[l] - 1) / 2.0 * (epochs[c] - current_lower_age) / 1e9;
      current_lower_age = epochs[c];
      c++;
      it2_num++;
      it2_denom++;
    }
    count_trees++;
    return 0;
  }
};

// the accumulators in the making, on the host or on a device
struct Coaltree {
  int N = 0, E = 0;
  const double *ep = nullptr;
  CoaltreeDevice *dev = nullptr;
  HostCoalTree *host = nullptr;
  ~Coaltree() {
    if (dev) coaltree_device_free(dev);
    delete host;
  }
  // `who` names the entry point or the file; ntrees: the trees of the whole sequence
  int begin(const char *who, int n, const double *epochs, int e, long long ntrees, int block_size, int device) {
    N = n, E = e, ep = epochs;
    if (N < 2 || N > kCoaltreeMaxN) {
      set_error("%s: trees of 2 <= N <= %d leaves (N=%d)", who, kCoaltreeMaxN, N);
      return RL_EINVAL;
    }
    if (device >= 0) return coaltree_device_begin(&dev, N, ep, E, ntrees, block_size, device);
    host = new HostCoalTree(N, E, ntrees, block_size);
    return RL_OK;
  }
  // the trees that follow those added before.  `where` names the trees' origin in a message, index0 the first tree's
  // number there
  int add(const int *parents, const double *bl, const float *factors, int ntrees, const char *where, long long index0) {
    const size_t nodes = (size_t)2 * N - 1;
    for (int t = 0; t < ntrees; t++)
      if (!(factors[t] >= 0.0f && factors[t] <= FLT_MAX)) {
        set_error("%s: tree %lld: its factor %g is negative or not finite", where, index0 + t, (double)factors[t]);
        return RL_EINVAL;
      }
    int bad = -1;
    if (dev) {
      const int rc = coaltree_device_add(dev, parents, bl, factors, ntrees, &bad);
      if (bad < 0) return rc;
    }
    std::vector<unsigned char> kids;
    for (int t = dev ? bad : 0; t < (dev ? bad + 1 : ntrees); t++) {
      const int *parent = parents + t * nodes;
      const double *b = bl + t * nodes;
      const std::string tree = std::string(where) + ": tree " + std::to_string(index0 + t);
      if (const int rc = check_tree(tree.c_str(), parent, b, N, 2 * N - 2, dev != nullptr, kids)) return rc;
      if (const int failed = host->populate(parent, b, (double)factors[t], ep)) {
        set_error("%s: the reference's assert `%s` fails", tree.c_str(), failed == 1 ? "lins >= 1" : "current_block < num_blocks");
        return RL_EINVAL;
      }
    }
    return RL_OK;
  }
  // num, denom: [num_blocks][E]
  int finish(double *num, double *denom) {
    if (dev) return coaltree_device_finish(dev, num, denom);
    memcpy(num, host->num.data(), host->num.size() * 8);
    memcpy(denom, host->denom.data(), host->denom.size() * 8);
    return RL_OK;
  }
};

}  // namespace
}  // namespace rl

using namespace rl;

extern "C" int rl_coaltree_batch_trees(int N) { return N < 2 ? 0 : coaltree_batch_trees(N); }

extern "C" int rl_coaltree_num_blocks(long long ntrees, int block_size) {
  return ntrees < 0 || block_size < 1 ? 0 : coaltree_num_blocks(ntrees, block_size);
}

extern "C" int rl_coaltree_trees(const int *parents, const double *branch_length, const float *factors, int N, int ntrees,
                                 const double *epochs, int nepochs, int block_size, int device, double *num, double *denom,
                                 int *num_blocks) {
  if (!parents || !branch_length || !factors || !epochs || !num || !denom || !num_blocks || ntrees < 0 || block_size < 1) {
    set_error("rl_coaltree_trees: bad arguments (ntrees=%d, block_size=%d; no null pointers)", ntrees, block_size);
    return RL_EINVAL;
  }
  if (const int rc = check_epochs("rl_coaltree_trees", epochs, nepochs, kCoaltreeMaxEpochs)) return rc;
  const int blocks = coaltree_num_blocks(ntrees, block_size), room = *num_blocks;
  *num_blocks = blocks;
  if (blocks > room) {
    set_error("rl_coaltree_trees: %d trees in blocks of %d are %d blocks, room for %d", ntrees, block_size, blocks, room);
    return RL_EINVAL;
  }
  Coaltree ct;
  int rc = ct.begin("rl_coaltree_trees", N, epochs, nepochs, ntrees, block_size, device);
  rc = rc ? rc : ct.add(parents, branch_length, factors, ntrees, "rl_coaltree_trees", 0);
  return rc ? rc : ct.finish(num, denom);
}

extern "C" int rl_coaltree_anc(const char *anc_path, const char *mut_path, const double *epochs, int nepochs, int device,
                               double *num, double *denom, int *ntrees) {
  if (!anc_path || !mut_path || !epochs || !num || !denom) return null_args("rl_coaltree_anc");
  if (const int rc = check_epochs("rl_coaltree_anc", epochs, nepochs, kCoaltreeMaxEpochs)) return rc;
  const int E = nepochs;
  AncText anc(kMode);
  int rc = anc.open(anc_path);
  if (rc) return rc;
  if (anc.has_ages) {
    set_error("%s: %s has sample ages: the coordinates with sample ages are not part of this build", kMode, anc_path);
    return RL_EINVAL;
  }
  if (anc.trees < 1) {
    set_error("%s: %s holds no tree", kMode, anc_path);
    return RL_EFORMAT;
  }
  const int N = anc.N;
  std::vector<MutRow> mut;
  if ((rc = read_mut_rows(kMode, mut_path, mut))) return rc;
  Coaltree ct;
  if ((rc = ct.begin(anc_path, N, epochs, E, anc.trees, kCoaltreeBlockSize, device))) return rc;
  // the loop of CoalescentRateForSection.cpp:757-766: every tree with the bases it persists for, until NextTree
  // returns a negative number -- after the last tree, or a negative persistence
  FactorTreeBatches w(N, coaltree_batch_trees(N));
  Persistence persistence(mut);
  const auto add = [&](const int *p, const double *b, const float *f, int n, long long index0) {
    return ct.add(p, b, f, n, anc_path, index0);
  };
  for (int t = 0; t < anc.trees; t++) {
    if ((rc = w.read(anc, t, add))) return rc;
    const float num_bases_tree_persists = (float)persistence.next(t);
    if (!(num_bases_tree_persists >= 0.0)) break;
    w.factors[w.held++] = num_bases_tree_persists;
  }
  if ((rc = w.flush(add))) return rc;
  const int blocks = coaltree_num_blocks(anc.trees, kCoaltreeBlockSize);
  std::vector<double> block_num((size_t)blocks * E), block_denom((size_t)blocks * E);
  if ((rc = ct.finish(block_num.data(), block_denom.data()))) return rc;
  // coal_tree::Dump with one bootstrap (coal_tree.cpp:242-297): every block once, in order
  for (int e = 0; e < E; e++) num[e] = denom[e] = 0.0;
  for (int b = 0; b < blocks; b++)
    for (int e = 0; e < E; e++) {
      num[e] += 1 * block_num[(size_t)b * E + e];
      denom[e] += 1 * block_denom[(size_t)b * E + e];
    }
  if (ntrees) *ntrees = (int)w.index0;
  return RL_OK;
}

extern "C" int rl_coaltree_rates(const double *num, const double *denom, int nepochs, double *rates) {
  if (!num || !denom || !rates || nepochs < 0) return null_args("rl_coaltree_rates");
  for (int i = 0; i < nepochs; i++) {  // coal_tree.cpp:309-319
    rates[i] = 0.0;
    if (denom[i] != 0) rates[i] = num[i] / denom[i];
    else if (i > 0) rates[i] = rates[i - 1];
  }
  return RL_OK;
}

extern "C" int rl_coaltree_write(const char *path, const double *epochs, int nepochs, const double *rates) {
  if (!path || !epochs || !rates || nepochs < 0) return null_args("rl_coaltree_write");
  std::ofstream os(path);
  if (os.fail()) {
    set_error("%s: error while opening file %s", kMode, path);
    return RL_EIO;
  }
  os << 0 << " " << "\n";  // coal_tree.cpp:299-343: one bootstrap
  for (int e = 0; e < nepochs; e++) os << epochs[e] << " ";
  os << "\n";
  os << "0 0 ";
  for (int e = 0; e < nepochs; e++) os << rates[e] << " ";
  os << "\n";
  os.close();
  if (os.fail()) {
    set_error("%s: writing %s failed", kMode, path);
    return RL_EIO;
  }
  return RL_OK;
}

// frequency.cpp -- Frequency, host side (include/relate_amd.h has the definition; the reference:
// include/evaluate/selection/RelateSelection.cpp:330-814).
//
// For every SNP of a .mut that maps to one branch b of its tree, the reference walks the tree from the root down in
// the order (time, label) and writes, at every epoch boundary, how many lineages remain (.lin) and how many of them
// carry the derived allele (.freq).  HostWalk is that walk restated statement by statement -- its sorts, its state
// machine, its order of ties -- with every assert of the reference (live in its build) turned into RL_EINVAL naming
// the tree and the SNP.  It is the `device < 0` path, the yardstick of the GPU tests and the authority for trees with
// tied times: the device (frequency_kernels.hip) answers tie-free trees from a closed form and hands the others back.
// This file also holds the reader of the .mut, the SNP filter, the two writers and the C entry points.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <fstream>
#include <memory>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "anc_text.h"
#include "common.h"
#include "frequency.h"
#include "mut_text.h"
#include "tree_host.h"

namespace rl {

namespace {

const char *const kMode = "Frequency";

// one tree's coordinates and the reference's walk over them
struct HostWalk : TreeTables {
  const int *par = nullptr;
  std::vector<float> unsorted, sorted, mut;  // coordinates_tree_unsrt, coordinates_tree, coordinates_mutation
  std::vector<int> index, index_mut, current, stack;
  const char *failed = nullptr;  // the check the last walk failed
  explicit HostWalk(int n) : TreeTables(n), unsorted(nodes), sorted(nodes), mut(nodes), index(nodes), index_mut(nodes), current(n) {}

  // sortAndGetIndices (:16-41): by (value, index)
  static void sort_with_indices(std::vector<float> &vec, std::vector<int> &idx, std::vector<float> &tmp) {
    std::iota(idx.begin(), idx.end(), 0);
    std::sort(idx.begin(), idx.end(), [&vec](int a, int b) { return vec[a] == vec[b] ? a < b : vec[a] < vec[b]; });
    tmp.resize(vec.size());
    for (size_t i = 0; i < vec.size(); i++) tmp[i] = vec[idx[i]];
    vec.swap(tmp);
  }

  // parent must have passed first_bad_node, the branch lengths first_bad_length.  Tree::GetCoordinates
  // (src/anc.cpp:525-537): the maximum over both children in double, rounded to float at every node
  void prepare(const int *parent, const double *bl) {
    par = parent;
    fill(parent);
    for (int v = 0; v < N; v++) unsorted[v] = 0.0f;
    for (int n = N; n < nodes; n++)
      unsorted[n] = (float)std::max((double)unsorted[second[n]] + bl[second[n]], (double)unsorted[first[n]] + bl[first[n]]);
    sorted = unsorted;
    sort_with_indices(sorted, index, tmp_);
  }
  float root_time() const { return sorted[nodes - 1]; }

  // :556-788 for branch b (neither -1 nor the root): freq [E], lin [E] from the oldest boundary to 0; tail: TreeFreq,
  // when_DAF_is_half, when_mutation_has_freq2.  false: a check of the reference failed (`failed` names it)
  bool walk(int b, const float *ep, int E, int *freq, int *lin, int *tail) {
#define RL_WALK_CHECK(cond)   \
  do {                        \
    if (!(cond)) {            \
      failed = #cond;         \
      return false;           \
    }                         \
  } while (0)
    const int root = nodes - 1;
    int col = 0;
    int DAF = 0;
    std::fill(mut.begin(), mut.end(), -1.0f);
    stack.assign(1, b);  // CopyCoordinates (:60-72)
    while (!stack.empty()) {
      const int v = stack.back();
      stack.pop_back();
      mut[v] = unsorted[v];
      if (v < N) DAF++;
      else stack.push_back(first[v]), stack.push_back(second[v]);
    }
    const int DAF_half = (int)((DAF + 1) / 2.0);
    mut[par[b]] = unsorted[par[b]];
    sort_with_indices(mut, index_mut, tmp_);
    std::fill(current.begin(), current.end(), -2);
    int num_carriers = 0, num_lineages = 1;
    int k_appears = -1, k_freq2 = -1, has_disappeared = -2, num_lin_half = -1;
    int n_mut = root, n_tree = root, e = E - 1;
    while (sorted[n_tree] < ep[e]) {  // (ep[0] = 0 and no time is negative: e stays >= 0)
      freq[col] = 0, lin[col] = 0, col++;
      e--;
      RL_WALK_CHECK(e >= 0);
    }
    do {
      if (num_carriers >= DAF_half && DAF_half > 1 && num_lin_half == -1) num_lin_half = num_lineages;
      while (sorted[n_tree] <= ep[e]) {
        RL_WALK_CHECK(col < E);
        freq[col] = k_appears != -1 && has_disappeared != 1 ? num_carriers : 0;
        lin[col] = num_lineages;
        col++;
        e--;
        if (e == -1) break;
      }
      RL_WALK_CHECK(num_carriers >= 0);
      RL_WALK_CHECK(num_lineages >= 0);
      for (int k = 0; k < num_carriers; k++) RL_WALK_CHECK(current[k] != -1);
      RL_WALK_CHECK(n_mut >= 0);
      const float coords = sorted[n_tree];
      const auto other_event = [&]() {  // a node that does not carry: a leaf ends a lineage, a coalescence adds one
        if (index[n_tree] < N) num_lineages--;
        else num_lineages++;
        n_tree--;
      };
      if (coords != mut[n_mut] || has_disappeared == 1) {
        while (coords == sorted[n_tree]) {
          other_event();
          if (n_tree < 0) break;
        }
      } else {
        while (sorted[n_tree] == coords) {
          if (index[n_tree] != index_mut[n_mut] || mut[n_mut] == -1) {
            other_event();
          } else {
            RL_WALK_CHECK(mut[n_mut] == coords);
            bool found = false;
            const int node = index_mut[n_mut];
            if (k_appears == -1) {
              num_lineages++;
              k_appears = num_lineages;
              RL_WALK_CHECK(par[b] == node);
              current[0] = b;
              num_carriers = 1;
              has_disappeared = -1;
              found = true;
            } else {
              for (int k = 0; k < num_carriers; k++)
                if (current[k] >= 0 && current[k] == node) {
                  found = true;
                  if (node < N) {
                    current[k] = -1;
                  } else {
                    RL_WALK_CHECK(num_carriers < N);
                    current[k] = first[node];
                    current[num_carriers] = second[node];
                    num_lineages++;
                    num_carriers++;
                  }
                }
            }
            RL_WALK_CHECK(found);
            n_tree--;
            n_mut--;
          }
          if (n_tree < 0 || n_mut < 0) break;
        }
        if (n_tree >= 0 && n_mut >= 0) {
          RL_WALK_CHECK(mut[n_mut] != coords);
          RL_WALK_CHECK(sorted[n_tree] != coords);
        }
      }
      if (num_carriers >= 2 && k_freq2 == -1) {
        k_freq2 = num_lineages;
        RL_WALK_CHECK(k_freq2 != 0);
      }
      for (int k = 0; k < num_carriers; k++) {  // the carriers that ended in a leaf leave the list
        for (int l = num_carriers - 1; l >= 0; l--) {
          if (current[l] != -1) break;
          num_carriers--;
          num_lineages--;
          if (num_carriers == 0) break;
        }
        if (k < num_carriers && current[k] == -1) {
          current[k] = current[num_carriers - 1];
          num_carriers--;
          num_lineages--;
        }
      }
      if (has_disappeared == -1 && num_carriers == 0) has_disappeared = 1;
      RL_WALK_CHECK(num_carriers <= num_lineages);
      RL_WALK_CHECK(num_lineages >= 0);
      RL_WALK_CHECK(num_carriers >= 0);
    } while (n_tree >= 0 && e >= 0);
    RL_WALK_CHECK(col == E);  // (a row of the reference with fewer columns)
    tail[0] = num_carriers;
    tail[1] = num_lin_half;
    tail[2] = k_freq2;
    return true;
#undef RL_WALK_CHECK
  }

 private:
  std::vector<float> tmp_;
};

// The rows of nsnps SNPs (tree indices rising) over ntrees trees: freq [nsnps][E+1] (the counts, TreeFreq), lin
// [nsnps][E+2] (the counts, when_DAF_is_half, when_mutation_has_freq2), marks [nsnps] (1: the row is there; 0: the
// branch is -1 or the root), root_time [ntrees].  `where` names the trees' origin in a message; tree_id / snp_id (or
// null: the index) what a tree and a SNP are called there.
int frequency_rows(const int *parents, const double *bl, int N, int ntrees, const int *snp_tree, const int *snp_branch,
                   int nsnps, const float *ep, int E, int device, int *freq, int *lin, unsigned char *marks,
                   float *root_time, int *host_trees, const char *where, const int *tree_id, const int *snp_id) {
  const size_t nodes = (size_t)2 * N - 1;
  const int root = 2 * N - 2;
  const auto tree_name = [&](int t) { return std::string(where) + ": tree " + std::to_string(tree_id ? tree_id[t] : t); };
  const auto snp_name = [&](int s) { return snp_id ? snp_id[s] : s; };
  std::vector<int> snp_first((size_t)ntrees + 1, 0);
  for (int s = 0; s < nsnps; s++) {
    if (snp_tree[s] < 0 || snp_tree[s] >= ntrees || (s && snp_tree[s] < snp_tree[s - 1])) {
      set_error("%s: SNP %d is on tree %d: the tree indices must not fall and lie in [0, %d)", where, snp_name(s), snp_tree[s], ntrees);
      return RL_EINVAL;
    }
    if (snp_branch[s] < -1 || snp_branch[s] > root) {
      set_error("%s: SNP %d is on branch %d of a tree with %zu nodes", where, snp_name(s), snp_branch[s], nodes);
      return RL_EINVAL;
    }
    marks[s] = snp_branch[s] != -1 && snp_branch[s] != root;
    snp_first[snp_tree[s] + 1]++;
  }
  for (int t = 0; t < ntrees; t++) snp_first[t + 1] += snp_first[t];
  std::vector<int> flags((size_t)ntrees, kTreeNeedsHost), rows;
  if (device >= 0) {
    rows.resize((size_t)nsnps * (2 * E + 2));
    if (const int rc = frequency_device(parents, bl, N, ntrees, snp_first.data(), snp_branch, nsnps, ep, E, device,
                                        rows.data(), root_time, flags.data()))
      return rc;
  }
  std::unique_ptr<HostWalk> host;  // made for the first tree that needs it
  *host_trees = 0;
  for (int t = 0; t < ntrees; t++) {
    const int *parent = parents + t * nodes;
    const double *b = bl + t * nodes;
    if (flags[t] == kTreeDone) {
      for (int s = snp_first[t]; s < snp_first[t + 1]; s++) {
        if (!marks[s]) continue;
        const int *row = &rows[(size_t)s * (2 * E + 2)];
        memcpy(freq + (size_t)s * (E + 1), row, (size_t)E * 4);
        freq[(size_t)s * (E + 1) + E] = 0;  // TreeFreq: the walk has consumed the leaves after its last output
        memcpy(lin + (size_t)s * (E + 2), row + E, ((size_t)E + 2) * 4);
      }
      continue;
    }
    std::vector<unsigned char> kids;
    if (const int rc = check_tree(tree_name(t).c_str(), parent, b, N, 2 * N - 2, flags[t] == kTreeRefused, kids)) return rc;
    if (!host) host.reset(new HostWalk(N));
    bool walked = false;
    host->prepare(parent, b);
    root_time[t] = host->root_time();
    for (int s = snp_first[t]; s < snp_first[t + 1]; s++) {
      if (!marks[s]) continue;
      walked = true;
      int tail[3];
      if (!host->walk(snp_branch[s], ep, E, freq + (size_t)s * (E + 1), lin + (size_t)s * (E + 2), tail)) {
        set_error("%s, SNP %d (branch %d): the reference's walk fails its check `%s`: the reference aborts on this input",
                  tree_name(t).c_str(), snp_name(s), snp_branch[s], host->failed);
        return RL_EINVAL;
      }
      freq[(size_t)s * (E + 1) + E] = tail[0];
      lin[(size_t)s * (E + 2) + E] = tail[1];
      lin[(size_t)s * (E + 2) + E + 1] = tail[2];
    }
    *host_trees += walked;
  }
  return RL_OK;
}

// ------------------------------------------------------------------------------------------------ the file layer

// what Frequency reads of a SNP (Mutations::Read, src/mutations.cpp:229-430)
struct MutSnp {
  int pos = 0, tree = 0, branch = -1, branches = 0;
  bool flipped = false;
  float age_begin = 0.0f;
  std::string rs_id;
};

// `snp;pos;dist;rs_id;tree;branches;is_not_mapping;is_flipped;age_begin;age_end;alleles;[upstream;downstream;[freq;...]]`
int read_mut(const std::string &fn, std::vector<MutSnp> &snps) {
  const char *const format = "snp;pos;dist;rs_id;tree;branches;is_not_mapping;is_flipped;age_begin;age_end;...";
  return read_mut_lines(kMode, fn, format, nullptr, snps, [&fn](std::vector<std::string> &col, MutSnp &m, long long n) {
    if (col.back().empty()) col.pop_back();  // (what follows the last `;`; a last field without its `;` stays)
    int dist = 0, flipped = 0;
    bool ok = col.size() >= 10 && parse_int(col[1], &m.pos) && parse_int(col[2], &dist) && parse_int(col[4], &m.tree) &&
              parse_int(col[7], &flipped);
    if (ok) {
      m.rs_id = col[3];
      m.flipped = flipped != 0;
      char *end = nullptr;
      m.age_begin = (float)strtod(col[8].c_str(), &end);  // (std::stod into a float)
      ok = end != col[8].c_str();
      std::istringstream br(col[5]);
      for (std::string b; ok && br >> b;) {
        int v = 0;
        ok = parse_int(b, &v);
        if (m.branches++ == 0) m.branch = v;
      }
    }
    if (!ok) return RL_EFORMAT;
    if (col.size() > 13) {
      set_error("%s: %s: line %lld has population-frequency columns: annotated .mut files are not part of this build", kMode, fn.c_str(), n);
      return RL_EINVAL;
    }
    return RL_OK;
  });
}

// pos rs_id, the boundaries from the oldest to 0 with std::to_string (:497-508)
std::string header(const float *ep, int E, const char *tail) {
  std::string h = "pos rs_id ";
  for (int e = E - 1; e >= 0; e--) h += std::to_string(ep[e]) + " ";
  return h + tail;
}

}  // namespace
}  // namespace rl

using namespace rl;

extern "C" int rl_frequency_batch_trees(int N) { return N < 2 ? 0 : frequency_batch_trees(N); }

extern "C" int rl_frequency_trees(const int *parents, const double *branch_length, int N, int ntrees, const int *snp_tree,
                                  const int *snp_branch, int nsnps, const float *epochs, int nepochs, int device,
                                  int *freq, int *lin, unsigned char *marks, float *root_time, int *host_trees) {
  if (!parents || !branch_length || !snp_tree || !snp_branch || !epochs || !freq || !lin || !marks || !root_time ||
      !host_trees || ntrees < 0 || nsnps < 0) {
    set_error("rl_frequency_trees: bad arguments (ntrees=%d, nsnps=%d; no null pointers)", ntrees, nsnps);
    return RL_EINVAL;
  }
  if (N < 2) {
    set_error("rl_frequency_trees: N=%d: no branch below the root", N);
    return RL_EINVAL;
  }
  if (const int rc = check_epochs("rl_frequency_trees", epochs, nepochs, kFrequencyMaxEpochs)) return rc;
  return frequency_rows(parents, branch_length, N, ntrees, snp_tree, snp_branch, nsnps, epochs, nepochs, device, freq, lin,
                        marks, root_time, host_trees, "rl_frequency_trees", nullptr, nullptr);
}

extern "C" int rl_frequency_anc(const char *anc_path, const char *mut_path, const float *epochs, int nepochs, int device,
                                const char *freq_path, const char *lin_path, long long *rows_out, int *host_trees_out) {
  if (!anc_path || !mut_path || !epochs || !freq_path || !lin_path) return null_args("rl_frequency_anc");
  if (const int rc = check_epochs("rl_frequency_anc", epochs, nepochs, kFrequencyMaxEpochs)) return rc;
  const int E = nepochs;
  AncText anc(kMode);
  int rc = anc.open(anc_path);
  if (rc) return rc;
  if (anc.has_ages) {
    set_error("%s: %s has sample ages: the coordinates with sample ages are not part of this build", kMode, anc_path);
    return RL_EINVAL;
  }
  const int N = anc.N, root = 2 * N - 2;
  std::vector<MutSnp> mut;
  if ((rc = read_mut(mut_path, mut))) return rc;
  if (mut.back().tree >= anc.trees || mut.front().tree < 0) {
    set_error("%s: %s names tree %d, %s holds %d", kMode, mut_path, mut.front().tree < 0 ? mut.front().tree : mut.back().tree, anc_path, anc.trees);
    return RL_EINVAL;
  }
  std::ofstream os_freq(freq_path), os_lin(lin_path);
  if (os_freq.fail() || os_lin.fail()) {
    set_error("%s: error while opening file %s", kMode, os_freq.fail() ? freq_path : lin_path);
    return RL_EIO;
  }
  os_freq << header(epochs, E, "TreeFreq DataFreq\n");
  os_lin << header(epochs, E, "when_DAF_is_half when_mutation_has_freq2\n");

  // the trees that have a SNP the filter may keep (:539-554: one branch, not flipped; the age is compared with the
  // root's time once that is known) go up batch by batch with those SNPs; the rows come back in the .mut's order
  SnpTreeBatches w(N, frequency_batch_trees(N));
  std::vector<int> snp_tree, snp_branch, snp_id, freq, lin;
  std::vector<unsigned char> marks;
  std::vector<float> root_time(w.batch);
  long long rows = 0;
  int host_trees = 0;
  std::string out_freq, out_lin;
  const auto flush = [&]() -> int {
    const int held = (int)w.tree_id.size(), ns = (int)snp_id.size();
    freq.assign((size_t)ns * (E + 1), 0);
    lin.assign((size_t)ns * (E + 2), 0);
    marks.assign(ns, 0);
    int on_host = 0;
    const int r = frequency_rows(w.parents.data(), w.bl.data(), N, held, snp_tree.data(), snp_branch.data(), ns, epochs, E, device,
                                 freq.data(), lin.data(), marks.data(), root_time.data(), &on_host, anc_path, w.tree_id.data(),
                                 snp_id.data());
    if (r) return r;
    host_trees += on_host;
    out_freq.clear();
    out_lin.clear();
    for (int s = 0; s < ns; s++) {
      const MutSnp &m = mut[snp_id[s]];
      if (!marks[s] || !(m.age_begin <= root_time[snp_tree[s]])) continue;
      const std::string head = std::to_string(m.pos) + " " + m.rs_id + " ";
      out_freq += head;
      out_lin += head;
      for (int c = 0; c < E; c++) {
        out_freq += std::to_string(freq[(size_t)s * (E + 1) + c]) + " ";
        out_lin += std::to_string(lin[(size_t)s * (E + 2) + c]) + " ";
      }
      out_freq += " " + std::to_string(freq[(size_t)s * (E + 1) + E]) + " 0\n";  // DataFreq: no frequency columns
      out_lin += std::to_string(lin[(size_t)s * (E + 2) + E]) + " " + std::to_string(lin[(size_t)s * (E + 2) + E + 1]) + "\n";
      rows++;
    }
    os_freq << out_freq;
    os_lin << out_lin;
    snp_tree.clear(), snp_branch.clear(), snp_id.clear();
    return RL_OK;
  };
  const auto wanted = [&](size_t k) { return mut[k].branches == 1 && !mut[k].flipped; };
  const auto take = [&](size_t s, int slot) {
    if (!wanted(s)) return RL_OK;
    if (mut[s].branch < -1 || mut[s].branch > root) {
      set_error("%s: %s: SNP %zu is on branch %d of a tree with %zu nodes", kMode, mut_path, s, mut[s].branch, w.nodes);
      return RL_EINVAL;
    }
    snp_tree.push_back(slot);
    snp_branch.push_back(mut[s].branch);
    snp_id.push_back((int)s);
    return RL_OK;
  };
  if ((rc = w.walk(anc, mut.size(), [&](size_t k) { return mut[k].tree; }, wanted, take, flush))) return rc;
  os_freq.close();
  os_lin.close();
  if (os_freq.fail() || os_lin.fail()) {
    set_error("%s: writing %s failed", kMode, os_freq.fail() ? freq_path : lin_path);
    return RL_EIO;
  }
  if (rows_out) *rows_out = rows;
  if (host_trees_out) *host_trees_out = host_trees;
  return RL_OK;
}

// subtrees.cpp -- SubTreesForSubpopulation, host side (include/relate_amd.h has the definition; the reference:
// include/extract/CreateAncesTreeFileForSubpopulation.cpp, Tree::GetSubTree and Tree::GetCoordinates of src/anc.cpp,
// Sample::AssignPopOfInterest of src/sample.cpp).
//
// HostSubTree restates Tree::GetSubTree and Tree::GetCoordinates operation by operation -- the internal nodes in
// label order, a contracted node's branch length added onto the subtree node its child converts to, the times a float
// at every node of the SUBTREE -- and is the `device < 0` path and the authority the device (subtrees_kernels.hip) is
// held to, bit for bit.  This file also holds the groups of interest, the loop over the text .anc and the .mut of
// MakeAncesTreeFile with its mutation walk, the association of neighbouring subtrees (equivalent.cpp), the three
// output files and the C entry points.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "anc_text.h"
#include "coalrate.h"
#include "common.h"
#include "mut_text.h"
#include "subtrees.h"
#include "tree_host.h"

namespace rl {

namespace {

const char *const kMode = "SubTreesForSubpopulation";

// Tree::GetSubTree(std::vector<int>&, ...) (src/anc.cpp:655-738) and Tree::GetCoordinates (:525-565) on its result
struct HostSubTree : TreeTables {
  int M;
  const int *subpop;      // [M] rising
  const int *leaf_label;  // [N] k for subpop[k], -1 otherwise
  std::vector<int> left, right;  // the subtree's child_left / child_right
  HostSubTree(int n, int m, const int *subset, const int *labels)
      : TreeTables(n), M(m), subpop(subset), leaf_label(labels), left(2 * m - 1), right(2 * m - 1) {}

  // parent must have passed first_bad_node.  false: the reference's assert `node == 2*subpop.size()-1` fails
  bool run(const int *parent, const double *bl, int *sub_parent, double *sub_bl, float *coordinates, int *convert_index,
           int *number_in_subpop) {
    fill(parent);
    const int sub_nodes = 2 * M - 1;
    for (int v = 0; v < nodes; v++) convert_index[v] = -1;
    // GetNumberOfLeavesInSubpop (:583-603): children before their parent
    for (int v = 0; v < N; v++) number_in_subpop[v] = leaf_label[v] >= 0 ? 1 : 0;
    for (int v = N; v < nodes; v++) number_in_subpop[v] = number_in_subpop[first[v]] + number_in_subpop[second[v]];
    if (M >= N) {
      for (int v = 0; v < nodes; v++) {
        sub_parent[v] = parent[v];
        sub_bl[v] = bl[v];
        convert_index[v] = v;
        left[v] = v < N ? -1 : first[v];
        right[v] = v < N ? -1 : second[v];
      }
    } else {
      int node = 0;
      for (node = 0; node < M; node++) {
        sub_bl[node] = bl[subpop[node]];
        left[node] = right[node] = -1;
        convert_index[subpop[node]] = node;
      }
      for (int i = N; i < nodes; i++) {
        const int child_left = first[i], child_right = second[i];
        if (number_in_subpop[child_left] > 0 && number_in_subpop[child_right] > 0) {
          if (node == sub_nodes) return false;
          sub_bl[node] = bl[i];
          left[node] = convert_index[child_left];
          right[node] = convert_index[child_right];
          sub_parent[convert_index[child_left]] = node;
          sub_parent[convert_index[child_right]] = node;
          convert_index[i] = node;
          node++;
        } else if (number_in_subpop[child_left] > 0) {
          convert_index[i] = convert_index[child_left];
          sub_bl[convert_index[i]] += bl[i];
        } else if (number_in_subpop[child_right] > 0) {
          convert_index[i] = convert_index[child_right];
          sub_bl[convert_index[i]] += bl[i];
        }
      }
      if (node != sub_nodes) return false;
      sub_parent[node - 1] = -1;
    }
    // TraverseTreeToGetCoordinates: a subtree node's label is above its children's
    for (int v = 0; v < M; v++) coordinates[v] = 0.0f;
    for (int n = M; n < sub_nodes; n++)
      coordinates[n] = (float)std::max((double)coordinates[right[n]] + sub_bl[right[n]], (double)coordinates[left[n]] + sub_bl[left[n]]);
    return true;
  }
};

// N and the subset [M]: labels of leaves, rising.  labels [N]: the new label of every leaf, -1 outside the subset
int check_subset(const char *who, int N, const int *subset, int M, std::vector<int> &labels) {
  if (N < 2 || N > kSubtreesMaxN) {
    set_error("%s: trees of 2 <= N <= %d leaves (N=%d)", who, kSubtreesMaxN, N);
    return RL_EINVAL;
  }
  if (M < 2 || M > N) {
    set_error("%s: a subset of 2 <= M <= N leaves (M=%d, N=%d)", who, M, N);
    return RL_EINVAL;
  }
  labels.assign(N, -1);
  for (int k = 0; k < M; k++) {
    if (subset[k] < 0 || subset[k] >= N) {
      set_error("%s: entry %d of the subset is %d: not a leaf of a tree of %d leaves", who, k, subset[k], N);
      return RL_EINVAL;
    }
    if (k && subset[k] <= subset[k - 1]) {
      set_error("%s: entry %d of the subset is %d after %d: the labels must rise", who, k, subset[k], subset[k - 1]);
      return RL_EINVAL;
    }
    labels[subset[k]] = k;
  }
  return RL_OK;
}

// the subtrees of ntrees trees, on a device or on the host.  `where` names the trees' origin in a message, index0 the
// first tree's number there; labels: check_subset's
int subtrees_of(const char *where, long long index0, const int *parents, const double *bl, int N, int ntrees,
                const int *subset, const std::vector<int> &labels, int M, int device, int *sub_parent, double *sub_bl,
                float *sub_time, int *convert_index, int *number_in_subpop) {
  const size_t nodes = (size_t)2 * N - 1, sub = (size_t)2 * M - 1;
  int bad = -1;
  if (device >= 0) {
    const int rc = subtrees_device(parents, bl, N, ntrees, labels.data(), M, device, sub_parent, sub_bl, sub_time,
                                   convert_index, number_in_subpop, &bad);
    if (bad < 0) return rc;
  }
  HostSubTree host(N, M, subset, labels.data());
  std::vector<unsigned char> kids;
  for (int t = device >= 0 ? bad : 0; t < (device >= 0 ? bad + 1 : ntrees); t++) {
    const int *parent = parents + t * nodes;
    const double *b = bl + t * nodes;
    const std::string tree = std::string(where) + ": tree " + std::to_string(index0 + t);
    // (all 2N-1 lengths: the root's ends in the subtree root's)
    if (const int rc = check_tree(tree.c_str(), parent, b, N, 2 * N - 1, device >= 0, kids)) return rc;
    if (!host.run(parent, b, sub_parent + t * sub, sub_bl + t * sub, sub_time + t * sub, convert_index + t * nodes,
                  number_in_subpop + t * nodes)) {
      set_error("%s: the reference's assert `node == 2*subpop.size()-1` fails", tree.c_str());
      return RL_EINVAL;
    }
  }
  return RL_OK;
}

// Sample::AssignPopOfInterest (src/sample.cpp:106-171): the groups named in `pops` (comma separated, duplicates
// ignored, `All` for every group), sorted
int assign_pop_of_interest(const std::vector<std::string> &groups, const std::string &pops, std::vector<int> &of_interest) {
  of_interest.clear();
  if (pops == "All") {
    for (size_t g = 0; g < groups.size(); g++) of_interest.push_back((int)g);
    return RL_OK;
  }
  size_t i = 0;
  while (i < pops.size()) {
    std::string pop;
    while (i < pops.size() && pops[i] != ',') pop += pops[i++];
    i++;
    const auto it = std::find(groups.begin(), groups.end(), pop);
    if (it == groups.end()) {
      set_error("%s: group label `%s` does not exist in the .poplabels file", kMode, pop.c_str());
      return RL_EINVAL;
    }
    const int index = (int)(it - groups.begin());
    if (std::find(of_interest.begin(), of_interest.end(), index) == of_interest.end()) of_interest.push_back(index);
  }
  std::sort(of_interest.begin(), of_interest.end());
  return RL_OK;
}

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace
}  // namespace rl

using namespace rl;

extern "C" int rl_subtrees_batch_trees(int N) { return N < 2 ? 0 : subtrees_batch_trees(N); }

extern "C" int rl_subtrees_trees(const int *parents, const double *branch_length, int N, int ntrees, const int *subset,
                                 int M, int device, int *sub_parent, double *sub_bl, float *sub_time, int *convert_index,
                                 int *number_in_subpop) {
  if (!parents || !branch_length || !subset || !sub_parent || !sub_bl || !sub_time || !convert_index || !number_in_subpop ||
      ntrees < 0) {
    set_error("rl_subtrees_trees: bad arguments (ntrees=%d; no null pointers)", ntrees);
    return RL_EINVAL;
  }
  std::vector<int> labels;
  if (const int rc = check_subset("rl_subtrees_trees", N, subset, M, labels)) return rc;
  return subtrees_of("rl_subtrees_trees", 0, parents, branch_length, N, ntrees, subset, labels, M, device, sub_parent,
                     sub_bl, sub_time, convert_index, number_in_subpop);
}

extern "C" int rl_subtrees_poplabels(const char *poplabels_path, const char *pops_or_null, int *group_of_haplotype,
                                     int *num_haplotypes, int *of_interest, int *num_groups, char *names, int *names_bytes) {
  if (!poplabels_path || !num_haplotypes || !num_groups || !names_bytes) return null_args("rl_subtrees_poplabels");
  std::vector<std::string> groups;
  std::vector<int> goh, goi;
  if (const int rc = read_poplabels(kMode, poplabels_path, groups, goh)) return rc;
  if (pops_or_null)
    if (const int rc = assign_pop_of_interest(groups, pops_or_null, goi)) return rc;
  std::string joined;
  for (const std::string &g : groups) joined += g + "\n";
  const int room_h = *num_haplotypes, room_g = *num_groups, room_n = *names_bytes;
  *num_haplotypes = (int)goh.size(), *num_groups = (int)groups.size(), *names_bytes = (int)joined.size();
  if (group_of_haplotype && room_h >= (int)goh.size()) memcpy(group_of_haplotype, goh.data(), goh.size() * sizeof(int));
  if (of_interest && room_g >= (int)groups.size())
    for (size_t g = 0; g < groups.size(); g++) of_interest[g] = std::find(goi.begin(), goi.end(), (int)g) != goi.end();
  if (names && room_n >= (int)joined.size()) memcpy(names, joined.data(), joined.size());
  return RL_OK;
}

extern "C" int rl_subtrees_rewrite(const char *anc_in, const char *mut_in, const char *anc_out, const char *mut_out) {
  if (!anc_in || !mut_in || !anc_out || !mut_out) return null_args("rl_subtrees_rewrite");
  AncText anc(kMode);
  int rc = anc.open(anc_in);
  if (rc) return rc;
  if (anc.has_ages) {
    set_error("%s: %s has sample ages: sample ages are not part of this build", kMode, anc_in);
    return RL_EINVAL;
  }
  const int nodes = 2 * anc.N - 1;
  std::vector<AncTree> trees(anc.trees);
  for (int t = 0; t < anc.trees; t++) {
    AncTree &a = trees[t];
    a.parent.resize(nodes), a.branch_length.resize(nodes), a.num_events.resize(nodes), a.snp_begin.resize(nodes), a.snp_end.resize(nodes);
    if ((rc = anc.next(t, a.parent.data(), a.branch_length.data(), &a.pos, a.num_events.data(), a.snp_begin.data(), a.snp_end.data()))) return rc;
  }
  std::string header;
  std::vector<MutFull> rows;
  if ((rc = read_mut_full(kMode, mut_in, header, rows))) return rc;
  if ((rc = write_anc_text(kMode, anc_out, anc.N, trees))) return rc;
  return write_mut_text(kMode, mut_out, header, rows);
}

extern "C" int rl_subtrees_files(const char *anc_path, const char *mut_path, const char *poplabels_path, const char *pops,
                                 const char *out_prefix, int device, rl_subtrees_summary *summary) {
  if (!anc_path || !mut_path || !poplabels_path || !pops || !out_prefix) return null_args("rl_subtrees_files");
  double t_mark = now(), t_parse = 0.0, t_subtrees = 0.0, t_walk = 0.0, t_assoc = 0.0, t_write = 0.0;
  const auto lap = [&](double &into) {
    const double t = now();
    into += t - t_mark;
    t_mark = t;
  };
  // ---- the subset (Sample::Read, Sample::AssignPopOfInterest, Tree::GetSubTree(Sample&, ...) src/anc.cpp:631-652)
  std::vector<std::string> groups;
  std::vector<int> group_of_haplotype, of_interest;
  int rc = read_poplabels(kMode, poplabels_path, groups, group_of_haplotype);
  if (rc) return rc;
  if ((rc = assign_pop_of_interest(groups, pops, of_interest))) return rc;
  std::vector<int> subset;
  for (size_t hap = 0; hap < group_of_haplotype.size(); hap++)
    if (std::find(of_interest.begin(), of_interest.end(), group_of_haplotype[hap]) != of_interest.end()) subset.push_back((int)hap);
  const int M = (int)subset.size();

  AncText anc(kMode);
  if ((rc = anc.open(anc_path))) return rc;
  if (anc.has_ages) {
    set_error("%s: %s has sample ages: subtrees with sample ages are not part of this build", kMode, anc_path);
    return RL_EINVAL;
  }
  const int N = anc.N;
  if ((int)group_of_haplotype.size() != N) {
    set_error("%s: number of haplotypes in %s (%d) does not match the %zu haplotypes of %s", kMode, anc_path, N,
              group_of_haplotype.size(), poplabels_path);
    return RL_EINVAL;
  }
  std::vector<int> labels;
  if ((rc = check_subset(kMode, N, subset.data(), M, labels))) return rc;
  std::string header;
  std::vector<MutFull> mut;
  if ((rc = read_mut_full(kMode, mut_path, header, mut))) return rc;
  std::vector<MutRow> rows(mut.size());  // (AncMutIterators keeps a .mut of its own: the walk below rewrites `mut`)
  for (size_t k = 0; k < mut.size(); k++) rows[k] = MutRow{mut[k].pos, mut[k].dist, mut[k].tree};
  lap(t_parse);

  // ---- MakeAncesTreeFile (CreateAncesTreeFileForSubpopulation.cpp:115-233), the trees a batch at a time
  const int nodes = 2 * N - 1, sub = 2 * M - 1, root = sub - 1, batch = subtrees_batch_trees(N);
  const int G = (int)groups.size(), L = (int)mut.size();
  // (the walk ends when the .mut does: no tree after the last SNP's is read)
  const int trees_to_read = (int)std::min<long long>(anc.trees, (long long)rows.back().tree + 1);
  std::vector<int> parents((size_t)batch * nodes), conv((size_t)batch * nodes), count((size_t)batch * nodes), sub_parent((size_t)batch * sub);
  std::vector<double> bl((size_t)batch * nodes), sub_bl((size_t)batch * sub);
  std::vector<float> sub_time((size_t)batch * sub), num_events(sub);
  std::vector<AncTree> seq;
  std::vector<int> include_snp;
  TreeTables tables(N);
  Persistence persistence(rows);
  int count_tree = 0, snp = 0;
  bool walk_over = false;
  for (int t0 = 0; t0 < trees_to_read && !walk_over; t0 += batch) {
    const int n = std::min(batch, trees_to_read - t0);
    for (int k = 0; k < n; k++)
      if ((rc = anc.next(t0 + k, &parents[(size_t)k * nodes], &bl[(size_t)k * nodes]))) return rc;
    lap(t_parse);
    if ((rc = subtrees_of(anc_path, t0, parents.data(), bl.data(), N, n, subset.data(), labels, M, device, sub_parent.data(),
                          sub_bl.data(), sub_time.data(), conv.data(), count.data())))
      return rc;
    lap(t_subtrees);
    for (int k = 0; k < n; k++) {
      const float num_bases_tree_persists = (float)persistence.next(count_tree);
      if (!(num_bases_tree_persists >= 0.0)) {
        walk_over = true;
        break;
      }
      const int *convert_index = &conv[(size_t)k * nodes], *number_in_subpop = &count[(size_t)k * nodes];
      const int *sp = &sub_parent[(size_t)k * sub];
      const float *coordinates = &sub_time[(size_t)k * sub];
      const int pos = (int)include_snp.size();
      std::fill(num_events.begin(), num_events.end(), 0.0f);
      int num_snps_mapped_onto_tree = 0;
      while (mut[snp].tree < count_tree) {
        snp++;
        if (snp == L) break;
      }
      if (snp == L) {
        walk_over = true;
        break;
      }
      if (mut[snp].tree != count_tree) {
        set_error("%s: %s: tree %d, SNP %d: the reference's assert `mut.info[snp].tree == count_tree` fails: the SNP lies on tree %d, tree %d has no SNP in %s",
                  kMode, anc_path, count_tree, snp, mut[snp].tree, count_tree, mut_path);
        return RL_EINVAL;
      }
      const bool with_freq = (int)mut[snp].freq.size() == G;
      while (mut[snp].tree == count_tree) {
        MutFull &m = mut[snp];
        bool take = true;
        if (with_freq) {
          float freq = 0.0f;
          for (int g : of_interest) {
            if (g >= (int)m.freq.size()) {
              set_error("%s: %s: tree %d, SNP %d: %zu frequency columns, the first SNP of the tree has %d", kMode, mut_path, count_tree, snp, m.freq.size(), G);
              return RL_EFORMAT;
            }
            freq += m.freq[g];
            if (freq > 0.0) break;
          }
          take = freq > 0.0;
        }
        if (take) {
          for (int b : m.branch)
            if (b < 0 || b >= nodes) {
              set_error("%s: %s: tree %d, SNP %d: branch %d is not a node of a tree of %d leaves", kMode, mut_path, count_tree, snp, b, N);
              return RL_EINVAL;
            }
          if (m.branch.size() == 1) {
            const int branch = convert_index[m.branch[0]];
            if (branch != -1 && branch != root && number_in_subpop[m.branch[0]] > 0) {
              num_snps_mapped_onto_tree++;
              include_snp.push_back(snp);
              m.age_begin = coordinates[branch];
              m.age_end = coordinates[sp[branch]];
              m.tree = (int)seq.size();
            }
          }
          for (int &b : m.branch) {
            const int branch = convert_index[b];
            if (branch != -1) {
              num_events[branch] += 1.0 / ((float)m.branch.size());
              b = branch;
            }
          }
        }
        snp++;
        if (snp == L) break;
      }
      if (num_snps_mapped_onto_tree != 0) {
        seq.emplace_back();
        AncTree &a = seq.back();
        a.pos = pos;
        a.parent.assign(sp, sp + sub);
        a.branch_length.assign(&sub_bl[(size_t)k * sub], &sub_bl[(size_t)k * sub] + sub);
        a.num_events = num_events;
        a.snp_begin.assign(sub, pos);
        a.snp_end.assign(sub, 0);
        // the subtree's child_left / child_right are the original node's, converted: of the nodes that convert to a
        // subtree node the one that was kept has the lowest label
        a.child_left.assign(sub, -1);
        a.child_right.assign(sub, -1);
        tables.fill(&parents[(size_t)k * nodes]);
        for (int i = N; i < nodes; i++) {
          const int s = convert_index[i];
          if (s >= M && a.child_left[s] == -1) {
            a.child_left[s] = convert_index[tables.first[i]];
            a.child_right[s] = convert_index[tables.second[i]];
          }
        }
      }
      count_tree++;
      if (snp == L) {
        walk_over = true;
        break;
      }
    }
    lap(t_walk);
  }
  if (seq.empty()) {
    set_error("%s: no SNP of %s maps onto a subtree of %s for %s: no tree is kept", kMode, mut_path, anc_path, pops);
    return RL_EINVAL;
  }
  // a tree extends to one position before the next kept one, the last to the last kept SNP (:134-139, :229-232)
  for (size_t k = 0; k < seq.size(); k++)
    seq[k].snp_end.assign(sub, (k + 1 < seq.size() ? seq[k + 1].pos : (int)include_snp.size()) - 1);
  lap(t_walk);

  // ---- BranchAssociation of neighbours and AssociateTrees (:235-277)
  associate_sequence(seq, M);
  lap(t_assoc);

  // ---- the three files (:277, :331-384)
  const std::string out(out_prefix);
  if ((rc = write_anc_text(kMode, out + ".anc", M, seq))) return rc;
  {
    std::ifstream is_pops;
    if ((rc = open_text(kMode, poplabels_path, is_pops))) return rc;
    std::ofstream os_pops(out + ".poplabels");
    std::string line, id, pop;
    getline(is_pops, line);
    os_pops << line << "\n";
    while (getline(is_pops, line)) {
      std::istringstream ls(line);
      if (!(ls >> id >> pop)) continue;
      for (int g : of_interest)
        if (pop == groups[g]) {
          os_pops << line << "\n";
          break;
        }
    }
    os_pops.close();
    if (os_pops.fail()) {
      set_error("%s: writing %s.poplabels failed", kMode, out.c_str());
      return RL_EIO;
    }
  }
  std::vector<MutFull> mut_subset(include_snp.size());
  std::string subset_header = "snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;ancestral_allele/alternative_allele;upstream_allele;downstream_allele;";
  for (int g : of_interest) subset_header += groups[g] + ";";
  for (size_t k = 0; k < include_snp.size(); k++) {
    mut_subset[k] = mut[include_snp[k]];
    // the distances of the dropped SNPs up to the next kept one
    const int next = k + 1 < include_snp.size() ? include_snp[k + 1] : L;
    for (int tmp_snp = include_snp[k] + 1; tmp_snp < next; tmp_snp++) mut_subset[k].dist += mut[tmp_snp].dist;
    if ((int)mut[k].freq.size() == G) {  // (row k of the .mut, not row include_snp[k]: :373)
      const std::vector<int> &from = mut[include_snp[k]].freq;
      mut_subset[k].freq.resize(of_interest.size());
      for (size_t j = 0; j < of_interest.size(); j++) {
        if (of_interest[j] >= (int)from.size()) {
          set_error("%s: %s: SNP %d has %zu frequency columns, SNP %zu has %d", kMode, mut_path, include_snp[k], from.size(), k, G);
          return RL_EFORMAT;
        }
        mut_subset[k].freq[j] = from[of_interest[j]];
      }
    }
  }
  if ((rc = write_mut_text(kMode, out + ".mut", subset_header, mut_subset))) return rc;
  lap(t_write);
  if (timing_level() >= 1)
    fprintf(stderr, "[%s] parsing %.3f s, subtrees (%s) %.3f s, mutations mapped %.3f s, branches associated %.3f s, files written %.3f s\n",
            kMode, t_parse, device >= 0 ? "device" : "host", t_subtrees, t_walk, t_assoc, t_write);
  if (summary) {
    summary->trees_read = count_tree;
    summary->trees_kept = (int)seq.size();
    summary->snps_read = L;
    summary->snps_kept = (int)include_snp.size();
    summary->M = M;
    summary->N = N;
    summary->has_freq = mut[0].freq.size() > 0;
  }
  return RL_OK;
}

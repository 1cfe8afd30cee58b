// mutctx.cpp -- MutationRateWithContext and FinalizeMutationRate, host side (include/relate_amd.h has the definition;
// the reference: include/evaluate/mutation_rate/RelateMutationRate.cpp, --mode WithContextForChromosome / Finalize).
//
// This file holds the category table (:746-794), the two FASTA readers and CountBasesByType (:40-260) restated phase by
// phase over indices, the loop over the SNPs (:829-908) -- qualification, category, the clamp of age_end to the root's
// time, the numerator and, on the `device < 0` path, the opportunity in the reference's order, which is the authority
// the device (mutctx_kernels.hip) is held to, bit for bit --, the writers and readers of _mut.bin / _opp.bin, the sum
// over chromosomes (:445-576), the writer of .rate (:344-443) and the C entry points.  The per-tree branch lengths
// and the root's time come from mutrate.cpp's host twin or from mutrate_kernels.hip.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "anc_text.h"
#include "common.h"
#include "mut_text.h"
#include "mutctx.h"
#include "tree_host.h"

namespace rl {

namespace {

const char *const kMode = "MutationRateWithContext";
const char *const kFinalize = "FinalizeMutationRate";
constexpr int C96 = kMutctxCategories;

// :746-794: 192 keys `upstream downstream ancestral derived` onto 96 indices, a pattern and its reverse complement
// onto the same one
const std::map<std::string, int> &category_table() {
  static const std::map<std::string, int> table = [] {
    std::map<std::string, int> m;
    const std::string alphabet = "ACGT", reverse_alphabet = "TGCA";
    int index = 0;
    for (char s1 : alphabet)
      for (char s2 : alphabet) {
        const std::string pattern = std::string(1, s1) + s2;
        for (const char *t : {"CA", "CG", "CT", "AT", "AG", "AC"}) m[pattern + t] = index++;
      }
    index = 0;
    for (char s1 : reverse_alphabet)
      for (char s2 : reverse_alphabet) {
        const std::string reverse_pattern = std::string(1, s2) + s1;
        for (const char *t : {"GT", "GC", "GA", "TA", "TC", "TG"}) m[reverse_pattern + t] = index++;
      }
    return m;
  }();
  return table;
}

// :397-410: the header of .rate, in index order
std::vector<std::string> category_names() {
  std::vector<std::string> names;
  const std::string alphabet = "ACGT";
  for (char s1 : alphabet)
    for (char s2 : alphabet)
      for (const char *t : {"C/A", "C/G", "C/T", "A/T", "A/G", "A/C"}) names.push_back(std::string(1, s1) + t + s2);
  return names;
}

// IsCharNucl (:21-37) as an index into "ACGT", -1 for 'N'
inline int nucl(char c) {
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
  }
  return -1;
}

// [up][down][ancestral][derived] -> the category, from the table
struct Cat4 {
  int at[4][4][4][4];
  Cat4() {
    const std::string nu = "ACGT";
    for (int a = 0; a < 4; a++)
      for (int b = 0; b < 4; b++)
        for (int c = 0; c < 4; c++)
          for (int d = 0; d < 4; d++) {
            const auto it = category_table().find(std::string() + nu[a] + nu[b] + nu[c] + nu[d]);
            at[a][b][c][d] = it == category_table().end() ? -1 : it->second;
          }
  }
};

// the ancestor (:49-60): the first line skipped, the rest concatenated as it is.  upper: the mask (fasta::Read,
// src/data.cpp:628-646), every character through toupper
int read_fasta(const std::string &fn, bool upper, std::string &seq) {
  std::ifstream is;
  if (const int rc = open_text(kMode, fn, is)) return rc;
  std::string line;
  getline(is, line);
  seq.clear();
  while (getline(is, line)) {
    if (upper)
      for (char &c : line) c = (char)std::toupper((unsigned char)c);
    seq += line;
  }
  return RL_OK;
}

// CountBasesByType (:62-260) over indices.  ancestor: case kept; mask: upper case; pos [M]: the position list;
// snp_pos, one_branch [L]: the .mut's.  cnt [L][96], zeroed here.
//
// The reference moves it_mask, it_ancestor and p together, so p is the index into both sequences; it_start / it_end
// are the ends of the window whose non-'P' characters `d` counts.
//   head   (:105-112) from p = 0 until p is 1001 or the first SNP's position: the window's right end moves, nothing
//          is counted.  The two loops that follow (:114-164) never run: each repeats a condition the head ended on.
//   main   (:168-213) while the window's right end is inside the mask and the SNP is not the last: threshold 2000.
//   tail   (:215-258) while p is inside and the SNP is not the last: only the left end moves, threshold 0.5 * 2000.
// The last SNP's row stays zero.  A read outside the sequences or the lists is RL_EINVAL -- except pos[-1] at :121 /
// :177 / :227, which is 0 (the upper half of the allocator's size word in front of the vector's storage).
int count_bases(std::string ancestor, std::string mask, const int *pos, long long M, const int *snp_pos,
                const unsigned char *one_branch, long long L, uint32_t *cnt) {
  static const Cat4 cat;
  const int mask_threshold = 2000;
  std::fill(cnt, cnt + (size_t)L * C96, 0u);
  if (mask.size() < ancestor.size()) mask.resize(ancestor.size(), 'N');
  else ancestor.resize(mask.size(), 'N');
  const long long S = (long long)mask.size();
  if (S == 0) {
    set_error("%s: the mask and the ancestor are empty: the reference reads in front of its sequences", kMode);
    return RL_EINVAL;
  }
  const auto out_of_sequence = [&](const char *what, long long at, long long snp) {
    set_error("%s: SNP %lld (position %d): the reference reads %s at %lld, outside its sequences of %lld bases", kMode, snp,
              snp_pos[snp], what, at, S);
    return RL_EINVAL;
  };
  const auto out_of_list = [&](long long snp, long long p) {
    set_error("%s: SNP %lld (position %d), base %lld: the reference reads past the end of its list of %lld positions", kMode,
              snp, snp_pos[snp], p, M);
    return RL_EINVAL;
  };
  long long i_start = 0, i_end = std::min(S, (long long)1001);
  int d = 0;  // d_num_nonpass_vincity
  for (long long i = 0; i < i_end; i++) d += mask[i] != 'P';
  i_end--;
  long long p = 0, snp = 0, j = 0;
  // ---- head
  while (i_end != S && p != 1001 && p < snp_pos[snp]) {
    i_end++;
    if (i_end >= S) return out_of_sequence("the mask", i_end, snp);
    if (mask[i_end] != 'P') d++;
    p++;
  }
  // one base: the tests of :121-138 (= :177-197, :227-244) and the advance of the SNP and of the list (:140-147)
  // 0: go on; 1: the SNPs are used up (break); 2: refused, the message is set
  const auto step = [&](double threshold) -> int {
    const long long before = j == 0 ? 0 : pos[j - 1];
    if ((double)p >= 0.5 * (double)(pos[j] + before)) {
      if (j + 1 >= M) return out_of_list(snp, p), 2;
      if ((double)p < 0.5 * (double)((long long)pos[j] + pos[j + 1])) {
        if (p < 0 || p >= S) return out_of_sequence("the mask", p, snp), 2;
        if (mask[p] == 'P' && (double)d <= threshold && one_branch[snp]) {
          if (p - 1 < 0) return out_of_sequence("the ancestor", p - 1, snp), 2;
          const int up = nucl(ancestor[p - 1]);
          if (up >= 0) {
            if (p + 1 >= S) return out_of_sequence("the ancestor", p + 1, snp), 2;
            const int down = nucl(ancestor[p + 1]), a = nucl(ancestor[p]);
            if (down >= 0 && a >= 0)
              for (int to = 0; to < 4; to++)
                if (to != a) cnt[(size_t)snp * C96 + cat.at[up][down][a][to]]++;
          }
        }
      }
    }
    if (j + 1 >= M) return out_of_list(snp, p), 2;
    if ((double)p >= 0.5 * (double)((long long)pos[j + 1] + pos[j])) {
      snp++;
      if (snp == L) return 1;
    }
    while (pos[j] < snp_pos[snp]) {
      j++;
      if (j >= M) return out_of_list(snp, p), 2;
    }
    return 0;
  };
  // ---- main
  while (i_end != S - 1 && snp != L - 1) {
    if (i_start >= S || i_end + 1 >= S) return out_of_sequence("the mask", std::max(i_start, i_end + 1), snp);
    if (mask[i_start] != 'P') d--;
    i_start++;
    i_end++;
    if (mask[i_end] != 'P') d++;
    const int r = step((double)mask_threshold);
    if (r == 2) return RL_EINVAL;
    if (r == 1 || snp == L - 1) break;
    p++;
  }
  // ---- tail
  while (p != S - 1 && snp != L - 1) {
    if (i_start >= S) return out_of_sequence("the mask", i_start, snp);
    if (mask[i_start] != 'P') d--;
    i_start++;
    const int r = step(0.5 * mask_threshold);
    if (r == 2) return RL_EINVAL;
    if (r == 1) break;
    p++;
  }
  return RL_OK;
}

// :842-848: both flanks not `NA`, alleles `X/Y` of three characters, X != Y, both in ACGT
bool qualifies(const MutFull &m) {
  const std::string &t = m.mutation_type;
  const auto base = [](char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; };
  return m.upstream_base != "NA" && m.downstream_base != "NA" && t.size() == 3 && t[0] != t[2] && base(t[0]) && base(t[2]);
}

// :851-853: a key the map lacks gets 0 (operator[])
int category_of(const MutFull &m) {
  const auto it = category_table().find(m.upstream_base + m.downstream_base + m.mutation_type[0] + m.mutation_type[2]);
  return it == category_table().end() ? 0 : it->second;
}

// the numerator of one qualifying SNP (:855-886), added to mutation [E][96]
int add_mutation(const char *mut_path, size_t snp, const MutFull &m, int ind, float root, const double *epochs, int E,
                 double *mutation) {
  int ep = 0;
  while (epochs[ep] <= m.age_begin) {
    ep++;
    if (ep == E) break;
  }
  ep--;
  if (ep < 0) {
    set_error("%s: %s: SNP %zu has age_begin %g below 0: the reference aborts on this input", kMode, mut_path, snp, (double)m.age_begin);
    return RL_EINVAL;
  }
  const float age_end = std::min(m.age_end, root);
  if (!(age_end < epochs[E - 1]) || ep + 1 >= E) {
    set_error("%s: %s: SNP %zu: age_begin %g, age_end %g (the root's time: %g) are not below the last epoch boundary %g: the reference aborts on this input",
              kMode, mut_path, snp, (double)m.age_begin, (double)m.age_end, (double)root, epochs[E - 1]);
    return RL_EINVAL;
  }
  const double branch_length = age_end - m.age_begin;  // (a float difference)
  double *col = mutation + ind;
  if (age_end <= epochs[ep + 1]) {
    col[(size_t)ep * C96] += 1.0;
  } else {
    col[(size_t)ep * C96] += (epochs[ep + 1] - m.age_begin) / branch_length;
    ep++;
    while (epochs[ep + 1] <= age_end) {  // (age_end is below the last boundary)
      col[(size_t)ep * C96] += (epochs[ep + 1] - epochs[ep]) / branch_length;
      ep++;
    }
    col[(size_t)ep * C96] += (age_end - epochs[ep]) / branch_length;
  }
  return RL_OK;
}

// the opportunity of a batch on the host (:888-893): SNP by SNP, epoch by epoch, category by category
void add_opportunity(const double *lengths, int E, const int *snp_tree, const uint32_t *counts, long long nsnps, double *opp) {
  for (long long s = 0; s < nsnps; s++) {
    const double *in_epoch = lengths + (size_t)snp_tree[s] * E;
    const uint32_t *row = counts + (size_t)s * C96;
    for (int e = 0; e < E; e++) {
      const double bl = in_epoch[e];
      for (int c = 0; c < C96; c++) opp[(size_t)e * C96 + c] += bl * (double)row[c];
    }
  }
}

// the trees and SNPs of one call, batch by batch, on the host or the device
struct Adder {
  int N, E, device;
  const double *epochs;
  MutctxDevice *dev = nullptr;
  std::vector<double> lengths, opp;
  Adder(int n, const double *ep, int e, int dv) : N(n), E(e), device(dv), epochs(ep) {}
  ~Adder() {
    if (dev) mutctx_device_free(dev);
  }
  int begin() {
    if (N < 2 || N > kMutrateMaxN) {
      set_error("rl_mutctx_trees: trees of 2 <= N <= %d leaves (N=%d)", kMutrateMaxN, N);
      return RL_EINVAL;
    }
    if (device >= 0) return mutctx_device_begin(&dev, N, epochs, E, device);
    opp.assign((size_t)E * C96, 0.0);
    return RL_OK;
  }
  // ntrees <= mutrate_batch_trees(N); roots [ntrees].  Nothing of a batch with a refused tree is added
  int add(const int *parents, const double *bl, int ntrees, const int *snp_tree, const uint32_t *counts, long long nsnps,
          float *roots, const char *where, const int *tree_id) {
    if (device >= 0) {
      int bad = -1;
      const int rc = mutctx_device_add(dev, parents, bl, ntrees, snp_tree, counts, nsnps, roots, &bad);
      if (rc && bad >= 0) {  // name it: the host's checks, the device's verdict
        const size_t nodes = (size_t)2 * N - 1;
        std::vector<double> row(E);
        const int id = tree_id ? tree_id[bad] : bad;
        return mutrate_host_rows(parents + bad * nodes, bl + bad * nodes, N, 1, epochs, E, row.data(), nullptr, where, &id, true);
      }
      return rc;
    }
    lengths.assign((size_t)ntrees * E, 0.0);
    if (const int rc = mutrate_host_rows(parents, bl, N, ntrees, epochs, E, lengths.data(), roots, where, tree_id)) return rc;
    add_opportunity(lengths.data(), E, snp_tree, counts, nsnps, opp.data());
    return RL_OK;
  }
  int finish(double *opportunity, double *seconds) {
    if (seconds) std::fill(seconds, seconds + 3, 0.0);
    if (device >= 0) {
      if (seconds) mutctx_device_seconds(dev, seconds);
      return mutctx_device_finish(dev, opportunity);
    }
    std::copy(opp.begin(), opp.end(), opportunity);
    return RL_OK;
  }
};

// ------------------------------------------------------------------------------------------------ the .bin files

int write_matrix(FILE *fp, int E, const double *m) {
  const uint64_t rows = (uint64_t)E, cols = C96;  // CollapsedMatrix::DumpToFile (src/collapsed_matrix.hpp:204-213)
  return fwrite(&rows, 8, 1, fp) == 1 && fwrite(&cols, 8, 1, fp) == 1 && fwrite(m, 8, (size_t)E * C96, fp) == (size_t)E * C96;
}

// E < 0: take the rows from the file (at most kMutrateMaxEpochs)
int read_matrix(const char *who, const std::string &fn, FILE *fp, int E, std::vector<double> &m) {
  uint64_t rows = 0, cols = 0;
  if (fread(&rows, 8, 1, fp) != 1 || fread(&cols, 8, 1, fp) != 1) {
    set_error("%s: %s ends before its matrix", who, fn.c_str());
    return RL_EFORMAT;
  }
  if (cols != (uint64_t)C96 || rows != (uint64_t)E) {
    set_error("%s: %s holds a matrix of %llu x %llu, not %d x %d", who, fn.c_str(), (unsigned long long)rows, (unsigned long long)cols, E, C96);
    return RL_EFORMAT;
  }
  m.resize((size_t)E * C96);
  if (fread(m.data(), 8, m.size(), fp) != m.size()) {
    set_error("%s: %s ends inside its matrix", who, fn.c_str());
    return RL_EFORMAT;
  }
  return RL_OK;
}

struct File {
  FILE *fp = nullptr;
  ~File() {
    if (fp) fclose(fp);
  }
  int open(const char *who, const std::string &fn, const char *how) {
    fp = fopen(fn.c_str(), how);
    if (!fp) {
      set_error("%s: failed to open file %s", who, fn.c_str());
      return RL_EIO;
    }
    return RL_OK;
  }
  int close(const char *who, const std::string &fn) {
    const int r = fclose(fp);
    fp = nullptr;
    if (r) {
      set_error("%s: writing %s failed", who, fn.c_str());
      return RL_EIO;
    }
    return RL_OK;
  }
};

int write_pair(const char *who, const std::string &prefix, const double *epochs, int E, const double *mutation,
               const double *opportunity) {
  const std::string fm = prefix + "_mut.bin", fo = prefix + "_opp.bin";
  File a, b;
  if (const int rc = a.open(who, fm, "wb")) return rc;
  if (fwrite(&E, 4, 1, a.fp) != 1 || fwrite(epochs, 8, (size_t)E, a.fp) != (size_t)E || !write_matrix(a.fp, E, mutation)) {
    set_error("%s: writing %s failed", who, fm.c_str());
    return RL_EIO;
  }
  if (const int rc = a.close(who, fm)) return rc;
  if (const int rc = b.open(who, fo, "wb")) return rc;
  if (!write_matrix(b.fp, E, opportunity)) {
    set_error("%s: writing %s failed", who, fo.c_str());
    return RL_EIO;
  }
  return b.close(who, fo);
}

int read_pair(const char *who, const std::string &prefix, std::vector<double> &epochs, std::vector<double> &mutation,
              std::vector<double> &opportunity) {
  const std::string fm = prefix + "_mut.bin", fo = prefix + "_opp.bin";
  File a, b;
  if (const int rc = a.open(who, fm, "rb")) return rc;
  int E = 0;
  if (fread(&E, 4, 1, a.fp) != 1 || E < 2 || E > kMutrateMaxEpochs) {
    set_error("%s: %s does not start with a number of epochs between 2 and %d", who, fm.c_str(), kMutrateMaxEpochs);
    return RL_EFORMAT;
  }
  epochs.resize(E);
  if (fread(epochs.data(), 8, (size_t)E, a.fp) != (size_t)E) {
    set_error("%s: %s ends inside its epochs", who, fm.c_str());
    return RL_EFORMAT;
  }
  if (const int rc = read_matrix(who, fm, a.fp, E, mutation)) return rc;
  if (const int rc = b.open(who, fo, "rb")) return rc;
  return read_matrix(who, fo, b.fp, E, opportunity);
}

}  // namespace
}  // namespace rl

using namespace rl;

extern "C" int rl_mutctx_category_names(char *names, int *bytes) {
  if (!bytes) return null_args("rl_mutctx_category_names");
  std::string all;
  for (const std::string &n : category_names()) all += n + "\n";
  const int room = *bytes;
  *bytes = (int)all.size() + 1;
  if (!names || room < *bytes) {
    set_error("rl_mutctx_category_names: %d bytes, room for %d", *bytes, names ? room : 0);
    return RL_EINVAL;
  }
  memcpy(names, all.c_str(), all.size() + 1);
  return RL_OK;
}

extern "C" int rl_mutctx_category(const char *key) {
  if (!key) return -1;
  const auto it = category_table().find(key);
  return it == category_table().end() ? -1 : it->second;
}

extern "C" int rl_mutctx_count_bases(const char *ancestor_path, const char *mask_path, const int *pos, long long npos,
                                     const int *snp_pos, const unsigned char *one_branch, long long nsnps,
                                     uint32_t *counts) {
  if (!ancestor_path || !mask_path || !pos || !snp_pos || !one_branch || !counts) return null_args("rl_mutctx_count_bases");
  if (npos < 1 || nsnps < 1) {
    set_error("rl_mutctx_count_bases: %lld positions, %lld SNPs: at least one of each", npos, nsnps);
    return RL_EINVAL;
  }
  for (long long j = 0; j < npos; j++)
    if (pos[j] < 0 || pos[j] > (1 << 30)) {
      set_error("rl_mutctx_count_bases: position %lld of the list is %d: 0 <= position <= 2^30", j, pos[j]);
      return RL_EINVAL;
    }
  std::string ancestor, mask;
  if (const int rc = read_fasta(ancestor_path, false, ancestor)) return rc;
  if (const int rc = read_fasta(mask_path, true, mask)) return rc;
  return count_bases(std::move(ancestor), std::move(mask), pos, npos, snp_pos, one_branch, nsnps, counts);
}

extern "C" int rl_mutctx_trees(const int *parents, const double *branch_length, int N, int ntrees, const int *snp_tree,
                               const uint32_t *snp_counts, long long nsnps, const double *epochs, int nepochs, int device,
                               double *opportunity, float *root_time_or_null, double *seconds_or_null) {
  if (!parents || !branch_length || !epochs || !opportunity || ntrees < 0 || nsnps < 0 || (nsnps && (!snp_tree || !snp_counts))) {
    set_error("rl_mutctx_trees: bad arguments (ntrees=%d, nsnps=%lld; no null pointers)", ntrees, nsnps);
    return RL_EINVAL;
  }
  if (const int rc = check_epochs("rl_mutctx_trees", epochs, nepochs, kMutrateMaxEpochs)) return rc;
  for (long long s = 0; s < nsnps; s++)
    if (snp_tree[s] < 0 || snp_tree[s] >= ntrees || (s && snp_tree[s] < snp_tree[s - 1])) {
      set_error("rl_mutctx_trees: SNP %lld names tree %d (of %d; the tree before: %d): the tree indices must not fall", s,
                snp_tree[s], ntrees, s ? snp_tree[s - 1] : 0);
      return RL_EINVAL;
    }
  Adder adder(N, epochs, nepochs, device);
  if (const int rc = adder.begin()) return rc;
  const size_t nodes = (size_t)2 * N - 1;
  const int B = mutrate_batch_trees(N);
  std::vector<float> roots((size_t)std::max(1, std::min(B, ntrees)));
  std::vector<int> in_batch, ids;
  long long s0 = 0;
  for (int t0 = 0; t0 < ntrees; t0 += B) {
    const int n = std::min(B, ntrees - t0);
    long long s1 = s0;
    while (s1 < nsnps && snp_tree[s1] < t0 + n) s1++;
    in_batch.resize((size_t)(s1 - s0));
    for (long long s = s0; s < s1; s++) in_batch[(size_t)(s - s0)] = snp_tree[s] - t0;
    ids.resize(n);
    for (int t = 0; t < n; t++) ids[t] = t0 + t;
    if (const int rc = adder.add(parents + t0 * nodes, branch_length + t0 * nodes, n, in_batch.data(),
                                 snp_counts + (size_t)s0 * C96, s1 - s0, roots.data(), "rl_mutctx_trees", ids.data()))
      return rc;
    if (root_time_or_null) std::copy(roots.begin(), roots.begin() + n, root_time_or_null + t0);
    s0 = s1;
  }
  return adder.finish(opportunity, seconds_or_null);
}

extern "C" int rl_mutctx_anc(const char *anc_path, const char *mut_path, const char *mask_path, const char *ancestor_path,
                             const char *dist_path_or_null, const double *epochs, int nepochs, int device, double *mutation,
                             double *opportunity, long long *snps3) {
  if (!anc_path || !mut_path || !mask_path || !ancestor_path || !epochs || !mutation || !opportunity) return null_args("rl_mutctx_anc");
  if (const int rc = check_epochs("rl_mutctx_anc", epochs, nepochs, kMutrateMaxEpochs)) return rc;
  const int E = nepochs;
  typedef std::chrono::steady_clock Clock;
  const auto since = [](Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); };
  const Clock::time_point begun = Clock::now();
  AncText anc(kMode);
  int rc = anc.open(anc_path);
  if (rc) return rc;
  if (anc.has_ages) {
    set_error("%s: %s has sample ages: the coordinates with sample ages are not part of this build", kMode, anc_path);
    return RL_EINVAL;
  }
  const int N = anc.N;
  std::string header;
  std::vector<MutFull> mut;
  if ((rc = read_mut_full(kMode, mut_path, header, mut))) return rc;
  if (mut.back().tree >= anc.trees || mut.front().tree < 0) {
    set_error("%s: %s names tree %d, %s holds %d", kMode, mut_path, mut.front().tree < 0 ? mut.front().tree : mut.back().tree, anc_path, anc.trees);
    return RL_EINVAL;
  }
  const size_t L = mut.size();
  std::vector<int> pos, snp_pos(L);
  std::vector<unsigned char> one_branch(L);
  for (size_t s = 0; s < L; s++) snp_pos[s] = mut[s].pos, one_branch[s] = mut[s].branch.size() == 1;
  if (dist_path_or_null) {
    if ((rc = read_dist(kMode, dist_path_or_null, pos, nullptr))) return rc;
  } else {
    pos = snp_pos;
  }
  std::vector<uint32_t> counts(L * C96);
  if ((rc = rl_mutctx_count_bases(ancestor_path, mask_path, pos.data(), (long long)pos.size(), snp_pos.data(), one_branch.data(),
                                  (long long)L, counts.data())))
    return rc;
  const double count_seconds = since(begun);

  // the trees with a qualifying SNP go up batch by batch with those SNPs' rows of counts; the root times come back
  // and the numerator is added on the host, in the .mut's order (:829-908)
  Adder adder(N, epochs, E, device);
  if ((rc = adder.begin())) return rc;
  SnpTreeBatches w(N, mutrate_batch_trees(N));
  std::vector<size_t> snp_id;  // the qualifying SNPs of the batch
  std::vector<int> snp_tree;   // ... and the tree of each, within the batch
  std::vector<uint32_t> rows;  // ... and its counts
  std::vector<float> roots((size_t)w.batch);
  std::fill(mutation, mutation + (size_t)E * C96, 0.0);
  long long ones = 0, qualifying = 0;
  int trees_done = 0;
  double add_seconds = 0.0;
  const auto flush = [&]() -> int {
    const int held = (int)w.tree_id.size();
    const Clock::time_point t0 = Clock::now();
    if (const int r = adder.add(w.parents.data(), w.bl.data(), held, snp_tree.data(), rows.data(), (long long)snp_id.size(),
                                roots.data(), anc_path, w.tree_id.data()))
      return r;
    add_seconds += since(t0);
    for (size_t i = 0; i < snp_id.size(); i++) {
      const MutFull &m = mut[snp_id[i]];
      if (const int r = add_mutation(mut_path, snp_id[i], m, category_of(m), roots[snp_tree[i]], epochs, E, mutation)) return r;
    }
    trees_done += held;
    snp_id.clear(), snp_tree.clear(), rows.clear();
    return RL_OK;
  };
  const auto wanted = [&](size_t k) {
    ones += one_branch[k];
    return one_branch[k] && qualifies(mut[k]);
  };
  const auto take = [&](size_t s, int slot) {
    if (one_branch[s] && qualifies(mut[s])) {
      snp_id.push_back(s), snp_tree.push_back(slot);
      rows.insert(rows.end(), counts.begin() + s * C96, counts.begin() + (s + 1) * C96);
      qualifying++;
    }
    return RL_OK;
  };
  if ((rc = w.walk(anc, L, [&](size_t k) { return mut[k].tree; }, wanted, take, flush))) return rc;
  double seconds[3];
  if ((rc = adder.finish(opportunity, seconds))) return rc;
  if (timing_level() >= 1)
    fprintf(stderr, "[mutctx] counting bases and reading the .mut: %.6f s; %d trees of N=%d and %lld qualifying SNPs on %s: %.6f s "
            "(trees %.6f s, counts up %.6f s, chains %.6f s); reading the .anc, the numerator and the rest: %.6f s\n",
            count_seconds, trees_done, N, qualifying, device >= 0 ? "the device" : "the host", add_seconds, seconds[0], seconds[1],
            seconds[2], since(begun) - count_seconds - add_seconds);
  if (snps3) snps3[0] = (long long)L, snps3[1] = ones, snps3[2] = qualifying;
  return RL_OK;
}

extern "C" int rl_mutctx_write(const char *prefix, const double *epochs, int nepochs, const double *mutation,
                               const double *opportunity) {
  if (!prefix || !epochs || !mutation || !opportunity) return null_args("rl_mutctx_write");
  if (nepochs < 2 || nepochs > kMutrateMaxEpochs) {
    set_error("rl_mutctx_write: 2 <= epochs <= %d (%d given)", kMutrateMaxEpochs, nepochs);
    return RL_EINVAL;
  }
  return write_pair(kMode, prefix, epochs, nepochs, mutation, opportunity);
}

extern "C" int rl_mutctx_read(const char *prefix, double *epochs, int *nepochs, double *mutation, double *opportunity) {
  if (!prefix || !nepochs) return null_args("rl_mutctx_read");
  std::vector<double> ep, m, o;
  if (const int rc = read_pair(kFinalize, prefix, ep, m, o)) return rc;
  const int room = *nepochs;
  *nepochs = (int)ep.size();
  if (!epochs || !mutation || !opportunity || room < *nepochs) {
    set_error("rl_mutctx_read: %d epochs, room for %d", *nepochs, epochs && mutation && opportunity ? room : 0);
    return RL_EINVAL;
  }
  std::copy(ep.begin(), ep.end(), epochs);
  std::copy(m.begin(), m.end(), mutation);
  std::copy(o.begin(), o.end(), opportunity);
  return RL_OK;
}

// SummarizeWholeGenome (:445-576): prefix_chr<c>_mut.bin / _opp.bin of every chromosome added element by element in the
// order given, onto the first; the epochs written are the last file's.  The per-chromosome files stay
extern "C" int rl_mutctx_sum(const char *prefix, const char *chromosomes, const char *out_prefix) {
  if (!prefix || !chromosomes || !out_prefix) return null_args("rl_mutctx_sum");
  std::vector<std::string> chr;
  std::istringstream is(chromosomes);
  for (std::string line; getline(is, line);) chr.push_back(line);
  if (chr.empty()) {
    set_error("%s: no chromosome to sum", kFinalize);
    return RL_EINVAL;
  }
  std::vector<double> epochs, mutation, opportunity, ep, m, o;
  for (size_t i = 0; i < chr.size(); i++) {
    const std::string p = std::string(prefix) + "_chr" + chr[i];
    if (const int rc = read_pair(kFinalize, p, ep, m, o)) return rc;
    if (i == 0) {
      mutation = m, opportunity = o;
    } else {
      if (ep.size() != epochs.size()) {
        set_error("%s: %s_mut.bin holds %zu epochs, the chromosomes before it %zu", kFinalize, p.c_str(), ep.size(), epochs.size());
        return RL_EINVAL;
      }
      for (size_t x = 0; x < m.size(); x++) mutation[x] += m[x];
      for (size_t x = 0; x < o.size(); x++) opportunity[x] += o[x];
    }
    epochs = ep;
  }
  return write_pair(kFinalize, out_prefix, epochs.data(), (int)epochs.size(), mutation.data(), opportunity.data());
}

// FinalizeMutationRate (:365-425)
extern "C" int rl_mutctx_finalize(const char *in_prefix, const char *rate_path) {
  if (!in_prefix || !rate_path) return null_args("rl_mutctx_finalize");
  std::vector<double> epochs, mutation, opportunity;
  if (const int rc = read_pair(kFinalize, in_prefix, epochs, mutation, opportunity)) return rc;
  std::ofstream os(rate_path);
  if (os.fail()) {
    set_error("%s: error while opening file %s", kFinalize, rate_path);
    return RL_EIO;
  }
  os << "epoch.start ";
  for (const std::string &n : category_names()) os << n << " ";
  os << "\n";
  const int E = (int)epochs.size();
  for (int ep = 0; ep < E - 1; ep++) {
    os << epochs[ep] << " ";
    for (int c = 0; c < C96; c++) os << mutation[(size_t)ep * C96 + c] / opportunity[(size_t)ep * C96 + c] << " ";
    os << "\n";
  }
  os.close();
  if (os.fail()) {
    set_error("%s: writing %s failed", kFinalize, rate_path);
    return RL_EIO;
  }
  return RL_OK;
}

// anc_text.h -- the text inputs of the modes that read a dated tree sequence (coalrate.cpp: CoalescentRateForSection;
// frequency.cpp: Frequency; mutrate.cpp: AvgMutationRate; coaltree.cpp: CoalRateForTree; mutctx.cpp:
// MutationRateWithContext; subtrees.cpp: SubTreesForSubpopulation): a text file that is refused when compressed, and
// the text .anc one tree at a time (AncText); the two walks over its trees in batches -- the trees that carry a wanted
// SNP (SnpTreeBatches: mutrate, frequency, mutctx) and every tree with a factor (FactorTreeBatches: coalrate,
// coaltree); and the writer of the text .anc for the modes that write one (subtrees).  `mode` is the name a message
// starts with.  The .mut and the --dist file: mut_text.h.
#pragma once
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "anc_file.h"
#include "common.h"

namespace rl {

inline bool is_gzip(const std::string &fn) {
  FILE *fp = fopen(fn.c_str(), "rb");
  if (!fp) return false;
  unsigned char m[2] = {0, 0};
  const bool gz = fread(m, 1, 2, fp) == 2 && m[0] == 0x1f && m[1] == 0x8b;
  fclose(fp);
  return gz;
}

// opens a text input of the mode; a missing file whose .gz twin exists, or a gzip file, is refused (RL_EINVAL)
inline int open_text(const char *mode, const std::string &fn, std::ifstream &is) {
  is.open(fn);
  if (is.fail()) {
    std::ifstream gz(fn + ".gz");
    if (!gz.fail()) {
      set_error("%s: %s.gz: compressed inputs are not part of this build, decompress the file", mode, fn.c_str());
      return RL_EINVAL;
    }
    set_error("%s: failed to open file %s", mode, fn.c_str());
    return RL_EIO;
  }
  if (is_gzip(fn)) {
    set_error("%s: %s is compressed: compressed inputs are not part of this build, decompress the file", mode, fn.c_str());
    return RL_EINVAL;
  }
  return RL_OK;
}

inline bool parse_int(const std::string &s, int *v) {
  errno = 0;
  char *end = nullptr;
  const long x = strtol(s.c_str(), &end, 10);
  if (end == s.c_str() || errno || x < INT32_MIN || x > INT32_MAX) return false;
  *v = (int)x;
  return true;
}

// the text .anc (AncMutIterators::OpenFiles, src/mutations.cpp:713-752; Tree::ReadTree, src/anc.cpp:39-80), one tree
// at a time
struct AncText {
  const char *mode;
  std::string fn;
  std::ifstream is;
  int N = 0, trees = 0;
  bool has_ages = false;
  std::string line;
  explicit AncText(const char *m) : mode(m) {}
  int open(const std::string &path) {
    fn = path;
    if (const int rc = open_text(mode, fn, is)) return rc;
    std::string tag;
    long long n = 0, t = 0;
    getline(is, line);
    std::istringstream h1(line);
    h1 >> tag >> n;
    if (h1.fail() || tag != "NUM_HAPLOTYPES") return bad_header();
    long long ages = 0;
    for (double a; ages < n && h1 >> a;) ages++;
    has_ages = n > 0 && ages == n;
    getline(is, line);
    std::istringstream h2(line);
    h2 >> tag >> t;
    if (h2.fail() || tag != "NUM_TREES") return bad_header();
    if (n < 2 || n > (1 << 30) || t < 0 || t > INT32_MAX) {
      set_error("%s: %s: %lld haplotypes, %lld trees: no pair to take", mode, fn.c_str(), n, t);
      return RL_EINVAL;
    }
    N = (int)n, trees = (int)t;
    return RL_OK;
  }
  int bad_header() {
    set_error("%s: %s does not start with `NUM_HAPLOTYPES N` and `NUM_TREES T`: not a text .anc file", mode, fn.c_str());
    return RL_EFORMAT;
  }
  // `pos: parent:(branch_length num_events snp_begin snp_end) ...`, 2N-1 nodes.  The last four (each may be null):
  // the tree's position and, per node, the other three fields as Tree::ReadTree's `%f %d %d` takes them
  int next(int index, int *parent, double *bl, int *pos = nullptr, float *num_events = nullptr, int *snp_begin = nullptr,
           int *snp_end = nullptr) {
    if (!getline(is, line)) {
      set_error("%s: %s ends before tree %d of %d", mode, fn.c_str(), index, trees);
      return RL_EFORMAT;
    }
    const bool all = num_events || snp_begin || snp_end;
    const char *p = line.c_str();
    char *end = nullptr;
    const long position = strtol(p, &end, 10);
    bool ok = end != p && *end == ':';
    if (pos) *pos = (int)position;
    p = end + 1;
    for (int v = 0; ok && v < 2 * N - 1; v++) {
      const long par = strtol(p, &end, 10);
      ok = end != p && end[0] == ':' && end[1] == '(' && par >= -1 && par < 2 * (long)N - 1;
      if (!ok) break;
      p = end + 2;
      bl[v] = strtod(p, &end);
      ok = end != p;
      parent[v] = (int)par;
      if (ok && all) {
        p = end;
        const float ne = strtof(p, &end);
        ok = end != p;
        p = end;
        const long sb = ok ? strtol(p, &end, 10) : 0;
        ok = ok && end != p;
        p = end;
        const long se = ok ? strtol(p, &end, 10) : 0;
        ok = ok && end != p;
        if (num_events) num_events[v] = ne;
        if (snp_begin) snp_begin[v] = (int)sb;
        if (snp_end) snp_end[v] = (int)se;
      }
      while (ok && *end && *end != ')') end++;
      ok = ok && *end == ')';
      p = end + 1;
    }
    if (!ok) {
      set_error("%s: %s: tree %d is not `pos: parent:(branch_length num_events snp_begin snp_end) ...` for %d nodes", mode, fn.c_str(), index, 2 * N - 1);
      return RL_EFORMAT;
    }
    return RL_OK;
  }
};

// The trees of an .anc that carry a wanted SNP of its .mut, a batch at a time (mutrate.cpp, frequency.cpp,
// mutctx.cpp).  The SNPs are numbered in the .mut's order, their tree indices do not fall.  The mode supplies
// tree_of(k), the tree of SNP k; wanted(k), called once for every SNP in order: a tree with a wanted SNP is kept;
// take(s, slot), called for every SNP of a kept tree with the tree's place in the batch (RL_OK, or the message set);
// and flush(), called with `batch` trees held and at the end with what is left: tree_id names the trees held, parents
// and bl hold them.  A tree that is not kept is read into a scratch tree (the file is read line by line).
struct SnpTreeBatches {
  const size_t nodes;
  const int batch;
  std::vector<int> parents, tree_id, scratch_parent;
  std::vector<double> bl, scratch_bl;
  SnpTreeBatches(int N, int batch_trees)
      : nodes((size_t)2 * N - 1), batch(batch_trees), parents(batch * nodes), scratch_parent(nodes), bl(batch * nodes),
        scratch_bl(nodes) {}
  template <class TreeOf, class Wanted, class Take, class Flush>
  int walk(AncText &anc, size_t nsnps, TreeOf tree_of, Wanted wanted, Take take, Flush flush) {
    size_t k = 0;
    for (int t = 0; t < anc.trees && k < nsnps; t++) {
      bool keep = false;
      const size_t k0 = k, slot = tree_id.size();
      for (; k < nsnps && tree_of(k) == t; k++) keep |= wanted(k);
      if (const int rc = anc.next(t, keep ? &parents[slot * nodes] : scratch_parent.data(), keep ? &bl[slot * nodes] : scratch_bl.data()))
        return rc;
      if (!keep) continue;
      for (size_t s = k0; s < k; s++)
        if (const int rc = take(s, (int)slot)) return rc;
      tree_id.push_back(t);
      if ((int)tree_id.size() < batch) continue;
      if (const int rc = flush()) return rc;
      tree_id.clear();
    }
    const int rc = tree_id.empty() ? RL_OK : flush();
    tree_id.clear();
    return rc;
  }
};

// Every tree of an .anc with a factor, a batch at a time (coalrate.cpp, coaltree.cpp): read() puts tree t behind the
// `held` trees of the batch, after a flush if the batch is full; the mode sets factors[held] and counts the tree in.
// flush(add) hands the batch to add(parents, bl, factors, held, index0), index0 the number of its first tree in the
// file.  Where the trees end is the mode's rule.
struct FactorTreeBatches {
  const size_t nodes;
  const int batch;
  std::vector<int> parents;
  std::vector<double> bl;
  std::vector<float> factors;
  int held = 0;
  long long index0 = 0;
  FactorTreeBatches(int N, int batch_trees)
      : nodes((size_t)2 * N - 1), batch(batch_trees), parents(batch * nodes), bl(batch * nodes), factors(batch) {}
  template <class Add>
  int flush(Add add) {
    const int r = held ? add(parents.data(), bl.data(), factors.data(), held, index0) : RL_OK;
    index0 += held;
    held = 0;
    return r;
  }
  template <class Add>
  int read(AncText &anc, int t, Add add) {
    if (held == batch)
      if (const int rc = flush(add)) return rc;
    return anc.next(t, &parents[held * nodes], &bl[held * nodes]);
  }
};

// the text .anc without sample ages as AncesTree::Dump(const std::string&) writes it (src/anc.cpp:1050-1073 and
// :991-1013): `NUM_HAPLOTYPES N ` with its trailing blank, `NUM_TREES T`, then per tree `pos: ` and per node
// `parent:(%.5f %.3f %d %d) `
inline int write_anc_text(const char *mode, const std::string &fn, int N, const std::vector<AncTree> &trees) {
  FILE *fp = fopen(fn.c_str(), "w");
  if (!fp) {
    set_error("%s: error while writing to %s", mode, fn.c_str());
    return RL_EIO;
  }
  fprintf(fp, "NUM_HAPLOTYPES %ld ", (long)N);
  fprintf(fp, "\n");
  fprintf(fp, "NUM_TREES %ld\n", (long)trees.size());
  for (const AncTree &t : trees) {
    fprintf(fp, "%d: ", t.pos);
    for (size_t v = 0; v < t.parent.size(); v++)
      fprintf(fp, "%d:(%.5f %.3f %d %d) ", t.parent[v], t.branch_length[v], (double)t.num_events[v], t.snp_begin[v], t.snp_end[v]);
    fprintf(fp, "\n");
  }
  const bool failed = ferror(fp) != 0;
  if (fclose(fp) != 0 || failed) {
    set_error("%s: writing %s failed", mode, fn.c_str());
    return RL_EIO;
  }
  return RL_OK;
}

}  // namespace rl

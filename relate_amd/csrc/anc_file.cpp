// anc_file.cpp -- reading and writing the binary .anc file (anc_file.h).
#include "anc_file.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "common.h"

namespace rl {

// AncesTree::ReadBin (src/anc.cpp:941-968) + Tree::ReadTreeBin (:83-125)
int read_anc(const std::string &fn, AncFile &a) {
  FILE *fp = fopen(fn.c_str(), "rb");
  if (!fp) {
    set_error("cannot open %s", fn.c_str());
    return RL_EIO;
  }
  unsigned T = 0;
  bool ok = fread(&a.has_ages, sizeof(bool), 1, fp) == 1 && fread(&a.N, 4, 1, fp) == 1;
  if (ok && a.has_ages) {
    a.ages.resize(a.N);
    ok = fread(a.ages.data(), 8, a.N, fp) == a.N;
  }
  ok = ok && fread(&T, 4, 1, fp) == 1;
  const int nodes = 2 * (int)a.N - 1;
  a.trees.assign(ok ? T : 0, AncTree());
  // a tree = `int pos` + nodes records of 24 bytes (parent, branch_length, num_events, SNP_begin, SNP_end, written
  // field by field: no padding): one read per tree -- field by field the C3 chunk's 22.9 GB were 4.8e9 fread calls
  std::vector<unsigned char> rec((size_t)nodes * 24);
  for (unsigned t = 0; ok && t < T; t++) {
    AncTree &tr = a.trees[t];
    tr.parent.resize(nodes);
    tr.snp_begin.resize(nodes);
    tr.snp_end.resize(nodes);
    tr.branch_length.resize(nodes);
    tr.num_events.resize(nodes);
    tr.child_left.assign(nodes, -1);
    tr.child_right.assign(nodes, -1);
    ok = fread(&tr.pos, 4, 1, fp) == 1 && fread(rec.data(), 24, (size_t)nodes, fp) == (size_t)nodes;
    for (int i = 0; ok && i < nodes; i++) {
      const unsigned char *q = rec.data() + (size_t)i * 24;
      memcpy(&tr.parent[i], q, 4);
      memcpy(&tr.branch_length[i], q + 4, 8);
      memcpy(&tr.num_events[i], q + 12, 4);
      memcpy(&tr.snp_begin[i], q + 16, 4);
      memcpy(&tr.snp_end[i], q + 20, 4);
      const int p = tr.parent[i];
      if (p != -1) {
        if (p < 0 || p >= nodes) {
          ok = false;
        } else if (tr.child_left[p] == -1) {
          tr.child_left[p] = i;
        } else {
          tr.child_right[p] = i;
        }
      }
    }
  }
  fclose(fp);
  if (!ok) {
    set_error("%s: truncated or malformed .anc file", fn.c_str());
    return RL_EIO;
  }
  return RL_OK;
}

// AncesTree::DumpBin (src/anc.cpp:1104-1167)
int write_anc(const std::string &fn, const AncFile &a) {
  FILE *fp = fopen(fn.c_str(), "wb");
  if (!fp) {
    set_error("cannot open %s for writing", fn.c_str());
    return RL_EIO;
  }
  const unsigned T = (unsigned)a.trees.size();
  fwrite(&a.has_ages, sizeof(bool), 1, fp);
  fwrite(&a.N, 4, 1, fp);
  if (a.has_ages) fwrite(a.ages.data(), 8, a.N, fp);
  fwrite(&T, 4, 1, fp);
  const int nodes = 2 * (int)a.N - 1;
  std::vector<unsigned char> rec((size_t)nodes * 24);
  for (const AncTree &tr : a.trees) {
    fwrite(&tr.pos, 4, 1, fp);
    for (int i = 0; i < nodes; i++) {
      unsigned char *q = rec.data() + (size_t)i * 24;
      memcpy(q, &tr.parent[i], 4);
      const double bl = tr.branch_length.empty() ? 0.0 : tr.branch_length[i];  // (empty: all zero, BuildTopology's trees)
      memcpy(q + 4, &bl, 8);
      memcpy(q + 12, &tr.num_events[i], 4);
      memcpy(q + 16, &tr.snp_begin[i], 4);
      memcpy(q + 20, &tr.snp_end[i], 4);
    }
    fwrite(rec.data(), 24, (size_t)nodes, fp);
  }
  const bool bad = ferror(fp) != 0;
  if (fclose(fp) != 0 || bad) {  // (a full disc must not pass for a tree file)
    set_error("writing %s failed", fn.c_str());
    return RL_EIO;
  }
  return RL_OK;
}

int anc_coverage(const AncFile &a, const char *fn, int *first, int *last) {
  if (a.trees.empty()) {
    set_error("%s holds no tree", fn);
    return RL_EFORMAT;
  }
  for (size_t t = 1; t < a.trees.size(); t++)
    if (a.trees[t].pos <= a.trees[t - 1].pos) {
      set_error("%s: the position of tree %zu (%d) is not above that of the tree before it (%d)", fn, t, a.trees[t].pos, a.trees[t - 1].pos);
      return RL_EFORMAT;
    }
  *first = a.trees.front().pos;
  const AncTree &z = a.trees.back();
  *last = std::max(z.pos, *std::max_element(z.snp_end.begin(), z.snp_end.end()));
  return RL_OK;
}

int read_anc_header(const std::string &fn, unsigned *N, unsigned *trees, bool *has_ages) {
  FILE *fp = fopen(fn.c_str(), "rb");
  if (!fp) {
    set_error("cannot open %s", fn.c_str());
    return RL_EIO;
  }
  bool ok = fread(has_ages, sizeof(bool), 1, fp) == 1 && fread(N, 4, 1, fp) == 1;
  if (ok && *has_ages) ok = fseek(fp, (long)*N * 8, SEEK_CUR) == 0;
  ok = ok && fread(trees, 4, 1, fp) == 1;
  fclose(fp);
  if (!ok) {
    set_error("%s: truncated or malformed .anc file", fn.c_str());
    return RL_EIO;
  }
  return RL_OK;
}

}  // namespace rl

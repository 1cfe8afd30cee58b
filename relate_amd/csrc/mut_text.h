// mut_text.h -- the text .mut (Mutations::Read, src/mutations.cpp:230-430) and the --dist file.  `mode` is the name a
// message starts with.
//   read_mut_lines   the line loop every reader of a .mut shares and nothing of what a reader accepts: read_mut_rows
//                    and read_mut_full below, the read_mut of mutrate.cpp (AvgMutationRate) and that of frequency.cpp
//                    (Frequency) each bring the parser of their own row
//   read_mut_rows, Persistence   three columns, for the modes that weigh a tree by the bases it persists for
//                    (coalrate.cpp: CoalescentRateForSection; coaltree.cpp: CoalRateForTree)
//   read_mut_full, write_mut_text   every column, for the modes that write a .mut or read its alleles (subtrees.cpp:
//                    SubTreesForSubpopulation; mutctx.cpp: MutationRateWithContext); the writer of Mutations::Dump
//                    (:457-508)
//   read_dist        the --dist file (mutrate.cpp, mutctx.cpp)
#pragma once
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "anc_text.h"
#include "common.h"

namespace rl {

// The lines of a .mut: the header (kept if asked for), then per line that is not empty its fields, split at `;` --
// what follows the last `;` is a field too, the reader decides what an empty one means.  parse(fields, row, line
// number) fills the row: RL_OK; RL_EFORMAT, and the message here names the line and `format`; or another code with
// the message set.  Row has a member `tree`: a file whose tree indices fall, or one without a SNP, is refused.
template <class Row, class Parse>
int read_mut_lines(const char *mode, const std::string &fn, const char *format, std::string *header_or_null,
                   std::vector<Row> &rows, Parse parse) {
  std::ifstream is;
  if (const int rc = open_text(mode, fn, is)) return rc;
  std::string line;
  getline(is, line);  // the header
  if (header_or_null) *header_or_null = line;
  long long n = 1;
  std::vector<std::string> f;
  while (getline(is, line)) {
    n++;
    if (line.empty()) continue;
    f.assign(1, std::string());
    for (char c : line) {
      if (c == ';') f.emplace_back();
      else f.back() += c;
    }
    Row r{};
    if (const int rc = parse(f, r, n)) {
      if (rc == RL_EFORMAT) set_error("%s: %s: line %lld is not `%s`", mode, fn.c_str(), n, format);
      return rc;
    }
    if (!rows.empty() && r.tree < rows.back().tree) {
      set_error("%s: %s: line %lld: tree index %d after %d: the tree indices must not fall", mode, fn.c_str(), n, r.tree, rows.back().tree);
      return RL_EINVAL;
    }
    rows.push_back(std::move(r));
  }
  if (rows.empty()) {
    set_error("%s: %s holds no SNP", mode, fn.c_str());
    return RL_EFORMAT;
  }
  return RL_OK;
}

// ---- the .mut as the modes that weigh a tree by the bases it persists for read it
struct MutRow {
  int pos, dist, tree;
};

// the second column pos, the third dist, the fifth tree; what follows the fifth is not read
inline int read_mut_rows(const char *mode, const std::string &fn, std::vector<MutRow> &rows) {
  return read_mut_lines(mode, fn, "snp;pos;dist;rs_id;tree;...", nullptr, rows, [](std::vector<std::string> &f, MutRow &r, long long) {
    return f.size() >= 5 && parse_int(f[1], &r.pos) && parse_int(f[2], &r.dist) && parse_int(f[4], &r.tree) ? RL_OK : RL_EFORMAT;
  });
}

// AncMutIterators::NextTree, mode 0 (src/mutations.cpp:854-912), with pos and dist the .mut's own (no --dist): the
// bases tree `tree` persists for -- half the dist before its first SNP, its SNPs' dists, minus half the last --
// or 0 for a tree without SNPs
struct Persistence {
  const std::vector<MutRow> &mut;
  size_t k = 0;
  int tree_in_mut;
  explicit Persistence(const std::vector<MutRow> &m) : mut(m), tree_in_mut(m[0].tree) {}
  double next(int tree) {
    if (tree != tree_in_mut) return 0.0;
    double bases = k != 0 ? mut[k - 1].dist / 2.0 : 0.0;
    while (tree_in_mut == mut[k].tree) {
      bases += mut[k].dist;
      k++;
      if (k == mut.size()) break;
    }
    if (k != mut.size()) {
      bases -= mut[k - 1].dist / 2.0;
      tree_in_mut = mut[k].tree;
    }
    return bases;
  }
};

// the --dist file (AvgMutationRate.cpp:326-357): one header line, then `pos dist` per line (sscanf "%d %d"); dist
// may be null
inline int read_dist(const char *mode, const std::string &fn, std::vector<int> &pos, std::vector<int> *dist_or_null) {
  std::ifstream is;
  if (const int rc = open_text(mode, fn, is)) return rc;
  std::string line;
  getline(is, line);
  long long n = 1;
  while (getline(is, line)) {
    n++;
    int p = 0, d = 0;
    if (sscanf(line.c_str(), "%d %d", &p, &d) != 2) {
      set_error("%s: %s: line %lld is not `pos dist`", mode, fn.c_str(), n);
      return RL_EFORMAT;
    }
    pos.push_back(p);
    if (dist_or_null) dist_or_null->push_back(d);
  }
  if (pos.empty()) {
    set_error("%s: %s holds no position", mode, fn.c_str());
    return RL_EFORMAT;
  }
  return RL_OK;
}

// ---- the .mut with every column

// SNPInfo (src/mutations.hpp:11-25)
struct MutFull {
  int snp_id = 0, pos = 0, dist = 0, tree = 0;
  std::string rs_id;
  std::vector<int> branch;
  bool flipped = false;
  float age_begin = 0.0f, age_end = 0.0f;
  std::string mutation_type, upstream_base = "NA", downstream_base = "NA";
  std::vector<int> freq;
};

// `snp;pos;dist;rs-id;tree;branches;is_not_mapping;is_flipped;age_begin;age_end;` and, optional, `alleles;` and
// `upstream;downstream;freq;...;`.  The branches are blank separated; is_not_mapping is not kept (the writer derives it
// from the number of branches).  A file whose tree indices fall is refused
inline int read_mut_full(const char *mode, const std::string &fn, std::string &header, std::vector<MutFull> &rows) {
  const char *const format = "snp;pos;dist;rs_id;tree;branches;is_not_mapping;is_flipped;age_begin;age_end;[alleles;[upstream;downstream;freq;...]]";
  return read_mut_lines(mode, fn, format, &header, rows, [](std::vector<std::string> &f, MutFull &r, long long) {
    if (f.back().empty()) f.pop_back();  // (what follows the last `;`)
    int flipped = 0;
    bool ok = f.size() >= 10 && f.size() != 12 && parse_int(f[0], &r.snp_id) && parse_int(f[1], &r.pos) &&
              parse_int(f[2], &r.dist) && parse_int(f[4], &r.tree) && parse_int(f[7], &flipped);
    if (ok) {
      r.rs_id = f[3];
      r.flipped = flipped != 0;
      const char *p = f[5].c_str();
      for (;;) {
        while (*p == ' ') p++;
        if (!*p) break;
        char *end = nullptr;
        const long b = strtol(p, &end, 10);
        if (end == p || b < INT32_MIN || b > INT32_MAX) {
          ok = false;
          break;
        }
        r.branch.push_back((int)b);
        p = end;
      }
      char *end = nullptr;
      r.age_begin = (float)strtod(f[8].c_str(), &end);  // (std::stod into a float member)
      ok = ok && end != f[8].c_str();
      r.age_end = (float)strtod(f[9].c_str(), &end);
      ok = ok && end != f[9].c_str();
    }
    if (ok && f.size() > 10) r.mutation_type = f[10];
    if (ok && f.size() > 12) {
      r.upstream_base = f[11];
      r.downstream_base = f[12];
      for (size_t k = 13; ok && k < f.size(); k++) {
        int x = 0;
        ok = parse_int(f[k], &x);
        r.freq.push_back(x);
      }
    }
    return ok ? RL_OK : RL_EFORMAT;
  });
}

// Mutations::Dump (src/mutations.cpp:457-508): the header (the standard one if empty), then a line per SNP; the ages
// with the precision of operator<<; the flanking bases and the frequencies only where a row has frequencies
inline int write_mut_text(const char *mode, const std::string &fn, const std::string &header, const std::vector<MutFull> &rows) {
  std::ofstream os(fn);
  if (os.fail()) {
    set_error("%s: error while writing to %s", mode, fn.c_str());
    return RL_EIO;
  }
  if (header.size() > 0) os << header;
  else os << "snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;ancestral_allele/alternative_allele;upstream_allele;downstream_allele;";
  os << "\n";
  for (const MutFull &r : rows) {
    os << r.snp_id << ";" << r.pos << ";" << r.dist << ";" << r.rs_id << ";" << r.tree << ";";
    for (size_t k = 0; k < r.branch.size(); k++) {
      if (k) os << " ";
      os << r.branch[k];
    }
    os << (r.branch.size() > 1 ? ";1;" : ";0;");
    os << r.flipped << ";" << r.age_begin << ";" << r.age_end << ";";
    os << r.mutation_type << ";";
    if (r.freq.size() > 0) {
      os << r.upstream_base << ";" << r.downstream_base << ";";
      for (int x : r.freq) os << x << ";";
    }
    os << "\n";
  }
  os.close();
  if (os.fail()) {
    set_error("%s: writing %s failed", mode, fn.c_str());
    return RL_EIO;
  }
  return RL_OK;
}

}  // namespace rl

// coalrate.cpp -- CoalescentRateForSection and FinalizePopulationSize, host side (include/relate_amd.h has the
// definitions; the reference: include/evaluate/coalescent_rate/CoalescentRateForSection.cpp, FinalizePopulationSize.cpp).
//
// D[e][i][j], E planes of N x N floats: for i < j with m = MRCA(i,j), t = t(m) the float time and es the epoch t falls
// in, D[es][i][j] gets the tree's factor (the count) and D[e][j][i], e <= es, the factor times the time the pair spent
// uncoalesced in epoch e (the opportunity).  Every element gets at most one float addition per tree, trees in order.
// As on the device (coalrate_kernels.hip) a row of a tree is a running maximum of g outwards from rank[i]
// (pairwise.cpp), no walk in the tree.  This file is that on one thread for any N (the CPU suite's implementation,
// the yardstick of the GPU tests and the `device < 0` path), the epochs, the loop over the text .anc (anc_text.h) and
// the .mut with the factors of AncMutIterators::NextTree, the .bin file, the finalize step with the .coal file, and
// the C entry points.
#include <cerrno>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "anc_text.h"
#include "coalrate.h"
#include "common.h"
#include "mut_text.h"
#include "tree_host.h"

namespace rl {

// Sample::Read (src/sample.cpp:4-110): the group names sorted, and the group of every haplotype -- two haplotypes per
// line, one if any line's fourth column is `1`.  `mode` is the name a message starts with (FinalizePopulationSize; subtrees.cpp:
// SubTreesForSubpopulation)
int read_poplabels(const char *mode, const std::string &fn, std::vector<std::string> &groups, std::vector<int> &group_of_haplotype) {
  std::ifstream is(fn);
  if (is.fail()) {
    set_error("%s: failed to open file %s", mode, fn.c_str());
    return RL_EIO;
  }
  if (is_gzip(fn)) {
    set_error("%s: %s is compressed: compressed inputs are not part of this build, decompress the file", mode, fn.c_str());
    return RL_EINVAL;
  }
  std::string line;
  std::vector<std::string> group_of_line;
  bool diploid = true;
  getline(is, line);  // the header
  while (getline(is, line)) {
    if (line.empty()) continue;
    std::vector<std::string> col(1);
    for (char c : line) {
      if (c == ' ' || c == '\t') col.emplace_back();
      else col.back() += c;
    }
    if (col.size() < 2) {
      set_error("%s: %s: `%s` has no second column (the group)", mode, fn.c_str(), line.c_str());
      return RL_EFORMAT;
    }
    const std::string ploidy = col.size() > 3 ? col[3] : std::string();
    if (ploidy != "NA") {
      if (ploidy == "1") diploid = false;
      else if (!diploid) {
        set_error("%s: %s: Detected both haploid and diploid samples.", mode, fn.c_str());
        return RL_EINVAL;
      }
    }
    group_of_line.push_back(col[1]);
    if (std::find(groups.begin(), groups.end(), col[1]) == groups.end()) groups.push_back(col[1]);
  }
  std::sort(groups.begin(), groups.end());
  for (const std::string &gname : group_of_line) {
    const int ind = (int)(std::find(groups.begin(), groups.end(), gname) - groups.begin());
    group_of_haplotype.push_back(ind);
    if (diploid) group_of_haplotype.push_back(ind);
  }
  return RL_OK;
}

namespace {

// the product is rounded, then the sum: no fused multiply-add (coalrate_kernels.hip does the same)
inline float term(float factor, float hi, float lo) {
#pragma clang fp contract(off)
  const float w = hi - lo;
  return factor * w;
}

// one tree's tables and its contribution to D
struct HostCoalrate : TreeTables {
  std::vector<int> order, g, es;
  std::vector<float> tm;
  explicit HostCoalrate(int n) : TreeTables(n), order(n), g(n), es(nodes), tm(nodes) {}

  // parent must have passed first_bad_node, the branch lengths first_bad_length
  void prepare(const int *parent, const double *bl, const float *ep, int E) {
    fill(parent);
    for (int v = 0; v < N; v++) tm[v] = 0.0f;
    for (int n = N; n < nodes; n++) {
      tm[n] = (float)((double)tm[first[n]] + bl[first[n]]);  // rounded at every node
      int e = 0;
      while (e < E - 1 && !(tm[n] < ep[e + 1])) e++;
      es[n] = e;
    }
    for (int p = N; p < nodes; p++) g[lo[second[p]] - 1] = p;
    for (int v = 0; v < N; v++) order[lo[v]] = v;
  }

  // row i of every plane: the counts of the pairs (i, j > i), the opportunities of the pairs (j < i, i)
  void add_row(int i, float *D, float f, const float *ep, const float *fw, int E) const {
    const size_t plane = (size_t)N * N;
    float *row = D + (size_t)i * N;
    const auto element = [&](int j, int m) {
      const int e = es[m];
      if (j > i) {
        if (e < E - 1) row[(size_t)e * plane + j] += f;
        return;
      }
      const int last = std::min(e, E - 2);
      for (int q = 0; q <= last; q++) row[(size_t)q * plane + j] += q == e ? term(f, tm[m], ep[e]) : fw[q];
    };
    const int r = lo[i];
    int m = 0;
    for (int p = r; p < N - 1; p++) {
      m = std::max(m, g[p]);
      element(order[p + 1], m);
    }
    m = 0;
    for (int p = r - 1; p >= 0; p--) {
      m = std::max(m, g[p]);
      element(order[p], m);
    }
  }
};

// the sum in the making, on the host (in the caller's planes) or on a device
struct Coalrate {
  int N = 0, E = 0, device = -1;
  const float *ep = nullptr;
  float *out = nullptr;
  CoalrateDevice *dev = nullptr;
  HostCoalrate *host = nullptr;
  ~Coalrate() {
    if (dev) coalrate_device_free(dev);
    delete host;
  }
  int begin(int n, const float *epochs, int e, int d, float *o) {
    N = n, E = e, device = d, ep = epochs, out = o;
    if (device >= 0) return coalrate_device_begin(&dev, N, ep, E, device);
    memset(out, 0, (size_t)4 * E * N * N);
    host = new HostCoalrate(N);
    return RL_OK;
  }
  // `where` names the trees' origin in a message (the entry point, or the file), index0 the first tree's number there
  int add(const int *parents, const double *bl, const float *factors, int ntrees, const char *where, long long index0) {
    const size_t nodes = (size_t)2 * N - 1;
    for (int t = 0; t < ntrees; t++)
      if (!(std::fabs(factors[t]) <= FLT_MAX)) {
        set_error("%s: tree %lld: its factor is not finite", where, index0 + t);
        return RL_EINVAL;
      }
    int bad = -1;
    if (dev) {
      const int rc = coalrate_device_add(dev, parents, bl, factors, ntrees, &bad);
      if (bad < 0) return rc;
    }
    for (int t = dev ? bad : 0; t < (dev ? bad + 1 : ntrees); t++) {
      const int *parent = parents + t * nodes;
      const double *b = bl + t * nodes;
      const std::string tree = std::string(where) + ": tree " + std::to_string(index0 + t);
      std::vector<unsigned char> kids;
      if (const int rc = check_tree(tree.c_str(), parent, b, N, 2 * N - 2, dev != nullptr, kids)) return rc;
      host->prepare(parent, b, ep, E);
      float fw[kCoalrateMaxEpochs];
      for (int e = 0; e < E - 1; e++) fw[e] = term(factors[t], ep[e + 1], ep[e]);
      for (int i = 0; i < N; i++) host->add_row(i, out, factors[t], ep, fw, E);
    }
    return RL_OK;
  }
  int finish() { return dev ? coalrate_device_finish(dev, out) : RL_OK; }
};

}  // namespace
}  // namespace rl

using namespace rl;

extern "C" int rl_coalrate_batch_trees(int N) { return N < 2 ? 0 : coalrate_batch_trees(N); }

extern "C" int rl_coalrate_epochs(float years_per_gen, const char *bins_or_null, float *epochs, int *nepochs) {
  return make_epochs("rl_coalrate_epochs", years_per_gen, bins_or_null, epochs, nepochs);
}

extern "C" int rl_coalrate_trees(const int *parents, const double *branch_length, const float *factors, int N,
                                 int ntrees, const float *epochs, int nepochs, int device, float *out) {
  if (!parents || !branch_length || !factors || !epochs || !out || ntrees < 0) {
    set_error("rl_coalrate_trees: bad arguments (ntrees=%d; no null pointers)", ntrees);
    return RL_EINVAL;
  }
  if (N < 2) {
    set_error("rl_coalrate_trees: N=%d: no pair to take", N);
    return RL_EINVAL;
  }
  if (const int rc = check_epochs("rl_coalrate_trees", epochs, nepochs, kCoalrateMaxEpochs)) return rc;
  Coalrate cr;
  int rc = cr.begin(N, epochs, nepochs, device, out);
  rc = rc ? rc : cr.add(parents, branch_length, factors, ntrees, "rl_coalrate_trees", 0);
  return rc ? rc : cr.finish();
}

extern "C" int rl_coalrate_anc(const char *anc_path, const char *mut_path, const float *epochs, int nepochs, int device,
                               float *out_or_null, int *N_out) {
  if (!anc_path || !mut_path || !epochs || !N_out) return null_args("rl_coalrate_anc");
  if (const int rc = check_epochs("rl_coalrate_anc", epochs, nepochs, kCoalrateMaxEpochs)) return rc;
  AncText anc("CoalescentRateForSection");
  int rc = anc.open(anc_path);
  if (rc) return rc;
  if (anc.has_ages) {
    set_error("CoalescentRateForSection: %s has sample ages: the recursion with sample ages and its re-cut epochs are not part of this build", anc_path);
    return RL_EINVAL;
  }
  if (anc.trees < 1) {
    set_error("CoalescentRateForSection: %s holds no tree", anc_path);
    return RL_EFORMAT;
  }
  const int N = anc.N;
  *N_out = N;
  if (!out_or_null) return RL_OK;
  std::vector<MutRow> mut;
  if ((rc = read_mut_rows("CoalescentRateForSection", mut_path, mut))) return rc;
  Coalrate cr;
  if ((rc = cr.begin(N, epochs, nepochs, device, out_or_null))) return rc;
  // the loop of CoalescentRateForSection.cpp:441-480: every tree with the bases it persists for -- and, NextTree
  // having returned -1 with the last tree still in place, the last tree once more with the factor -1
  FactorTreeBatches w(N, coalrate_batch_trees(N));
  const size_t nodes = w.nodes;
  Persistence persistence(mut);
  const auto add = [&](const int *p, const double *b, const float *f, int n, long long index0) {
    return cr.add(p, b, f, n, anc_path, index0);
  };
  bool over = false;  // a negative factor ends the reference's loop
  for (int t = 0; t < anc.trees && !over; t++) {
    if ((rc = w.read(anc, t, add))) return rc;
    w.factors[w.held] = (float)persistence.next(t);
    over = !(w.factors[w.held] >= 0.0f);
    w.held++;
  }
  if (!over) {
    const size_t last = (size_t)(w.held - 1) * nodes;  // (held >= 1: the batch is flushed before a tree is read)
    const std::vector<int> p(w.parents.begin() + last, w.parents.begin() + last + nodes);
    const std::vector<double> b(w.bl.begin() + last, w.bl.begin() + last + nodes);
    if ((rc = w.flush(add))) return rc;
    std::copy(p.begin(), p.end(), w.parents.begin());
    std::copy(b.begin(), b.end(), w.bl.begin());
    w.factors[0] = -1.0f;
    w.held = 1;
    w.index0--;  // (a message names the tree, not the pass)
  }
  if ((rc = w.flush(add))) return rc;
  return cr.finish();
}

extern "C" int rl_coalrate_write_bin(const char *path, const float *epochs, int nepochs, const float *data, int N) {
  if (!path || !epochs || !data || nepochs < 1 || N < 1) return null_args("rl_coalrate_write_bin");
  FILE *fp = fopen(path, "wb");
  const int32_t E = nepochs;
  const uint64_t words[2] = {(uint64_t)N, (uint64_t)N};  // (CollapsedMatrix::size_type)
  const size_t plane = (size_t)N * N;
  bool ok = fp && fwrite(&E, 4, 1, fp) == 1 && fwrite(epochs, 4, (size_t)E, fp) == (size_t)E;
  for (int e = 0; ok && e < E; e++) ok = fwrite(words, 8, 2, fp) == 2 && fwrite(data + e * plane, 4, plane, fp) == plane;
  if ((fp && fclose(fp) != 0) || !ok) {
    set_error("rl_coalrate_write_bin: writing %s failed", path);
    return RL_EIO;
  }
  return RL_OK;
}

extern "C" int rl_coalrate_read_bin(const char *path, float *epochs_or_null, int *nepochs, float *data_or_null, int *N) {
  if (!path || !nepochs || !N) return null_args("rl_coalrate_read_bin");
  FILE *fp = fopen(path, "rb");
  if (!fp) {
    set_error("rl_coalrate_read_bin: cannot open %s", path);
    return RL_EIO;
  }
  int32_t E = 0;
  uint64_t words[2] = {0, 0};
  std::vector<float> ep;
  bool ok = fread(&E, 4, 1, fp) == 1 && E >= 1 && E <= (1 << 20);
  if (ok) {
    ep.resize((size_t)E);
    ok = fread(ep.data(), 4, (size_t)E, fp) == (size_t)E && fread(words, 8, 2, fp) == 2 && words[0] == words[1] &&
         words[0] >= 1 && words[0] <= (1u << 30);
  }
  const size_t n = (size_t)words[0], plane = n * n;
  for (int e = 0; ok && e < E; e++) {
    uint64_t w[2] = {words[0], words[1]};
    if (e) ok = fread(w, 8, 2, fp) == 2 && w[0] == words[0] && w[1] == words[1];
    if (!ok) break;
    if (data_or_null) ok = fread(data_or_null + e * plane, 4, plane, fp) == plane;
    else ok = fseek(fp, (long)(plane * 4), SEEK_CUR) == 0;
  }
  if (ok && !data_or_null) {  // (a seek past the end succeeds: the size decides)
    const long at = ftell(fp);
    ok = fseek(fp, 0, SEEK_END) == 0 && ftell(fp) >= at;
  }
  fclose(fp);
  if (!ok) {
    set_error("rl_coalrate_read_bin: %s is not `int32 E, E floats, E x (N, N, N x N floats)`", path);
    return RL_EFORMAT;
  }
  *nepochs = E;
  *N = (int)n;
  if (epochs_or_null) memcpy(epochs_or_null, ep.data(), ep.size() * 4);
  return RL_OK;
}

extern "C" int rl_coalrate_finalize(const float *data, int N, int nepochs, const int *group_of_haplotype_or_null,
                                    int ngroups, double *rates) {
  if (!data || !rates || N < 1 || nepochs < 1 || ngroups < 1) {
    set_error("rl_coalrate_finalize: bad arguments (N=%d, nepochs=%d, ngroups=%d; no null pointers)", N, nepochs, ngroups);
    return RL_EINVAL;
  }
  const int *grp = group_of_haplotype_or_null;
  if (!grp && ngroups != 1) {
    set_error("rl_coalrate_finalize: %d groups without a group per haplotype", ngroups);
    return RL_EINVAL;
  }
  for (int i = 0; grp && i < N; i++)
    if (grp[i] < 0 || grp[i] >= ngroups) {
      set_error("rl_coalrate_finalize: haplotype %d is in group %d of %d", i, grp[i], ngroups);
      return RL_EINVAL;
    }
  // FinalizePopulationSize.cpp:69-91, :201-235: float sums over i < j in that order, per (group pair, epoch)
  const size_t G = (size_t)ngroups, E = (size_t)nepochs, plane = (size_t)N * N;
  std::vector<float> num(G * G * E, 0.0f), denom(G * G * E, 0.0f);
  for (int i = 0; i < N; i++)
    for (int j = i + 1; j < N; j++) {
      int gi = grp ? grp[i] : 0, gj = grp ? grp[j] : 0;
      if (gi > gj) std::swap(gi, gj);
      float *nu = &num[(gi * G + gj) * E], *de = &denom[(gi * G + gj) * E];
      for (size_t e = 0; e + 1 < E; e++) {
        nu[e] += data[e * plane + (size_t)i * N + j];
        de[e] += data[e * plane + (size_t)j * N + i];
      }
    }
  for (size_t i = 0; i < G; i++)
    for (size_t j = 0; j < G; j++) {
      const size_t a = std::min(i, j), b = std::max(i, j);
      for (size_t e = 0; e < E; e++) {
        const float rate = num[(a * G + b) * E + e] / denom[(a * G + b) * E + e];  // (0 / 0 in the last epoch)
        rates[(i * G + j) * E + e] = rate;
      }
    }
  return RL_OK;
}

extern "C" int rl_coalrate_finalize_files(const char *bin_path, const char *poplabels_or_null, const char *coal_path) {
  if (!bin_path || !coal_path) return null_args("rl_coalrate_finalize_files");
  if (poplabels_or_null && std::string(poplabels_or_null) == "hap") {
    set_error("FinalizePopulationSize: --poplabels hap (FinalizePopulationSizeByHaplotype) is not part of this build");
    return RL_EINVAL;
  }
  std::vector<std::string> groups;
  std::vector<int> group_of_haplotype;
  if (poplabels_or_null)
    if (const int rc = read_poplabels("FinalizePopulationSize", poplabels_or_null, groups, group_of_haplotype)) return rc;
  int E = 0, N = 0;
  int rc = rl_coalrate_read_bin(bin_path, nullptr, &E, nullptr, &N);
  if (rc) return rc;
  if (poplabels_or_null && (int)group_of_haplotype.size() != N) {
    set_error("FinalizePopulationSize: number of haplotypes in anc/mut (%d) does not match number of samples in .poplabels file (%zu haplotypes)", N, group_of_haplotype.size());
    return RL_EINVAL;
  }
  std::vector<float> ep((size_t)E), data((size_t)E * N * N);
  if ((rc = rl_coalrate_read_bin(bin_path, ep.data(), &E, data.data(), &N))) return rc;
  const size_t G = poplabels_or_null ? groups.size() : 1;
  std::vector<double> rates(G * G * E);
  if ((rc = rl_coalrate_finalize(data.data(), N, E, poplabels_or_null ? group_of_haplotype.data() : nullptr, (int)G, rates.data()))) return rc;
  std::ofstream os(coal_path);  // FinalizePopulationSize.cpp:93-114, :239-277: operator<< of string, float, int, double
  if (os.fail()) {
    set_error("FinalizePopulationSize: error while opening file %s", coal_path);
    return RL_EIO;
  }
  if (!poplabels_or_null) os << "group1\n";
  else {
    for (const std::string &gname : groups) os << gname << " ";
    os << "\n";
  }
  for (int e = 0; e < E; e++) os << ep[e] << " ";
  os << "\n";
  for (size_t i = 0; i < G; i++)
    for (size_t j = 0; j < G; j++) {
      os << i << " " << j << " ";
      for (int e = 0; e < E; e++) os << rates[(i * G + j) * E + e] << " ";
      os << "\n";
    }
  os.close();
  if (os.fail()) {
    set_error("FinalizePopulationSize: writing %s failed", coal_path);
    return RL_EIO;
  }
  return RL_OK;
}

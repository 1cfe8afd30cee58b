// tree_host.cpp -- see tree_host.h.
#include "tree_host.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "common.h"

namespace rl {

int first_bad_node(const int *parent, int N, std::vector<unsigned char> &kids) {
  const int nodes = 2 * N - 1;
  kids.assign((size_t)nodes, 0);
  for (int v = 0; v < nodes - 1; v++) {
    const int p = parent[v];
    if (!(p > v && p >= N && p < nodes) || ++kids[p] > 2) return v + 1;
  }
  if (parent[nodes - 1] != -1) return nodes;
  for (int v = N; v < nodes; v++)
    if (kids[v] != 2) return v + 1;
  return 0;
}

int refuse_tree(const char *tree, const int *parent, int N) {
  std::vector<unsigned char> kids;
  const int bad = first_bad_node(parent, N, kids);
  const int v = bad - 1;
  if (bad == 0) set_error("%s was refused by the device and not by the host", tree);
  else if (v == 2 * N - 2) set_error("%s: node %d is not the root (parent %d, expected -1) or has not two children", tree, v, parent[v]);
  else if (parent[v] <= v) set_error("%s: parent %d of node %d does not have a label above its child's", tree, parent[v], v);
  else set_error("%s: node %d (parent %d) does not fit a binary tree on %d leaves", tree, v, parent[v], N);
  return RL_EINVAL;
}

int first_bad_length(const double *bl, int count) {
  for (int v = 0; v < count; v++)
    if (!(bl[v] >= 0.0 && bl[v] <= DBL_MAX)) return v + 1;
  return 0;
}

int check_tree(const char *tree_name, const int *parent, const double *bl_or_null, int N, int n_lengths,
               bool refused_by_device, std::vector<unsigned char> &kids) {
  if (first_bad_node(parent, N, kids)) return refuse_tree(tree_name, parent, N);
  if (const int v = bl_or_null ? first_bad_length(bl_or_null, n_lengths) : 0) {
    set_error("%s: branch length %g of node %d is negative or not finite", tree_name, bl_or_null[v - 1], v - 1);
    return RL_EINVAL;
  }
  return refused_by_device ? refuse_tree(tree_name, parent, N) : RL_OK;  // (refused by the device and not by the host)
}

template <class T>
int check_epochs(const char *who, const T *ep, int E, int max_epochs) {
  if (E < 2 || E > max_epochs) {
    set_error("%s: 2 <= epochs <= %d (%d given)", who, max_epochs, E);
    return RL_EINVAL;
  }
  if (ep[0] != (T)0) {
    set_error("%s: the first epoch boundary is %g, not 0", who, (double)ep[0]);
    return RL_EINVAL;
  }
  for (int e = 1; e < E; e++)
    if (!(ep[e] > ep[e - 1] && ep[e] <= std::numeric_limits<T>::max())) {
      set_error("%s: epoch boundary %d (%g) is not finite and above boundary %d (%g)", who, e, (double)ep[e], e - 1, (double)ep[e - 1]);
      return RL_EINVAL;
    }
  return RL_OK;
}
template int check_epochs<float>(const char *, const float *, int, int);
template int check_epochs<double>(const char *, const double *, int, int);

// every boundary is stored in a T as it is made, and the last one of --bins is computed from the stored one
template <class T>
int make_epochs(const char *who, float years_per_gen, const char *bins_or_null, T *out, int *nepochs) {
  if (!out || !nepochs) return null_args(who);
  if (!(years_per_gen > 0.0f && years_per_gen <= FLT_MAX)) {
    set_error("%s: years_per_gen %g is not positive and finite", who, (double)years_per_gen);
    return RL_EINVAL;
  }
  const int cap = *nepochs;
  std::vector<T> ep;
  const float log_10 = std::log(10);
  if (bins_or_null) {
    double v[3];
    const char *p = bins_or_null;
    for (int k = 0; k < 3; k++) {
      char *end = nullptr;
      v[k] = strtof(p, &end);  // (std::stof)
      if (end == p || (k < 2 && *end != ',') || (k == 2 && *end != '\0' && *end != ',')) {
        set_error("%s: bins `%s`: epochs format is wrong. Specify x,y,stepsize.", who, bins_or_null);
        return RL_EINVAL;
      }
      p = end + 1;
    }
    const double lower = v[0], upper = v[1], step = v[2];
    if (!(step > 0.0) || !(std::fabs(lower) <= 1e30) || !(std::fabs(upper) <= 1e30) || (upper - lower) / step > 1e6) {
      set_error("%s: bins `%s`: the step must be positive and the range finite", who, bins_or_null);
      return RL_EINVAL;
    }
    ep.push_back(0.0);
    for (double boundary = lower; boundary < upper; boundary += step) ep.push_back(std::exp(log_10 * boundary) / years_per_gen);
    ep.push_back(std::exp(log_10 * upper) / years_per_gen);
    ep.push_back(std::max(1e8, 10.0 * ep[ep.size() - 1]) / years_per_gen);
  } else {
    const int E = 31;
    ep.resize(E);
    ep[0] = 0.0;
    ep[1] = 1e3 / years_per_gen;
    for (int e = 2; e < E - 1; e++) ep[e] = std::exp(log_10 * (3.0 + 4.0 * (e - 1.0) / (E - 3.0))) / years_per_gen;
    ep[E - 1] = 1e8 / years_per_gen;
  }
  *nepochs = (int)ep.size();
  if ((int)ep.size() > cap) {
    set_error("%s: %zu epoch boundaries, room for %d", who, ep.size(), cap);
    return RL_EINVAL;
  }
  memcpy(out, ep.data(), ep.size() * sizeof(T));
  return RL_OK;
}
template int make_epochs<float>(const char *, float, const char *, float *, int *);
template int make_epochs<double>(const char *, float, const char *, double *, int *);

void TreeTables::fill(const int *parent) {
  std::fill(first.begin(), first.end(), -1);
  for (int v = 0; v < nodes; v++) size[v] = v < N ? 1 : 0;
  for (int v = 0; v < nodes - 1; v++) {  // label order: a node is complete before its parent reads it
    const int p = parent[v];
    size[p] += size[v];
    if (first[p] == -1) first[p] = v;
    else second[p] = v;
  }
  lo[nodes - 1] = 0;
  for (int p = nodes - 1; p >= N; p--) {  // falling order: a parent hands the left ends down
    lo[first[p]] = lo[p];
    lo[second[p]] = lo[p] + size[first[p]];
  }
}

void flatten_anc(const AncFile &a, std::vector<int> &parents, std::vector<double> *branch_length) {
  const size_t nodes = (size_t)2 * a.N - 1, T = a.trees.size();
  parents.resize(T * nodes);
  if (branch_length) branch_length->resize(T * nodes);
  for (size_t t = 0; t < T; t++) {
    memcpy(&parents[t * nodes], a.trees[t].parent.data(), nodes * sizeof(int));
    if (branch_length) memcpy(&(*branch_length)[t * nodes], a.trees[t].branch_length.data(), nodes * sizeof(double));
  }
}

}  // namespace rl

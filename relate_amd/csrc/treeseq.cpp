// treeseq.cpp -- the tree-sequence loop of one section.
//
// Host restatement of AncesTreeBuilder::BuildTopology (src/anc_builder.cpp:398-656),
// MapMutation / ForceMapMutation / PropagateMutation* (:1064-1413), the .anc
// writer AncesTree::DumpBin (src/anc.cpp:1104-1167) and the .mut writer
// Mutations::DumpShortFormat (src/mutations.cpp:548-581), for the
// configuration the stage driver uses (pipeline/BuildTopology.cpp:14-167; stage.cpp):
// ancestral_state = true, sample_ages empty.
//
// Distance matrices come from a provider (callbacks): the stage wires the GPU
// rl_window in; nothing here computes painting on the CPU.
#include <algorithm>
#include <atomic>
#include <climits>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <thread>

#include "common.h"
#include "minmatch.h"
#include "treeseq.h"

namespace rl {

// ---- Where a SNP sits on a tree (anc_builder.cpp:1064-1413: MapMutation, ForceMapMutation and their two
// recursions PropagateMutationGlobal / PropagateMutationLocal).
//
// The reference walks the tree recursively and carries eight counters per call.  Everything it decides at a node
// follows from two numbers -- the carriers and the leaves below it -- and from what its two children decided, so
// here the tree is swept once, bottom-up, over flat arrays:
//   * MinMatch labels a merged node N + (merge index): children always carry smaller labels than their parent, so
//     the label order 0 .. 2N-2 IS a bottom-up order (no stack, no recursion 5000 deep);
//   * for the orders in which the reference *emits* branches (ForceMapMutation's lists) the post-order of the
//     recursion (left subtree, right subtree, node) is made explicit once per call.
// Float semantics kept: every ratio is a float division compared against the double literals 0.3 / 0.7 / 0.03.

// A branch and how many leaves it misplaces; `leaves == INT_MAX`: no admissible branch in the subtree.
struct Fit {
  int leaves = INT_MAX;
  int branch = -1;
};

// the two ratio tests every clade has to pass in either orientation (:1265-1279, :1295-1310)
static inline bool small_share(int part, float whole) { return (float)part / whole < 0.3; }
static inline bool pure(int agreeing, int all) { return all <= 0 || (float)agreeing / (float)all > 0.7; }

// MapMutation's search (:1237-1341): over all branches, the one whose clade is closest to the carrier set -- as it
// stands (`direct`: the leaves below carry the derived allele) and with the alleles flipped (`flipped`).  A clade
// replaces the best of its subtrees only when strictly better than both; of two subtrees the left one keeps ties.
static void best_branches(const rl_treeseq &ts, const HostTree &t, Fit &direct_root, Fit &flipped_root) {
  const int N = ts.N, T = 2 * N - 1;
  const float carriers = (float)ts.num_carriers, others = (float)N - carriers;
  static thread_local std::vector<int> below_c, below_n;  // carriers / non-carriers below each node
  static thread_local std::vector<Fit> direct, flipped;
  below_c.resize(T);
  below_n.resize(T);
  direct.resize(T);
  flipped.resize(T);
  for (int v = 0; v < N; v++) {  // leaves (:1313-1339): one ratio test per orientation, two for the "wrong" allele
    const int c = ts.member[v] == 1 ? 1 : 0, in_c = c, in_n = 1 - c;
    const int out_c = (int)(carriers - (float)in_c), out_n = (int)(others - (float)in_n);
    below_c[v] = in_c;
    below_n[v] = in_n;
    Fit d, f;
    if (c) {
      if (small_share(out_c, carriers)) d = Fit{out_c, v};
      if (small_share(in_c, carriers) && small_share(out_n, others)) f = Fit{out_n + in_c, v};
    } else {
      if (small_share(out_c, carriers) && small_share(in_n, others)) d = Fit{out_c + in_n, v};
      if (small_share(out_n, others)) f = Fit{out_n, v};
    }
    direct[v] = d;
    flipped[v] = f;
  }
  for (int v = N; v < T; v++) {
    const int l = t.child_left[v], r = t.child_right[v];
    const int in_c = below_c[l] + below_c[r], in_n = below_n[l] + below_n[r];
    const int out_c = (int)(carriers - (float)in_c), out_n = (int)(others - (float)in_n);
    below_c[v] = in_c;
    below_n[v] = in_n;
    {  // as it stands: carriers outside and non-carriers inside are the misplaced leaves
      const int wrong = out_c + in_n;
      const bool ok = small_share(out_c, carriers) && small_share(in_n, others) && pure(in_c, in_c + in_n) &&
                      pure(out_n, out_c + out_n);
      if (ok && direct[l].leaves > wrong && direct[r].leaves > wrong)
        direct[v] = Fit{wrong, v};
      else
        direct[v] = direct[l].leaves > direct[r].leaves ? direct[r] : direct[l];
    }
    {  // flipped: carriers inside and non-carriers outside
      const int wrong = in_c + out_n;
      const bool ok = small_share(in_c, carriers) && small_share(out_n, others) && pure(out_c, out_c + out_n) &&
                      pure(in_n, in_c + in_n);
      if (ok && flipped[l].leaves > wrong && flipped[r].leaves > wrong)
        flipped[v] = Fit{wrong, v};
      else
        flipped[v] = flipped[l].leaves > flipped[r].leaves ? flipped[r] : flipped[l];
    }
  }
  direct_root = direct[T - 1];
  flipped_root = flipped[T - 1];
}

// MapMutation (:1064-1139, the version without random flipping): 1 = the SNP maps, 2 = maps with the alleles
// flipped, 3 = no branch within the tolerance (si untouched).  misfit: the misplaced leaves of the best branch.
static int map_mutation(rl_treeseq &ts, HostTree &t, SnpInfo &si, float &misfit, bool count_event) {
  const int N = ts.N, root = 2 * N - 2;
  if (ts.num_carriers == 0 || ts.num_carriers == N) {  // nothing to place; a fixed site sits on the root branch
    misfit = 0.0f;
    si.flipped = false;
    si.branch.clear();
    if (ts.num_carriers == N) {
      si.branch.push_back(root);
      t.num_events[root] += 1.0f;  // (counted whatever the SNP's state, :1075)
    }
    return 1;
  }
  Fit direct, flipped;
  best_branches(ts, t, direct, flipped);
  const bool as_is = direct.leaves <= flipped.leaves;  // (ties go to the unflipped reading)
  const Fit &best = as_is ? direct : flipped;
  misfit = (float)best.leaves;
  if (best.leaves > ts.thr) return 3;
  si.branch.assign(1, best.branch);
  si.flipped = !as_is;
  if (count_event) t.num_events[best.branch] += 1.0f;
  return as_is ? 1 : 2;
}

// ForceMapMutation (:1143-1204) with PropagateMutationLocal (:1344-1413): a SNP that fits no single branch goes
// onto the maximal clades that are (almost, < 3 % of their leaves) pure in carriers -- or, flipped, in non-carriers
// -- whichever reading needs fewer branches.  A clade stays "open" while it is pure and both children are open; its
// branch is the node itself if both children hold leaves of the kind, else the one child's branch.  When a clade
// closes, its children's open branches are emitted (left, then right) -- in the order the recursion reaches the
// closing nodes, i.e. post-order, which the sweep below follows through an explicit list.
static void force_map_mutation(rl_treeseq &ts, const HostTree &t, SnpInfo &si) {
  const int N = ts.N, T = 2 * N - 1;
  if (ts.num_carriers == 0 || ts.num_carriers == N) return;
  static thread_local std::vector<int> post, stack, kind_count[2], open_branch[2];
  post.clear();
  stack.assign(1, T - 1);
  while (!stack.empty()) {  // (root, right, left) reversed = (left, right, root)
    const int v = stack.back();
    stack.pop_back();
    post.push_back(v);
    if (t.child_left[v] >= 0) {
      stack.push_back(t.child_left[v]);
      stack.push_back(t.child_right[v]);
    }
  }
  std::reverse(post.begin(), post.end());
  std::vector<int> emitted[2];  // [0] carriers' clades, [1] non-carriers' clades (the flipped reading)
  for (int s = 0; s < 2; s++) {
    kind_count[s].resize(T);
    open_branch[s].resize(T);
  }
  for (int v : post) {
    const int l = t.child_left[v], r = t.child_right[v];
    if (l < 0) {
      const int s = ts.member[v] == 1 ? 0 : 1;
      kind_count[s][v] = 1;
      kind_count[1 - s][v] = 0;
      open_branch[s][v] = v;
      open_branch[1 - s][v] = -1;
      continue;
    }
    const int n0 = kind_count[0][l] + kind_count[0][r], n1 = kind_count[1][l] + kind_count[1][r];
    kind_count[0][v] = n0;
    kind_count[1][v] = n1;
    const float leaves = (float)(n0 + n1);
    for (int s = 0; s < 2; s++) {
      const int foreign = s == 0 ? n1 : n0;
      const int bl = open_branch[s][l], br = open_branch[s][r];
      if ((float)foreign / leaves < 0.03 && bl != -1 && br != -1) {
        const bool in_l = kind_count[s][l] > 0, in_r = kind_count[s][r] > 0;
        open_branch[s][v] = in_l && in_r ? v : (in_l ? bl : br);
      } else {
        if (bl != -1) emitted[s].push_back(bl);
        if (br != -1) emitted[s].push_back(br);
        open_branch[s][v] = -1;
      }
    }
  }
  // fewer branches win, the unflipped reading on ties -- unless it found none (:1180-1203)
  const bool as_is = emitted[1].empty() || (!emitted[0].empty() && emitted[0].size() <= emitted[1].size());
  if (!as_is) si.flipped = true;
  si.branch = emitted[as_is ? 0 : 1];
}

// Prior `dist` from the previous tree's clades (anc_builder.cpp:583-606):
// dist[i][j] = val added once per clade that contains i but not j.  Computed
// here per pair from leaf depths and the depth of the pair's lowest common
// ancestor; the repeated float additions of `val` are replayed through a table
// (acc[c] = val added c times, left to right), so every entry is bit-identical
// to the reference's accumulation.
// f(row) for row = 0..N-1 on the tree builder's share of host threads (minmatch.h build_threads)
template <typename F>
static void parallel_rows(int N, F f) {
  const int T = std::min(build_threads(), std::max(1, N / 256));
  if (T <= 1) {
    for (int r = 0; r < N; r++) f(r);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < T; t++)
    th.emplace_back([=]() {
      for (int r = t; r < N; r += T) f(r);
    });
  for (auto &x : th) x.join();
}

// dist[a][b] = val added (#clades of the previous tree that contain a but not b) times, accumulated in
// float as the reference does (:588-606): the clades containing a but not b are a's internal ancestors
// strictly below lca(a, b).  Row a is filled ancestor by ancestor: for ancestor v, the leaves below v's other
// child have their lca with a at v; leaves below a node are a contiguous range of a depth-first leaf order.
static void clade_prior(const HostTree &t, float val, MatrixBuf &dist) {
  const int N = t.N, T = 2 * N - 1;
  dist.resize((size_t)N * N);
  std::vector<float> acc((size_t)N + 1, 0.0f);
  for (int c = 1; c <= N; c++) acc[c] = acc[c - 1] + val;
  // depth of every node, and a depth-first leaf order with [lo, lo + size) of every node (minmatch.h)
  std::vector<int> depth(T), size(T), lo(T), order(N);
  clade_tables(t, N, depth.data(), size.data(), lo.data(), order.data());
  parallel_rows(N, [&](int a) {
    float *row = &dist[(size_t)a * N];
    row[a] = 0.0f;
    const int da = depth[t.parent[a]];
    int child = a;
    for (int v = t.parent[a]; v >= 0; child = v, v = t.parent[v]) {
      const int other = t.child_left[v] == child ? t.child_right[v] : t.child_left[v];
      const float x = acc[da - depth[v]];
      for (int p = lo[other]; p < lo[other] + size[other]; p++) row[order[p]] = x;
    }
  });
}

// carrier penalty (:563-581): d[c][*] += val, then d[c][c'] -= val
static void carrier_penalty_host(MatrixBuf &d, int N, const std::vector<char> &member, float val) {
  parallel_rows(N, [&](int c) {
    if (member[c]) {
      float *row = &d[(size_t)c * N];
      for (int col = 0; col < N; col++) row[col] += val;
      for (int c2 = 0; c2 < N; c2++)
        if (member[c2]) row[c2] -= val;
    }
  });
}

// A tree from the device-resident path: the distance matrix of `snp` written on the device -- by the provider that
// also applies the carrier penalty (`carriers`, `val`) and leaves the row minima, if the caller has one and wants it
// (`with_rowmin`) --, then on_device(row minima done?): whatever the caller applies to the staged matrix and the build
// itself, a DeviceMinMatch status.  0: the tree is the device's.  > 0: the device hands this tree to the host (more tied
// candidates than its lists hold, or no room for the symmetric matrix): the device matrices are half merged by now and
// the host builder's state untouched, so on_host() fetches the matrix again, to the host, and builds there.
template <class OnDevice, class OnHost>
static int resident_tree(rl_treeseq *ts, DeviceMinMatch *dev, void *user, int snp, bool with_rowmin, const char *carriers,
                         float val, OnDevice on_device, OnHost on_host) {
  float *dd = dev->device_matrix();
  if (!dd) return RL_ENOMEM;
  int rc;
  float *rmin = with_rowmin && ts->matrix_dev_ex ? dev->rowmin_device() : nullptr;
  if (rmin) {  // the penalty and the row minima in the matrix kernel's own last pass over each row
    if ((rc = ts->matrix_dev_ex(user, snp, dd, carriers, val, rmin))) return rc;
    dev->rowmin_is_ready();
  } else if ((rc = ts->matrix_dev(user, snp, dd))) {
    return rc;
  }
  const int st = on_device(rmin != nullptr);
  if (st < 0) {
    set_error("tree builder on the device failed at SNP %d", snp);
    return RL_EHIP;
  }
  if (st > 0) return on_host();
  ts->gpu_trees++;
  return RL_OK;
}

}  // namespace rl

using namespace rl;

extern "C" {

rl_treeseq *rl_treeseq_create(int N, int L, const uint32_t *bits, int row_words, const double *rpos,
                              const int *bp_pos, const int *state, double theta) {
  if (N < 2 || L < 2 || !bits || row_words < (N + 31) / 32 || !rpos || !(theta > 0.0 && theta < 1.0)) {
    set_error("rl_treeseq_create: bad arguments");
    return nullptr;
  }
  rl_treeseq *ts = new rl_treeseq();
  ts->N = N;
  ts->L = L;
  ts->theta = theta;
  ts->row_words = row_words;
  ts->bits_own.assign(bits, bits + (size_t)L * row_words);
  ts->bits = ts->bits_own.data();
  ts->rpos.assign(rpos, rpos + L + 1);
  if (bp_pos) ts->bp.assign(bp_pos, bp_pos + L);
  if (state)
    ts->state.assign(state, state + L);
  else
    ts->state.assign(L, 1);
  ts->thr = (int)(0.03 * N);  // anc_builder.cpp:383
  ts->member.assign(N, 0);
  return ts;
}

void rl_treeseq_destroy(rl_treeseq *ts) { delete ts; }

}  // extern "C"

// as rl_treeseq_create, the panel borrowed instead of copied (also used by shard.cpp)
namespace rl {
rl_treeseq *treeseq_borrowing(int N, int L, const uint32_t *bits, int row_words, const double *rpos,
                                     const int *bp_pos, const int *state, double theta) {
  rl_treeseq *ts = new rl_treeseq();
  ts->N = N;
  ts->L = L;
  ts->theta = theta;
  ts->row_words = row_words;
  ts->bits = bits;
  ts->rpos.assign(rpos, rpos + L + 1);
  ts->bp.assign(bp_pos, bp_pos + L);
  ts->state.assign(state, state + L);
  ts->thr = (int)(0.03 * N);  // anc_builder.cpp:383
  ts->member.assign(N, 0);
  return ts;
}
}  // namespace rl

extern "C" {

int rl_treeseq_build(rl_treeseq *ts, int start, int end, rl_matrix_fn matrix, rl_advance_fn advance, void *user,
                     int flags, int fb) {
  if (!ts || !matrix || start < 0 || end >= ts->L || start > end) {
    set_error("rl_treeseq_build: bad arguments");
    return RL_EINVAL;
  }
  if (fb > 0 && ts->bp.empty()) {
    set_error("rl_treeseq_build: --fb needs bp positions");
    return RL_EINVAL;
  }
  const int N = ts->N;
  const bool consistency = !(flags & 1);
  ts->start = start;
  ts->end = end;
  ts->trees.clear();
  ts->info.assign((size_t)(end - start + 1), SnpInfo());
  // carriers: the reference fills them for snp < section_endpos only, so the
  // last SNP of a window is processed with none (anc_builder.cpp:407-414)
  auto set_carriers = [&](int snp) {
    ts->num_carriers = 0;
    std::fill(ts->member.begin(), ts->member.end(), 0);
    if (snp < end)
      for (int i = 0; i < N; i++)
        if (ts->derived(snp, i)) {
          ts->member[i] = 1;
          ts->num_carriers++;
        }
  };
  MinMatch tb(N, ts->theta);
  // with sample ages (ancient samples) the candidates carry a third key and a clock: its own builder (and its own
  // workers on the device, minmatch_worker.hip AGES)
  std::unique_ptr<MinMatchAges> tb_ages;
  if ((int)ts->sample_ages.size() == N) tb_ages.reset(new MinMatchAges(N, ts->theta));
  DeviceMinMatch *dev = nullptr;
  if (ts->build_device >= 0 && N <= 10240) {  // (its registers per thread)
    if (!ts->dev_builder) ts->dev_builder = new DeviceMinMatch(N, ts->build_device);
    dev = ts->dev_builder;
  }
  int build_rc = 0;
  auto host_build = [&](float *dm, const float *prior, HostTree &t) {
    ts->host_trees++;
    if (tb_ages) tb_ages->quick_build(dm, prior, ts->sample_ages, t);
    else tb.quick_build(dm, prior, t);
  };
  auto build_tree = [&](float *dm, const float *prior, HostTree &t) {
    if (dev) {
      const int st = tb_ages ? dev->build(*tb_ages, ts->sample_ages, dm, prior, t) : dev->build(tb, dm, prior, t);
      if (st == 0) {
        ts->gpu_trees++;
        return;
      }
      if (st < 0) build_rc = RL_EHIP;
    }
    host_build(dm, prior, t);
  };
  auto build_resident = [&](bool with_prior, HostTree &t) {
    return tb_ages ? dev->build_resident(*tb_ages, ts->sample_ages, with_prior, t) : dev->build_resident(tb, with_prior, t);
  };
  MatrixBuf d((size_t)N * N), dist;
  float min_value = 0.f, min_value_alt = 0.f;
  int rc;
  const bool resident = dev && ts->matrix_dev;
  const float val = -std::log(ts->theta / (1.0 - ts->theta));  // :555
  // RELATE_AMD_TIMING=1: where a section's wall-clock goes (stderr)
  const bool timing = timing_level() >= 1;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_matrix = 0, t_prior = 0, t_build = 0, t_map = 0, t_mark = 0;
  auto lap = [&](double &acc) {
    const double t = now();
    acc += t - t_mark;
    t_mark = t;
  };
  // The distance matrix of `snp` on the host and, with `prev` (the tree before, when the call keeps trees consistent),
  // the carrier penalty in it and the clade prior in `dist`; `timed`: the laps of the host path.
  auto host_matrix = [&](int snp, const HostTree *prev, bool timed) -> int {
    if (int r = matrix(user, snp, d.data())) return r;
    if (!prev) return RL_OK;
    if (timed) lap(t_matrix);
    carrier_penalty_host(d, N, ts->member, val);
    clade_prior(*prev, val, dist);
    if (timed) lap(t_prior);
    return RL_OK;
  };
  // The tree of `snp` into t.  A section's first tree has neither penalty nor prior (:447) and is not in the laps.
  auto new_tree = [&](int snp, const HostTree *prev, bool first, HostTree &t) -> int {
    if (!resident) {
      if (int r = host_matrix(snp, prev, true)) return r;
      build_tree(d.data(), prev ? dist.data() : nullptr, t);
      return build_rc;
    }
    // matrix, carrier penalty, clade prior and the build itself on the device
    return resident_tree(
        ts, dev, user, snp, true, prev ? ts->member.data() : nullptr, first ? 0.0f : val,
        [&](bool rowmin_done) {
          if (first) return build_resident(false, t);  // (the row minima alone)
          lap(t_matrix);
          int st = 0;
          if (prev) {
            if (!rowmin_done) st = dev->apply_penalty(ts->member.data(), val);
            st = st ? st : dev->apply_prior(*prev, val);
            lap(t_prior);
          }
          return st ? st : build_resident(prev != nullptr, t);
        },
        [&]() -> int {  // with the penalty and the prior of the host path
          if (int r = host_matrix(snp, prev, false)) return r;
          host_build(d.data(), prev ? dist.data() : nullptr, t);
          return RL_OK;
        });
  };

  ts->trees.emplace_back();
  if ((rc = new_tree(start, nullptr, true, ts->trees.back()))) return rc;
  ts->trees.back().pos = start;
  std::fill(ts->trees.back().snp_begin.begin(), ts->trees.back().snp_begin.end(), start);
  set_carriers(start);
  ts->info[0].tree = 0;
  int is_mapping = map_mutation(*ts, ts->trees.back(), ts->info[0], min_value, ts->state[start] != 0);
  if (is_mapping > 2) force_map_mutation(*ts, ts->trees.back(), ts->info[0]);

  int num_tree = 1, builds = 0;
  for (int snp = start + 1; snp <= end; snp++) {
    SnpInfo &si = ts->info[(size_t)(snp - start)];
    set_carriers(snp);
    if (advance && snp < end && (rc = advance(user, snp))) return rc;  // :487-495 (carriers only)
    si.tree = num_tree - 1;
    const bool use = ts->state[snp] != 0;
    t_mark = now();
    is_mapping = map_mutation(*ts, ts->trees.back(), si, min_value, use);
    lap(t_map);
    bool force_new = false;
    if (snp < end && fb > 0)
      if (((int)(ts->bp[snp + 1] / fb)) - ((int)(ts->bp[snp] / fb)) >= 1) force_new = true;

    if (is_mapping > 1 || force_new) {
      int prev_branch = -1;
      if (is_mapping == 2 || (is_mapping == 1 && force_new)) prev_branch = si.branch[0];
      ts->trees.emplace_back();
      HostTree &nt = ts->trees.back();
      HostTree &pt = ts->trees[ts->trees.size() - 2];
      t_mark = now();
      builds++;
      if ((rc = new_tree(snp, consistency ? &pt : nullptr, false, nt))) return rc;
      lap(t_build);
      nt.pos = snp;
      const int is_mapping_alt = map_mutation(*ts, nt, si, min_value_alt, use);
      lap(t_map);
      if (is_mapping_alt > 1 && min_value_alt >= min_value && !force_new) {
        // new tree is not better: keep the old one (:621-630)
        if (is_mapping == 2) si.branch[0] = prev_branch;
        ts->trees.pop_back();
        if (is_mapping > 2) force_map_mutation(*ts, ts->trees.back(), si);
      } else {
        if (is_mapping == 2 || (is_mapping == 1 && force_new)) {
          if (use) pt.num_events[prev_branch] -= 1.0f;
        }
        if (is_mapping_alt > 2) force_map_mutation(*ts, nt, si);
        si.tree = num_tree;
        std::fill(pt.snp_end.begin(), pt.snp_end.end(), snp);
        std::fill(nt.snp_begin.begin(), nt.snp_begin.end(), snp);
        num_tree++;
      }
    }
  }
  std::fill(ts->trees.back().snp_end.begin(), ts->trees.back().snp_end.end(), end);
  if (timing) {
    // (the host builder's own phases only when it built trees: for the device's workers the per-phase times are the
    //  "[gpu tree builder]" lines, one per tree, and its host side the line the builder prints when it is destroyed)
    char host_phases[256] = "";
    if (ts->host_trees > 0)
      snprintf(host_phases, sizeof host_phases,
               "; host builder: row minima + pair scan %.2f, merges: parallel part %.2f [updates %.2f] + ordered part "
               "%.2f, %.2f rebuilt clusters per merge", tb.t_init, tb.t_phase1, tb.t_phase1a, tb.t_phase2,
               (double)tb.n_updated / std::max<long long>(1, tb.n_merges));
    fprintf(stderr,
            "[tree sequence] SNPs %d..%d: %d trees kept of %d built; distance matrices %.2f s, penalty + clade prior "
            "%.2f s, tree builds %.2f s (%lld trees on the GPU, %lld on the host%s), mutation mapping %.2f s\n",
            start, end, num_tree, builds + 1, t_matrix, t_prior, t_build, ts->gpu_trees, ts->host_trees, host_phases, t_map);
  }
  return RL_OK;
}

int rl_treeseq_set_sample_ages(rl_treeseq *ts, const double *ages, int n) {
  if (!ts || (n != 0 && (n != ts->N || !ages))) {
    rl::set_error("rl_treeseq_set_sample_ages: one age per haplotype (%d), or none", ts ? ts->N : 0);
    return RL_EINVAL;
  }
  ts->sample_ages.assign(ages, ages + n);
  if (ts->dev_builder) ts->dev_builder->forget_ages();
  return RL_OK;
}

int rl_treeseq_set_build_device(rl_treeseq *ts, int device) {
  if (!ts) return RL_EINVAL;
  if (ts->dev_builder && device != ts->build_device) {
    delete ts->dev_builder;
    ts->dev_builder = nullptr;
  }
  ts->build_device = device;
  return RL_OK;
}

int rl_treeseq_set_device_matrix_ex(rl_treeseq *ts, rl_matrix_dev_ex_fn matrix_dev_ex) {
  if (!ts) return RL_EINVAL;
  ts->matrix_dev_ex = matrix_dev_ex;
  return RL_OK;
}

int rl_treeseq_set_device_matrix(rl_treeseq *ts, rl_matrix_dev_fn matrix_dev) {
  if (!ts) return RL_EINVAL;
  ts->matrix_dev = matrix_dev;
  return RL_OK;
}

int rl_treeseq_num_trees(const rl_treeseq *ts) { return ts ? (int)ts->trees.size() : RL_EINVAL; }

int rl_treeseq_get_tree(const rl_treeseq *ts, int t, int *pos, int *parent) {
  if (!ts || t < 0 || t >= (int)ts->trees.size()) return RL_EINVAL;
  if (pos) *pos = ts->trees[t].pos;
  if (parent) memcpy(parent, ts->trees[t].parent.data(), sizeof(int) * (2 * ts->N - 1));
  return RL_OK;
}

// AncesTree::DumpBin (anc.cpp:1104-1167) and Mutations::DumpShortFormat (mutations.cpp:548-581)
int rl_treeseq_write(const rl_treeseq *ts, const char *anc_path, const char *mut_path) {
  if (!ts || ts->trees.empty()) {
    set_error("rl_treeseq_write: nothing built");
    return RL_ESTATE;
  }
  const int N = ts->N, T = 2 * N - 1;
  if (anc_path) {
    FILE *fp = fopen(anc_path, "wb");
    if (!fp) {
      set_error("cannot open %s for writing", anc_path);
      return RL_EIO;
    }
    const unsigned char has_ages = 0;
    const unsigned int uN = N, nt = (unsigned int)ts->trees.size();
    fwrite(&has_ages, 1, 1, fp);
    fwrite(&uN, 4, 1, fp);
    fwrite(&nt, 4, 1, fp);
    std::vector<unsigned char> buf((size_t)T * 24);
    for (const HostTree &t : ts->trees) {
      fwrite(&t.pos, 4, 1, fp);
      const double bl = 0.0;
      for (int i = 0; i < T; i++) {
        unsigned char *p = &buf[(size_t)i * 24];
        memcpy(p, &t.parent[i], 4);
        memcpy(p + 4, &bl, 8);
        memcpy(p + 12, &t.num_events[i], 4);
        memcpy(p + 16, &t.snp_begin[i], 4);
        memcpy(p + 20, &t.snp_end[i], 4);
      }
      fwrite(buf.data(), 1, buf.size(), fp);
    }
    const bool bad = ferror(fp) != 0;
    if (fclose(fp) != 0 || bad) {  // (a full disc must not pass for a tree sequence)
      set_error("writing %s failed", anc_path);
      return RL_EIO;
    }
  }
  if (mut_path) {
    FILE *fp = fopen(mut_path, "w");
    if (!fp) {
      set_error("cannot open %s for writing", mut_path);
      return RL_EIO;
    }
    fputs("tree_index;branch_index;is_mapping;is_flipped;age_of_mutation\n", fp);
    for (const SnpInfo &si : ts->info) {
      fprintf(fp, "%d;", si.tree);
      for (size_t b = 0; b < si.branch.size(); b++) fprintf(fp, b ? " %d" : "%d", si.branch[b]);
      fputs(si.branch.size() > 1 ? ";1;" : ";0;", fp);
      fprintf(fp, "%d;0;0;\n", si.flipped ? 1 : 0);
    }
    const bool bad = ferror(fp) != 0;
    if (fclose(fp) != 0 || bad) {
      set_error("writing %s failed", mut_path);
      return RL_EIO;
    }
  }
  return RL_OK;
}

}  // extern "C"

namespace rl {

// ---- `--mode OptimizeParameters`: one section (AncesTreeBuilder::OptimizeParameters, anc_builder.cpp:821-973) ------
// A tree at EVERY SNP start..end of the section, each from the distance matrix with the SNP "cancelled" (:869-882,
// :926-939) and without a prior (MinMatch::QuickBuild, tree_builder.cpp:1061-1303), by ONE MinMatch whose generator and
// carried state run on from tree to tree (:848); the SNP is then mapped onto its own tree (MapMutation without random
// flipping, :1064-1139) and counted when it comes back flipped or not mapping (> 1, :886, :962).  The tree is thrown
// away.  The cursors advance at every SNP after the first, the section's last included (:898-907 -- BuildTopology
// stops one short, :487-495), and the last SNP has its carriers like any other.  The first SNP's matrix is computed
// twice by the reference (:837, :867): the same matrix, once here.  The `seed` argument seeds a generator the path
// never draws from (:831), so there is none.  (What the sections of a grid point add up: OptRun, treeseq.h.)

// the cancellation on the host (the fallback's matrix; the device's is optimize_kernels.hip cancel_rowmin_kernel)
static void cancel_snp_host(float *d, int N, const char *member, float log_ratio) {
  for (int i = 0; i < N; i++) {
    if (!member[i]) continue;
    float *row = d + (size_t)i * N;
    float mn = std::numeric_limits<float>::infinity();
    for (int j = 0; j < N; j++) {
      if (!member[j]) row[j] += log_ratio;
      if (mn > row[j]) mn = row[j];
    }
    for (int j = 0; j < N; j++) row[j] -= mn;
  }
}

int optimize_section(rl_treeseq *ts, int start, int end, rl_window *win, OptRun &run) {
  const int N = ts->N;
  MinMatch tb(N, ts->theta);
  DeviceMinMatch *dev = nullptr;
  if (ts->build_device >= 0 && N <= 10240) {
    if (!ts->dev_builder) ts->dev_builder = new DeviceMinMatch(N, ts->build_device);
    dev = ts->dev_builder;
  }
  const bool resident = dev && ts->matrix_dev;
  MatrixBuf d;  // (the host's matrix: only when a tree is the host's)
  SnpInfo si;
  HostTree tree;
  int rc, not_mapping = 0;
  const long long gpu_before = ts->gpu_trees, host_before = ts->host_trees;
  for (int snp = start; snp <= end; snp++) {
    ts->num_carriers = 0;
    for (int i = 0; i < N; i++) {
      ts->member[i] = ts->derived(snp, i) ? 1 : 0;
      ts->num_carriers += ts->member[i];
    }
    if (snp > start && (rc = rl_window_advance(win, snp))) return rc;
    // the tree from a matrix on the host: by the device builder when that is how it gets its matrices, by the host's
    // when there is none or it hands the tree back (the symmetric fallback; tb untouched)
    auto host_matrix_tree = [&]() -> int {
      if (d.empty()) d.resize((size_t)N * N);
      if (int r = rl_window_matrix(win, snp, d.data(), nullptr)) return r;
      cancel_snp_host(d.data(), N, ts->member.data(), run.log_ratio);
      int st = 1;
      if (dev && !resident) {
        st = dev->build(tb, d.data(), nullptr, tree);
        if (st < 0) return RL_EHIP;
        if (st == 0) ts->gpu_trees++;
      }
      if (st > 0) {
        ts->host_trees++;
        tb.quick_build(d.data(), nullptr, tree);
      }
      return RL_OK;
    };
    if (resident)  // matrix, cancellation + row minima and the build on the device: no matrix crosses PCIe
      rc = resident_tree(ts, dev, win, snp, false, nullptr, 0.0f,
                         [&](bool) {
                           const int st = dev->apply_cancel(ts->member.data(), run.log_ratio);
                           return st ? st : dev->build_resident(tb, false, tree);
                         },
                         host_matrix_tree);
    else
      rc = host_matrix_tree();
    if (rc) return rc;
    float misfit = 0.0f;
    if (map_mutation(*ts, tree, si, misfit, true) > 1) not_mapping++;
  }
  run.count += not_mapping;
  run.trees += end - start + 1;
  run.gpu_trees += ts->gpu_trees - gpu_before;
  run.host_trees += ts->host_trees - host_before;
  return RL_OK;
}

}  // namespace rl

extern "C" {

// (measurement hook, tools/bench_builder_many.py) `builders` device builders, a host thread each, build the SAME tree
// `reps` times side by side -- the matrices stay on the device: a copy per build into the builder's staging pair, as
// K3 and the prior kernel would leave them -- with `workers` resident workgroups at most (0: the queue's own limit).
// seconds: wall-clock from the first submit to the last tree; mismatches: builds whose parent array differs from
// builder 0's of the same repetition (0 expected: every builder carries the same state through the same trees).
int rl_debug_builder_throughput(int N, double theta, int device, int builders, int reps, int workers, const float *d,
                                const float *prior, double *seconds, int *mismatches, int *first_parents) {
  if (N < 2 || builders < 1 || reps < 1 || !d || !seconds || !mismatches) return RL_EINVAL;
  RL_HIP(hipSetDevice(device));
  const size_t NN = (size_t)N * N;
  DevBuf masterD, masterCF;
  if (masterD.alloc(NN * 4) || (prior && masterCF.alloc(NN * 4))) return RL_ENOMEM;
  RL_HIP(hipMemcpy(masterD.p, d, NN * 4, hipMemcpyHostToDevice));
  if (prior) RL_HIP(hipMemcpy(masterCF.p, prior, NN * 4, hipMemcpyHostToDevice));
  std::vector<std::unique_ptr<MinMatch>> tbs;
  std::vector<std::unique_ptr<DeviceMinMatch>> devs;
  for (int b = 0; b < builders; b++) {
    tbs.emplace_back(new MinMatch(N, theta));
    devs.emplace_back(new DeviceMinMatch(N, device));
    if (devs.back()->reserve(false)) return RL_ENOMEM;
  }
  if (device_builder_expect(device, N, workers, false)) return RL_EHIP;
  std::vector<std::vector<int>> parents((size_t)builders * reps);
  std::atomic<int> ready(0), failed(0);
  std::atomic<bool> go(false);
  std::vector<std::thread> th;
  for (int b = 0; b < builders; b++)
    th.emplace_back([&, b] {
      (void)hipSetDevice(device);
      ready.fetch_add(1);
      while (!go.load()) std::this_thread::sleep_for(std::chrono::microseconds(50));
      for (int r = 0; r < reps && !failed.load(); r++) {
        HostTree t;
        if (devs[b]->stage_from_device(masterD.as<float>(), prior ? masterCF.as<float>() : nullptr) ||
            devs[b]->build_resident(*tbs[b], prior != nullptr, t) != 0) {
          failed.store(1);
          break;
        }
        parents[(size_t)b * reps + r].assign(t.parent.begin(), t.parent.begin() + (2 * N - 1));
      }
    });
  while (ready.load() < builders) std::this_thread::sleep_for(std::chrono::microseconds(100));
  const auto t0 = std::chrono::steady_clock::now();
  go.store(true);
  for (auto &x : th) x.join();
  *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  (void)device_builder_expect(device, N, 0, false);
  if (failed.load()) return RL_EHIP;
  int bad = 0;
  for (int b = 1; b < builders; b++)
    for (int r = 0; r < reps; r++) bad += parents[(size_t)b * reps + r] != parents[r];
  *mismatches = bad;
  if (first_parents)
    for (int r = 0; r < reps; r++) memcpy(first_parents + (size_t)r * (2 * N - 1), parents[r].data(), ((size_t)2 * N - 1) * 4);
  return RL_OK;
}

// Test hook (host only): AncesTreeBuilder::MapMutation without random flipping (anc_builder.cpp:1064-1139 with
// PropagateMutationGlobal, :1237-1341) on a tree given by its parent array.
int rl_debug_map_mutation(int N, const int *parent, const char *carriers) {
  if (N < 2 || !parent || !carriers) {
    set_error("rl_debug_map_mutation: bad arguments");
    return RL_EINVAL;
  }
  const int T = 2 * N - 1;
  HostTree t;
  t.reset(N);
  for (int v = 0; v < T; v++) {
    const int p = parent[v];
    if (v == T - 1 ? p != -1 : (p <= v || p < N || p >= T)) {  // (MinMatch's labels: a parent above its children)
      set_error("rl_debug_map_mutation: node %d has parent %d", v, p);
      return RL_EINVAL;
    }
    t.parent[v] = p;
    if (p < 0) continue;
    if (t.child_left[p] < 0) t.child_left[p] = v;
    else if (t.child_right[p] < 0) t.child_right[p] = v;
    else {
      set_error("rl_debug_map_mutation: node %d has more than two children", p);
      return RL_EINVAL;
    }
  }
  for (int v = N; v < T; v++)
    if (t.child_right[v] < 0) {
      set_error("rl_debug_map_mutation: internal node %d has fewer than two children", v);
      return RL_EINVAL;
    }
  std::vector<uint32_t> no_panel((size_t)((N + 31) / 32) * 2, 0u);
  std::vector<double> rpos(3, 0.0);
  std::vector<int> zeros(2, 0);
  rl_treeseq *ts = treeseq_borrowing(N, 2, no_panel.data(), (N + 31) / 32, rpos.data(), zeros.data(), zeros.data(), 0.001);
  for (int i = 0; i < N; i++) {
    ts->member[i] = carriers[i] ? 1 : 0;
    ts->num_carriers += ts->member[i];
  }
  SnpInfo si;
  float misfit = 0.0f;
  const int r = map_mutation(*ts, t, si, misfit, true);
  rl_treeseq_destroy(ts);
  return r;
}

}  // extern "C"

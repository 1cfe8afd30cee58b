// minmatch_builder.hip -- a tree of the GPU tree builder from its matrices to its nodes: the per-tree kernels around a
// build, the pools the builders of a device share, DeviceMinMatch and the rl_builder_* entry points.  The build is a request
// to the workers of minmatch_worker.hip: nothing here instantiates the build kernel, whose header lends its reductions.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <type_traits>
#include <vector>

#include "common.h"
#include "minmatch.h"
#include "minmatch_build.h"
#include "minmatch_worker.h"

namespace rl {

namespace {

// ---- the per-tree kernels around the build: every tree pays them on the CUs the workers leave, next to RePaint, so
// they are counted in bytes.  Round 5: four passes over the matrices instead of six --
//   rowmin_penalty_kernel  the carrier penalty of a tree's distance matrix (in place) AND its row minima, one pass;
//   prior_kernel           the clade prior row by row AND its row minima (the row is in LDS anyway);
//   weave_kernel           M[a][b] = (d(a,b), d(b,a), cf(a,b), cf(b,a)) AND the pair scan of the initialisation (the
//                          row minima are complete by then): every element of D / CF read once, M written once and
//                          never read back.
// Before: penalty (in place), prior, pack (read 2 x 2 matrices, write M), rowmin (read both matrices again), pairscan
// (read half of M): 0.42 ms of kernels and ~1.5 GB per tree at N = 5000; now ~1.1 GB.

// Carrier penalty of AncesTreeBuilder::BuildTopology (anc_builder.cpp:563-581): every entry of a carrier's row gets
// + val, and - val again where the column is a carrier too (the same two operations in the same order per entry as
// the host loop); member == nullptr: no penalty (the first tree of a section, --no_consistency).  And, of the row as
// it then is, out[a] = min over l != a: the row minima of tree_builder.cpp:1659-1666.  A workgroup per row.
__global__ void __launch_bounds__(256) rowmin_penalty_kernel(float *__restrict__ D, int N,
                                                            const unsigned char *__restrict__ member, float val,
                                                            float *__restrict__ out) {
  __shared__ float part[4];
  const int a = blockIdx.x;
  float *row = D + (size_t)a * N;
  const bool carrier = member && member[a];
  float mv = INFINITY;
  for (int col = threadIdx.x; col < N; col += 256) {
    float x = row[col];
    if (carrier) {
      x = x + val;
      if (member[col]) x -= val;
      row[col] = x;
    }
    if (col != a) mv = fminf(mv, x);
  }
  mv = wave_min_f(mv);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mv;
  __syncthreads();
  if (threadIdx.x == 0) out[a] = fminf(fminf(part[0], part[1]), fminf(part[2], part[3]));
}

// The woven matrix M[a][b] = (d(a,b), d(b,a), cf(a,b), cf(b,a)) from the row-major matrices (CF may be null) and, in
// the same pass, the pair scan of MinMatch's initialisation (tree_builder.cpp:1690-1722): row a's partners b > a
// with d(a,b) <= min_a and d(b,a) <= min_b (minima + threshold), in order, with the symmetric distance the
// reference's loop would compute for the pair (0 when the pair is also mutually closest under the prior,
// :1699-1702).  mvcf_old: min_values_CF as carried over from the previous tree (:2399-2400).
// One workgroup per strip of 32 rows, walking the column panels of 64 from its own on, in order (so a row's hits
// come out in order): wave w holds rows a0 + 8 w + r, lane l column 64 pb + l.  d(a,b) and cf(a,b) arrive as the lanes need
// them (a wave reads 256 contiguous bytes of a row), d(b,a) and cf(b,a) -- 64 rows b, 32 columns -- through LDS;
// a wave's store is 1 KB of M's panel.  The next panel's loads are in flight while this one is woven.
constexpr int WV_ROWS = 32;
// (Every strip walking ALL panels and weaving its own rows only -- each element read twice, no 512-byte runs -- was
//  within the noise of this in the C3 stage: removed, DESIGN_NOTES.md 11.)
template <bool PRIOR>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) weave_kernel(const float *__restrict__ D, const float *__restrict__ CF,
                                                    float4 *__restrict__ M, int N, const float *__restrict__ rowmin_D,
                                                    const float *__restrict__ rowmin_CF,
                                                    const float *__restrict__ mvcf_old, int ages, float threshold,
                                                    float threshold_CF, int *__restrict__ hit_cnt,
                                                    unsigned *__restrict__ hit_b, float *__restrict__ hit_sym) {
  __shared__ float tD[64][WV_ROWS + 1], tC[PRIOR ? 64 : 1][WV_ROWS + 1];  // [b][a]: d(b,a), cf(b,a)
  __shared__ float tX[WV_ROWS][64 + 1], tZ[PRIOR ? WV_ROWS : 1][64 + 1];   // [a][b]: d(a,b), cf(a,b)
  // (the wave's index as a scalar: its rows' addresses are scalar bases, the lane's column a 32-bit offset)
  const int a0 = blockIdx.x * WV_ROWS, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int trow = threadIdx.x >> 2, tcol = (threadIdx.x & 3) * 8;  // the thread's 8 floats of the transposed tile
  typedef const __attribute__((address_space(1))) float *GF;
  typedef const __attribute__((address_space(1))) f32x4 *GF4;
  const GF Dg = (GF)D, CFg = (GF)CF;
  const bool vec = (N & 3) == 0;                                     // (rows 16-byte aligned: float4 loads)
  float mva[8], mvcfa[8];
  int cnt[8];
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int a = a0 + wave * 8 + r;
    cnt[r] = 0;
    mva[r] = a < N ? rowmin_D[a] + threshold : 0.0f;
    mvcfa[r] = 0.0f;
    if (PRIOR && a < N) {
      const float old = mvcf_old[a], mc_ = rowmin_CF[a];
      mvcfa[r] = (old > mc_ ? mc_ : old) + threshold_CF;
    }
  }
  struct Panel {
    float x[8], z[8];    // d(a,b), cf(a,b) of the wave's rows at the lane's column
    float td[8], tc[8];  // the thread's piece of the transposed tile: d(b', a0 + tcol ..), cf likewise
  };
  auto load = [&](int pb, Panel &q) {
    const unsigned b = (unsigned)(pb * 64 + lane);
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int a = a0 + wave * 8 + r;  // (wave-uniform)
      const bool in = a < N && (int)b < N;
      const GF drow = Dg + (size_t)a * N, crow = CFg + (size_t)a * N;
      q.x[r] = in ? drow[b] : 0.0f;
      q.z[r] = (PRIOR && in) ? crow[b] : 0.0f;
    }
    const int bb = pb * 64 + trow;
    const unsigned toff = (unsigned)bb * (unsigned)N + (unsigned)(a0 + tcol);  // (N <= 10240: N * N < 2^32)
    if (vec && bb < N && a0 + tcol + 8 <= N) {
      const GF4 s4 = (GF4)(Dg + toff);
      const f32x4 u = s4[0], v = s4[1];
      q.td[0] = u.x, q.td[1] = u.y, q.td[2] = u.z, q.td[3] = u.w, q.td[4] = v.x, q.td[5] = v.y, q.td[6] = v.z, q.td[7] = v.w;
      if (PRIOR) {
        const GF4 c4 = (GF4)(CFg + toff);
        const f32x4 cu = c4[0], cv = c4[1];
        q.tc[0] = cu.x, q.tc[1] = cu.y, q.tc[2] = cu.z, q.tc[3] = cu.w, q.tc[4] = cv.x, q.tc[5] = cv.y, q.tc[6] = cv.z, q.tc[7] = cv.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const bool in = bb < N && a0 + tcol + k < N;
        q.td[k] = in ? Dg[toff + k] : 0.0f;
        q.tc[k] = (PRIOR && in) ? CFg[toff + k] : 0.0f;
      }
    }
  };
  // Every element of D and CF is read ONCE: the strip walks the panels from its own on (pa), and a tile right of
  // the diagonal panel is woven both ways -- M[a][b] for the strip's rows, a wave's store 1 KB of panel pb, and
  // M[b][a] = (d(b,a), d(a,b), cf(b,a), cf(a,b)) for the panel's 64 rows b at the strip's 32 columns, 512 B runs of
  // panel pa -- so nobody reads the tiles left of its diagonal.
  const int pa = a0 / 64;
  auto weave = [&](int pb, const Panel &q) {
    const bool both = pb > pa;  // (wave-uniform)
#pragma unroll
    for (int k = 0; k < 8; k++) {
      tD[trow][tcol + k] = q.td[k];
      if (PRIOR) tC[trow][tcol + k] = q.tc[k];
    }
    if (both) {
#pragma unroll
      for (int r = 0; r < 8; r++) {
        tX[wave * 8 + r][lane] = q.x[r];
        if (PRIOR) tZ[wave * 8 + r][lane] = q.z[r];
      }
    }
    __syncthreads();
    const int b = pb * 64 + lane;
    const float mvb = b < N ? rowmin_D[b] + threshold : 0.0f;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int a = a0 + wave * 8 + r;
      const float y = tD[lane][wave * 8 + r], w = PRIOR ? tC[lane][wave * 8 + r] : 0.0f;
      const bool in = a < N && b < N;
      if (in) M[mm_index(a, b, N)] = make_float4(q.x[r], y, q.z[r], w);
      const bool hit = in && b > a && mva[r] >= q.x[r] && mvb >= y;
      const unsigned long long m = __ballot(hit);
      if (m) {  // (wave-uniform, rare)
        const int at = cnt[r] + __popcll(m & ((1ull << lane) - 1ull));
        if (hit && at < MM_HITS) {
          float sym = y + q.x[r];
          if (PRIOR) {
            const float old = mvcf_old[b], mc_ = rowmin_CF[b];
            const float mvcf_b = (old > mc_ ? mc_ : old) + threshold_CF;
            // (with sample ages the initialisation keeps the pairs the prior agrees with and voids the others, :1792-1797)
            const bool agrees = q.z[r] <= mvcfa[r] && w <= mvcf_b;
            if (ages ? !agrees : agrees) sym = ages ? INFINITY : 0.0f;
          }
          hit_b[(size_t)a * MM_HITS + at] = (unsigned)b;
          hit_sym[(size_t)a * MM_HITS + at] = sym;
        }
        cnt[r] += __popcll(m);
      }
    }
    if (both) {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int bl = wave * 16 + 2 * k + (lane >> 5), al = lane & 31;
        const int bq = pb * 64 + bl, aq = a0 + al;
        if (aq < N && bq < N)
          M[mm_index(bq, aq, N)] = make_float4(tD[bl][al], tX[al][bl], PRIOR ? tC[bl][al] : 0.0f, PRIOR ? tZ[al][bl] : 0.0f);
      }
    }
    __syncthreads();
  };
  const int P = (N + 63) / 64;
  Panel p0, p1;
  load(pa, p0);
  for (int pb = pa; pb < P; pb += 2) {
    if (pb + 1 < P) load(pb + 1, p1);
    weave(pb, p0);
    if (pb + 1 < P) {
      if (pb + 2 < P) load(pb + 2, p0);
      weave(pb + 1, p1);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int a = a0 + wave * 8 + r;
      if (a < N) hit_cnt[a] = cnt[r];
    }
  }
}

// Clade prior from the previous tree (treeseq.cpp: clade_prior; anc_builder.cpp:583-606): row a holds, for
// every other leaf b, acc[depth(parent(a)) - depth(mrca(a,b))]; the leaves under the sibling of every ancestor
// step are a contiguous range of the depth-first leaf order.
__global__ void __launch_bounds__(256) prior_kernel(float *__restrict__ CF, int N, const int *__restrict__ parent,
                             const int *__restrict__ child_left, const int *__restrict__ child_right,
                             const int *__restrict__ depth, const int *__restrict__ lo,
                             const int *__restrict__ size, const int *__restrict__ order,
                             const float *__restrict__ acc, float *__restrict__ rowmin) {
  // The row is put together in LDS -- the ranges are contiguous in depth-first order, the entries they name are
  // scattered over the row (order[q]): as 4-byte stores to HBM the kernel wrote its 100 MB at 0.4 TB/s, 0.24 ms per
  // tree at N = 5000 and the largest of the per-tree kernels that share the chip with RePaint -- and leaves the block
  // in one coalesced pass.  (Every leaf but a itself lies under exactly one sibling on the way up: all of the row is
  // written.)
  extern __shared__ float prior_row[];  // N floats
  const int a = blockIdx.x;
  if (threadIdx.x == 0) prior_row[a] = 0.0f;
  const int da = depth[parent[a]];
  int child = a;
  for (int v = parent[a]; v >= 0; child = v, v = parent[v]) {
    const int other = child_left[v] == child ? child_right[v] : child_left[v];
    const float x = acc[da - depth[v]];
    const int b = lo[other], e = b + size[other];
    for (int q = b + threadIdx.x; q < e; q += blockDim.x) prior_row[order[q]] = x;
  }
  __syncthreads();
  float *__restrict__ row = CF + (size_t)a * N;
  float mv = INFINITY;  // the row's minimum off the diagonal (tree_builder.cpp:1659-1666), while the row is here
  for (int j = threadIdx.x; j < N; j += blockDim.x) {
    const float x = prior_row[j];
    row[j] = x;
    if (j != a) mv = fminf(mv, x);
  }
  __shared__ float part[4];
  mv = wave_min_f(mv);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mv;
  __syncthreads();
  if (threadIdx.x == 0) rowmin[a] = fminf(fminf(part[0], part[1]), fminf(part[2], part[3]));
}

}  // namespace

// What the builders of one device share.
//
// * Staging: the row-major distance matrix (K3 writes it, the carrier penalty edits it) and clade prior of a tree
//   are needed from K3 until the weave (weave_kernel) -- ~30 ms of a tree's ~0.2 s with a hundred sections sharing
//   the hardware queues: 32 pairs (12 were a queue of their own at 134 sections: 11 s of every section's 60).  A builder takes a pair from
//   a small pool for that time instead of owning 8 N^2 bytes for life (200 MB of the 725 MB a section used to pin
//   at N = 5000: why 91 sections were all that fitted).
// * The symmetric matrix of the fallback (tree_builder.cpp:255-293): a pool of `sym_slots` matrices the build
//   kernels take and give back themselves (MMParams::sym_locks).
constexpr int MM_STAGING = 32;  // staging pairs (row-major distance matrix + clade prior of a tree, K3 -> weave) per device
class DeviceShare {
 public:
  struct Staging {
    DevBuf D, CF;
  };
  static DeviceShare &of(int device) {
    static std::mutex gm;
    static std::vector<DeviceShare *> all;
    std::lock_guard<std::mutex> lk(gm);
    if ((int)all.size() <= device) all.resize(device + 1, nullptr);
    if (!all[device]) all[device] = new DeviceShare();  // lives as long as the process
    return *all[device];
  }
  // a staging pair with room for N x N floats each (blocks while all are out); nullptr: no memory
  Staging *take(int N) {
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      if (!free_.empty()) {
        Staging *s = free_.back();
        free_.pop_back();
        lk.unlock();
        if (s->D.alloc((size_t)N * N * 4) || s->CF.alloc((size_t)N * N * 4)) {
          give(s);
          return nullptr;
        }
        return s;
      }
      if (made_ < cap_) {
        made_++;
        lk.unlock();
        Staging *s = new Staging();
        if (s->D.alloc((size_t)N * N * 4) || s->CF.alloc((size_t)N * N * 4)) {
          delete s;
          lk.lock();
          made_--;
          if (made_ == 0) return nullptr;  // not even one: out of memory
          cap_ = made_;                    // what there is has to do
          continue;
        }
        return s;
      }
      cv_.wait(lk);
    }
  }
  void give(Staging *s) {
    {
      std::lock_guard<std::mutex> lk(m_);
      free_.push_back(s);
    }
    cv_.notify_one();
  }
  // a pair that is free or can still be made; nullptr rather than waiting
  Staging *take_if_any(int N) {
    {
      std::lock_guard<std::mutex> lk(m_);
      if (free_.empty() && made_ >= cap_) return nullptr;
    }
    return take(N);
  }
  // the pool of symmetric matrices for trees of N leaves (grown on demand, never shrunk); *slots = 0: none
  void sym_pool(int N, float **base, int **locks, int *slots) {
    std::lock_guard<std::mutex> lk(m_);
    if (sym_n_ < N) {
      int want = env_int("RELATE_AMD_TEST_SYM_SLOTS", 8, 0, 64);
      DevBuf nb, nl;
      while (want > 0 && nb.alloc((size_t)want * N * N * 4)) want /= 2;
      if (want > 0 && !nl.alloc(64 * 4) && hipMemset(nl.p, 0, 64 * 4) == hipSuccess) {
        // (builds in flight hold pointers into the old pool: it is kept, not freed)
        retired_.emplace_back(new DevBuf());
        retired_.back()->swap(sym_);
        retired_.emplace_back(new DevBuf());
        retired_.back()->swap(sym_locks_);
        sym_.swap(nb);
        sym_locks_.swap(nl);
        sym_n_ = N;
        sym_slots_ = want;
      }
    }
    *base = sym_n_ >= N ? sym_.as<float>() : nullptr;
    *locks = sym_locks_.as<int>();
    *slots = sym_n_ >= N ? sym_slots_ : 0;
  }
  // every staging pair and the symmetric pool now (the stage admits its sections against what is free after this)
  int prefill(int N) {
    std::vector<Staging *> got;
    for (int x = 0; x < cap_; x++) {
      Staging *s = take_if_any(N);
      if (!s) break;
      got.push_back(s);
    }
    const bool any = !got.empty();
    for (Staging *s : got) give(s);
    float *b;
    int *l, n;
    sym_pool(N, &b, &l, &n);
    return any ? 0 : -1;
  }
  // bytes of HBM the shared pools take for trees of N leaves (the stage's admission counts them once)
  static double bytes(int N) {
    return (double)MM_STAGING * 8.0 * N * N +
           (double)env_int("RELATE_AMD_TEST_SYM_SLOTS", 8, 0, 64) * 4.0 * N * N;
  }

 private:
  DeviceShare() : cap_(MM_STAGING) {}
  std::mutex m_;
  std::condition_variable cv_;
  std::vector<Staging *> free_;
  int made_ = 0, cap_;
  DevBuf sym_, sym_locks_;
  std::vector<std::unique_ptr<DevBuf>> retired_;
  int sym_n_ = 0, sym_slots_ = 0;
};
double device_builder_shared_bytes(int N) { return DeviceShare::bytes(N); }
int device_builder_reserve_shared(int device, int N) {
  if (hipSetDevice(device) != hipSuccess) return -1;
  return DeviceShare::of(device).prefill(N);
}

// the word of coherent pinned memory a worker tells its builder "this tree is out" in: taken from / given back to a
// list (give != nullptr), never freed
static int *done_word(int *give) {
  static std::mutex m;
  static std::vector<int *> spare;
  std::lock_guard<std::mutex> lk(m);
  if (give) {
    spare.push_back(give);
    return nullptr;
  }
  if (!spare.empty()) {
    int *w = spare.back();
    spare.pop_back();
    return w;
  }
  int *w = nullptr;
  return hipHostMalloc(reinterpret_cast<void **>(&w), 64, hipHostMallocCoherent) == hipSuccess ? w : nullptr;
}

// The blocks of memory a builder carves up, stated once: the size of each and where every array of it begins.  A block is
// "slots" of N elements side by side (what the arrays hold: MM_PARAM_FIELDS); reserve(), the passes before a build and
// build_impl address the blocks through this and nothing else -- a resident worker writes wherever these offsets send it.
struct BuilderLayout {
  const size_t N, T;  // leaves and nodes of a tree
  explicit BuilderLayout(int n) : N((size_t)n), T(2 * (size_t)n - 1) {}
  enum { F_MIN_VALUES, F_MIN_VALUES_CF, F_MC_DIST, F_MC_DIST2, F_MIN_VALUES_SYM, F_MCS_DIST, F_ROWMIN_D, F_ROWMIN_CF, F_SLOTS };
  size_t f_bytes() const { return F_SLOTS * N * 4; }  // d_f, floats
  float *f(const DevBuf &d_f, int slot) const { return d_f.as<float>() + slot * N; }
  // d_i, ints; mc_lin1 / mc_lin2 and merge_i / merge_j are copied as pairs: neighbours.  8 ints lie behind the slots.
  enum { I_MC_LIN1, I_MC_LIN2, I_CLUSTER_INDEX, I_CLUSTER_SIZE, I_UNUSED_4, I_UPD_POS, I_MCS_LIN1, I_MCS_LIN2, I_MERGE_I,
         I_MERGE_J, I_UNUSED_10, I_UNUSED_11, I_UPD_G, I_UPDV_G, I_SLOTS };
  size_t i_bytes() const { return (I_SLOTS * N + 8) * 4; }
  int *i(const DevBuf &d_i, int slot) const { return d_i.as<int>() + slot * N; }
  // d_ages (the AGES build): slots of doubles, then slots of ints.  bucket and bucket_off hold N + 1 entries: bucket_off
  // begins 8 ints behind its slot, and 16 ints lie behind the slots.
  enum { AD_MC_DIST2D, AD_UNIQUE_AGES, AD_SLOTS };
  enum { AI_MC_LVL, AI_AGE_LVL, AI_AGE_LVL0, AI_AGES_COUNT, AI_UPD_G, AI_UPDV_G, AI_BUCKET, AI_BUCKET_OFF, AI_SLOTS };
  size_t ages_bytes() const { return AD_SLOTS * N * 8 + (AI_SLOTS * N + 16) * 4; }
  double *ages_d(const DevBuf &d_ages, int slot) const { return d_ages.as<double>() + slot * N; }
  int *ages_i(const DevBuf &a, int slot) const { return (int *)ages_d(a, AD_SLOTS) + slot * N + (slot == AI_BUCKET_OFF ? 8 : 0); }
  // d_hits: the pairs of weave_kernel's scan -- hit_cnt [N], then hit_b and hit_sym [N][MM_HITS]
  size_t hits_bytes() const { return (N + 2 * N * MM_HITS) * 4; }
  int *hit_cnt(const DevBuf &d_hits) const { return d_hits.as<int>(); }
  unsigned *hit_b(const DevBuf &d_hits) const { return d_hits.as<unsigned>() + N; }
  float *hit_sym(const DevBuf &d_hits) const { return d_hits.as<float>() + N + N * MM_HITS; }
  // h_io (pinned), ints: carried state in and out, merges out (pairs, neighbours as in d_i); then 16 timers, 8-byte aligned
  enum { IO_LIN1, IO_LIN2, IO_MVCF, IO_MERGE_I, IO_MERGE_J, IO_SLOTS };
  size_t io_bytes() const { return IO_SLOTS * N * 4 + 16 * 8 + 8; }
  int *io(int *h_io, int slot) const { return h_io + slot * N; }
  long long *io_timers(int *h_io) const { return (long long *)(((uintptr_t)io(h_io, IO_SLOTS) + 7) & ~(uintptr_t)7); }
  // h_tab (pinned) and d_tab, ints: the last tree's tables for prior_kernel, T each, its leaf order, N; h_tab: + N flag bytes
  enum { TAB_PARENT, TAB_LEFT, TAB_RIGHT, TAB_DEPTH, TAB_LO, TAB_SIZE, TAB_ORDER };
  size_t tab_ints() const { return TAB_ORDER * T + N; }
  size_t h_tab_bytes() const { return tab_ints() * 4 + N; }
  int *tab(int *base, int which) const { return base + which * T; }
  char *tab_flags(int *h_tab) const { return reinterpret_cast<char *>(h_tab + tab_ints()); }
  // d_feas: feasible pairs of a merge beyond MM_PAIRS_LDS, 6 words each (with sample ages a merge of the lineage the last
  // tree's candidates were renamed to sends most clusters through the rebuilding branch: every feasible pair again)
  static long long pair_cap(int N, bool ages) { return (long long)(ages ? 32 : 8) * N; }
};

struct DeviceMinMatch::Impl {
  int N = 0, device = 0;
  hipStream_t stream = nullptr;
  DeviceShare::Staging *staging = nullptr;  // held from device_matrix() / the upload until the matrices are woven
  DevBuf d_M, d_hits, d_f, d_i, d_feas, d_rowlist, d_status, d_flags, d_member, d_tab, d_acc;
  DevBuf d_ages;  // --sample_ages: the third key and the draw of the candidates, the clusters' age levels, the table
  bool ages_up = false;  // ... whose constant part is in place
  long long builds = 0, n_built = 0;
  double t_prep = 0, t_wait = 0, t_out = 0;  // RELATE_AMD_TIMING: uploads + weave, submit -> tree done, copy-out (s)
  long long n_timed = 0;
  int *h_done = nullptr;  // pinned: the worker's "this tree is out"
  // pinned: what goes in and comes out per tree (candidate indices 2N, min_values_CF N, the merges 2N) -- from
  // pageable memory every one of these small copies is staged and synchronised by the runtime, milliseconds each
  // with a hundred sections copying at once
  int *h_io = nullptr;
  size_t h_io_bytes = 0, h_tab_bytes = 0;
  int *h_tab = nullptr;   // pinned: the previous tree's tables for prior_kernel (6T + N ints), then N carrier flags
  float acc_val = 0.0f;   // d_acc holds acc[c] = val added c times for this val
  bool acc_valid = false;
  bool abandoned = false;  // a tree was given up while its ticket may be live: nothing of this builder is recycled
  // the row minima of the staged matrices are in d_f already (apply_penalty / apply_prior took them in their pass)
  bool rowmin_d_ready = false, rowmin_cf_ready = false;
  void drop_staging() {
    if (staging) DeviceShare::of(device).give(staging);
    staging = nullptr;
    rowmin_d_ready = rowmin_cf_ready = false;
  }
  hipError_t ensure_stream() { return stream ? hipSuccess : make_stream(&stream, false, true); }
  // h_tab, allocated at its first use, and in *flags its carrier flag bytes; nullptr: no pinned host memory for `what`
  int *tables(const char *what, char **flags = nullptr) {
    const BuilderLayout lay(N);
    if (!h_tab) h_tab = static_cast<int *>(pinned_cache_alloc(lay.h_tab_bytes(), &h_tab_bytes));
    if (!h_tab) set_error("tree builder: no pinned host memory for the %s", what);
    if (h_tab && flags) *flags = lay.tab_flags(h_tab);
    return h_tab;
  }
};

DeviceMinMatch::DeviceMinMatch(int N, int device) : impl(new Impl()) {
  impl->N = N;
  impl->device = device;
}
DeviceMinMatch::~DeviceMinMatch() {
  impl->drop_staging();
  if (getenv("RELATE_AMD_TIMING") && impl->n_timed)
    fprintf(stderr, "[gpu tree builder] %lld trees, host ms per tree: uploads + weave %.2f, submit -> done %.2f, "
                    "copy-out %.2f\n", impl->n_timed, 1e3 * impl->t_prep / impl->n_timed,
            1e3 * impl->t_wait / impl->n_timed, 1e3 * impl->t_out / impl->n_timed);
  if (impl->abandoned) {
    // (leaked on purpose: handed to the caches these blocks would be given out again at once, and a worker that
    //  claims or finishes the abandoned ticket later would write into somebody else's tree)
    for (DevBuf *b : {&impl->d_M, &impl->d_hits, &impl->d_f, &impl->d_i, &impl->d_feas, &impl->d_rowlist, &impl->d_status,
                      &impl->d_flags, &impl->d_member, &impl->d_tab, &impl->d_acc, &impl->d_ages}) {
      b->p = nullptr;
      b->bytes = 0;
    }
    impl->staging = nullptr;
    delete impl;
    return;
  }
  if (impl->stream) (void)hipStreamDestroy(impl->stream);
  // (nothing goes back to the driver here: hipFree / hipHostFree would wait for the workers of the other builders)
  if (impl->h_done) done_word(impl->h_done);
  if (impl->h_io) pinned_cache_release(impl->h_io, impl->h_io_bytes);
  if (impl->h_tab) pinned_cache_release(impl->h_tab, impl->h_tab_bytes);
  delete impl;
}

void DeviceMinMatch::forget_ages() { impl->ages_up = false; }

float *DeviceMinMatch::device_matrix() {
  Impl &m = *impl;
  if (hipSetDevice(m.device) != hipSuccess) return nullptr;
  if (!m.staging) m.staging = DeviceShare::of(m.device).take(m.N);
  return m.staging ? m.staging->D.as<float>() : nullptr;
}

int DeviceMinMatch::stage_from_device(const float *dD, const float *dCF) {
  Impl &m = *impl;
  RL_HIP(hipSetDevice(m.device));
  RL_HIP(m.ensure_stream());
  if (!m.staging) m.staging = DeviceShare::of(m.device).take(m.N);
  if (!m.staging) return -1;
  const size_t bytes = (size_t)m.N * m.N * 4;
  RL_HIP(hipMemcpyAsync(m.staging->D.p, dD, bytes, hipMemcpyDeviceToDevice, m.stream));
  if (dCF) RL_HIP(hipMemcpyAsync(m.staging->CF.p, dCF, bytes, hipMemcpyDeviceToDevice, m.stream));
  m.rowmin_d_ready = m.rowmin_cf_ready = false;
  return 0;
}

float *DeviceMinMatch::rowmin_device() {
  Impl &m = *impl;
  const BuilderLayout lay(m.N);
  if (hipSetDevice(m.device) != hipSuccess || m.d_f.alloc(lay.f_bytes())) return nullptr;
  return lay.f(m.d_f, lay.F_ROWMIN_D);
}
void DeviceMinMatch::rowmin_is_ready() { impl->rowmin_d_ready = true; }

int DeviceMinMatch::apply_penalty(const char *member, float val) {
  Impl &m = *impl;
  const int N = m.N;
  const BuilderLayout lay(N);
  if (!m.staging) return -1;
  RL_HIP(hipSetDevice(m.device));
  RL_HIP(m.ensure_stream());
  char *flags;
  if (m.d_member.alloc((size_t)N) || !m.tables("carrier flags", &flags)) return -1;
  memcpy(flags, member, (size_t)N);
  if (m.d_f.alloc(lay.f_bytes())) return -1;  // (reserve()'s)
  RL_HIP(hipMemcpyAsync(m.d_member.p, flags, (size_t)N, hipMemcpyHostToDevice, m.stream));
  // the penalty and, of the rows as they then are, the row minima of the build: one pass over the matrix
  hipLaunchKernelGGL(rowmin_penalty_kernel, dim3(N), dim3(256), 0, m.stream, m.staging->D.as<float>(), N,
                     m.d_member.as<unsigned char>(), val, lay.f(m.d_f, lay.F_ROWMIN_D));
  RL_HIP(hipGetLastError());
  m.rowmin_d_ready = true;
  return 0;
}

hipError_t launch_cancel_rowmin(float *D, int N, const unsigned char *member, float log_ratio, float *rowmin,
                                hipStream_t stream);  // (optimize_kernels.hip)

int DeviceMinMatch::apply_cancel(const char *member, float log_ratio) {
  Impl &m = *impl;
  const int N = m.N;
  const BuilderLayout lay(N);
  if (!m.staging) return -1;
  RL_HIP(hipSetDevice(m.device));
  RL_HIP(m.ensure_stream());
  char *flags;  // (the block apply_penalty keeps its flags in)
  if (m.d_member.alloc((size_t)N) || !m.tables("carrier flags", &flags)) return -1;
  for (int i = 0; i < N; i++) flags[i] = member[i] ? 1 : 0;
  if (m.d_f.alloc(lay.f_bytes())) return -1;  // (reserve()'s)
  RL_HIP(hipMemcpyAsync(m.d_member.p, flags, (size_t)N, hipMemcpyHostToDevice, m.stream));
  RL_HIP(launch_cancel_rowmin(m.staging->D.as<float>(), N, m.d_member.as<unsigned char>(), log_ratio,
                              lay.f(m.d_f, lay.F_ROWMIN_D), m.stream));
  m.rowmin_d_ready = true;
  return 0;
}

int DeviceMinMatch::apply_prior(const HostTree &t, float val) {
  Impl &m = *impl;
  const int N = m.N, T = 2 * N - 1;
  const BuilderLayout lay(N);
  if (!m.staging) return -1;
  RL_HIP(hipSetDevice(m.device));
  RL_HIP(m.ensure_stream());
  // the same tables as the host's clade_prior (treeseq.cpp), in pinned memory: nothing here waits for the copy
  // (the next tree of this builder -- the next writer of the block -- comes after this one is built)
  int *h = m.tables("prior's tables");
  if (!h) return -1;
  std::copy_n(t.parent.begin(), T, lay.tab(h, lay.TAB_PARENT));
  std::copy_n(t.child_left.begin(), T, lay.tab(h, lay.TAB_LEFT));
  std::copy_n(t.child_right.begin(), T, lay.tab(h, lay.TAB_RIGHT));
  clade_tables(t, N, lay.tab(h, lay.TAB_DEPTH), lay.tab(h, lay.TAB_SIZE), lay.tab(h, lay.TAB_LO), lay.tab(h, lay.TAB_ORDER));
  int rc = m.d_tab.alloc(lay.tab_ints() * 4);
  rc = rc ? rc : m.d_acc.alloc(((size_t)N + 1) * 4);
  rc = rc ? rc : m.d_f.alloc(lay.f_bytes());  // (reserve()'s)
  if (rc) return -1;
  if (!m.acc_valid || m.acc_val != val) {  // (one val per section: once)
    std::vector<float> acc((size_t)N + 1, 0.0f);
    for (int c = 1; c <= N; c++) acc[c] = acc[c - 1] + val;
    RL_HIP(hipMemcpy(m.d_acc.p, acc.data(), acc.size() * 4, hipMemcpyHostToDevice));
    m.acc_val = val;
    m.acc_valid = true;
  }
  RL_HIP(hipMemcpyAsync(m.d_tab.p, h, lay.tab_ints() * 4, hipMemcpyHostToDevice, m.stream));
  int *q = m.d_tab.as<int>();
  hipLaunchKernelGGL(prior_kernel, dim3(N), dim3(256), (size_t)N * sizeof(float), m.stream, m.staging->CF.as<float>(), N,
                     lay.tab(q, lay.TAB_PARENT), lay.tab(q, lay.TAB_LEFT), lay.tab(q, lay.TAB_RIGHT), lay.tab(q, lay.TAB_DEPTH),
                     lay.tab(q, lay.TAB_LO), lay.tab(q, lay.TAB_SIZE), lay.tab(q, lay.TAB_ORDER), m.d_acc.as<float>(),
                     lay.f(m.d_f, lay.F_ROWMIN_CF));
  RL_HIP(hipGetLastError());
  m.rowmin_cf_ready = true;
  return 0;
}

int DeviceMinMatch::reserve(bool ages) {
  Impl &m = *impl;
  const int N = m.N;
  if (hipSetDevice(m.device) != hipSuccess) return -1;
  const BuilderLayout lay(N);
  int rc = m.d_M.alloc(mm_elements(N) * 16);
  rc = rc ? rc : m.d_hits.alloc(lay.hits_bytes());
  rc = rc ? rc : m.d_f.alloc(lay.f_bytes());
  rc = rc ? rc : m.d_i.alloc(lay.i_bytes());
  rc = rc ? rc : m.d_feas.alloc((size_t)lay.pair_cap(N, ages) * 6 * 4);
  rc = rc ? rc : m.d_rowlist.alloc((size_t)MM_WAVES * N * 4);
  rc = rc ? rc : m.d_status.alloc(16 + 16 * 8);
  rc = rc ? rc : m.d_flags.alloc((size_t)N);
  return rc ? -1 : 0;
}

int DeviceMinMatch::build_resident(MinMatch &tb, bool with_prior, HostTree &tree) {
  return build_impl(tb, nullptr, nullptr, nullptr, true, with_prior, tree);
}

int DeviceMinMatch::build(MinMatch &tb, const float *d, const float *prior, HostTree &tree) {
  return build_impl(tb, nullptr, d, prior, false, prior != nullptr, tree);
}

int DeviceMinMatch::build_resident(MinMatchAges &tb, const std::vector<double> &sample_ages, bool with_prior, HostTree &tree) {
  return build_impl(tb, &sample_ages, nullptr, nullptr, true, with_prior, tree);
}

int DeviceMinMatch::build(MinMatchAges &tb, const std::vector<double> &sample_ages, const float *d, const float *prior,
                          HostTree &tree) {
  return build_impl(tb, &sample_ages, d, prior, false, prior != nullptr, tree);
}

template <class TB>
int DeviceMinMatch::build_impl(TB &tb, const std::vector<double> *sample_ages, const float *d, const float *prior_host,
                               bool resident, bool with_prior, HostTree &tree) {
  Impl &m = *impl;
  const int N = m.N;
  struct Drop { Impl &m; ~Drop() { m.drop_staging(); } } drop{m};  // however the build ends, the staging pair goes back
  constexpr bool ages = std::is_same<TB, MinMatchAges>::value;
  if (ages && (!sample_ages || (int)sample_ages->size() != N)) {
    set_error("tree builder: one sample age per haplotype");
    return -1;
  }
  if (N < 2 || N > MM_MAXN) return 1;  // (the painting kernels stop at N = 10240 too)
  if (resident) {  // tests: every k-th resident build is handed to the host, as a tree with too many tied candidates is
    static const int every = getenv("RELATE_AMD_TEST_HANDOVER_EVERY") ? atoi(getenv("RELATE_AMD_TEST_HANDOVER_EVERY")) : 0;
    if (every > 0 && ++m.builds % every == 0) return 2;
  }
  RL_HIP(hipSetDevice(m.device));
  RL_HIP(m.ensure_stream());
  BuildQueue *queue = build_queue_of(m.device, N, ages);
  if (!queue) {
    set_error("tree builder: no queue on device %d (pinned host memory)", m.device);
    return -1;
  }
  if (!m.staging) {
    if (resident) {
      set_error("tree builder: build_resident without device_matrix()");
      return -1;
    }
    m.staging = DeviceShare::of(m.device).take(N);
    if (!m.staging) return -1;
  }
  const bool prior = with_prior;
  const size_t NN = (size_t)N * N;
  const auto tb0 = std::chrono::steady_clock::now();
  if (reserve(ages)) return -1;
  const BuilderLayout lay(N);
  MMParams p;
  memset(&p, 0, sizeof(p));
  p.N = N;
  p.layout = worker_layout(N, ages);
  p.threshold = tb.threshold;
  p.threshold_CF = tb.threshold_CF;
  p.M = m.d_M.as<float4>();
  p.has_prior = prior ? 1 : 0;
  p.rowmin_D = lay.f(m.d_f, lay.F_ROWMIN_D);
  p.rowmin_CF = lay.f(m.d_f, lay.F_ROWMIN_CF);
  p.hit_cnt = lay.hit_cnt(m.d_hits);
  p.hit_b = lay.hit_b(m.d_hits);
  p.hit_sym = lay.hit_sym(m.d_hits);
  p.min_values = lay.f(m.d_f, lay.F_MIN_VALUES);
  p.min_values_CF = lay.f(m.d_f, lay.F_MIN_VALUES_CF);
  p.mc_dist = lay.f(m.d_f, lay.F_MC_DIST);
  p.mc_dist2 = lay.f(m.d_f, lay.F_MC_DIST2);
  p.min_values_sym = lay.f(m.d_f, lay.F_MIN_VALUES_SYM);
  p.mcs_dist = lay.f(m.d_f, lay.F_MCS_DIST);
  DeviceShare::of(m.device).sym_pool(N, &p.SYM, &p.sym_locks, &p.sym_slots);
  p.mc_lin1 = lay.i(m.d_i, lay.I_MC_LIN1);
  p.mc_lin2 = lay.i(m.d_i, lay.I_MC_LIN2);
  p.cluster_index = lay.i(m.d_i, lay.I_CLUSTER_INDEX);
  p.cluster_size = lay.i(m.d_i, lay.I_CLUSTER_SIZE);
  p.upd_pos = lay.i(m.d_i, lay.I_UPD_POS);
  p.mcs_lin1 = lay.i(m.d_i, lay.I_MCS_LIN1);
  p.mcs_lin2 = lay.i(m.d_i, lay.I_MCS_LIN2);
  p.merge_i = lay.i(m.d_i, lay.I_MERGE_I);  // [N-1]
  p.merge_j = lay.i(m.d_i, lay.I_MERGE_J);  // [N-1]
  p.upd_g = reinterpret_cast<unsigned *>(lay.i(m.d_i, lay.I_UPD_G));  // (the AGES build: a list of its own, below)
  p.updv_g = reinterpret_cast<float *>(lay.i(m.d_i, lay.I_UPDV_G));
  p.kflag = m.d_flags.as<unsigned char>();
  p.pair_g = m.d_feas.as<unsigned>();
  p.pair_cap = lay.pair_cap(N, ages);
  p.rowlist = m.d_rowlist.as<int>();
  p.status = m.d_status.as<int>();
  if (!m.h_done && !(m.h_done = done_word(nullptr))) {
    set_error("tree builder: no pinned host memory for the completion word");
    return -1;
  }
  p.host_done = m.h_done;
  if constexpr (ages) {
    // the age levels: a candidate's third key is the index of an age in the sorted table of the distinct sample ages
    // (tree_builder.cpp:1125-1152)
    tb.prepare_levels(*sample_ages);
    const std::vector<double> *unique = &tb.unique_ages;
    const std::vector<int> *count = &tb.ages_count;
    p.Ne = tb.Ne;
    const int nlev = (int)unique->size();
    if (m.d_ages.alloc(lay.ages_bytes())) return -1;
    p.mc_dist2d = lay.ages_d(m.d_ages, lay.AD_MC_DIST2D);
    p.unique_ages = lay.ages_d(m.d_ages, lay.AD_UNIQUE_AGES);
    p.mc_lvl = lay.ages_i(m.d_ages, lay.AI_MC_LVL);
    p.age_lvl = lay.ages_i(m.d_ages, lay.AI_AGE_LVL);
    p.age_lvl0 = lay.ages_i(m.d_ages, lay.AI_AGE_LVL0);
    p.ages_count = lay.ages_i(m.d_ages, lay.AI_AGES_COUNT);
    p.upd_g = reinterpret_cast<unsigned *>(lay.ages_i(m.d_ages, lay.AI_UPD_G));
    p.updv_g = reinterpret_cast<float *>(lay.ages_i(m.d_ages, lay.AI_UPDV_G));
    p.bucket = lay.ages_i(m.d_ages, lay.AI_BUCKET);
    p.bucket_off = lay.ages_i(m.d_ages, lay.AI_BUCKET_OFF);
    p.n_levels = nlev;
    if (!m.ages_up) {  // (one set of ages per builder)
      std::vector<int> lvl0((size_t)N);
      for (int c = 0; c < N; c++)
        lvl0[c] = (int)(std::lower_bound(unique->begin(), unique->end(), (*sample_ages)[c]) - unique->begin());
      RL_HIP(hipMemcpy(lay.ages_d(m.d_ages, lay.AD_UNIQUE_AGES), unique->data(), (size_t)nlev * 8, hipMemcpyHostToDevice));
      RL_HIP(hipMemcpy(lay.ages_i(m.d_ages, lay.AI_AGE_LVL0), lvl0.data(), (size_t)N * 4, hipMemcpyHostToDevice));
      RL_HIP(hipMemcpy(lay.ages_i(m.d_ages, lay.AI_AGES_COUNT), count->data(), (size_t)nlev * 4, hipMemcpyHostToDevice));
      m.ages_up = true;
    }
  }
  const bool timing = getenv("RELATE_AMD_TIMING") != nullptr;
  p.timers = nullptr;  // (set below: a corner of the pinned block, read when the tree is out -- no copy)

  // state the builders carry from tree to tree: in
  if (!m.h_io && !(m.h_io = static_cast<int *>(pinned_cache_alloc(lay.io_bytes(), &m.h_io_bytes)))) {
    set_error("tree builder: no pinned host memory for the per-tree copies");
    return -1;
  }
  int *lin1 = lay.io(m.h_io, lay.IO_LIN1), *lin2 = lay.io(m.h_io, lay.IO_LIN2);
  int *merge_i = lay.io(m.h_io, lay.IO_MERGE_I), *merge_j = lay.io(m.h_io, lay.IO_MERGE_J);
  long long *h_timers = lay.io_timers(m.h_io);
  if (timing) p.timers = h_timers;
  float *mvcf = reinterpret_cast<float *>(lay.io(m.h_io, lay.IO_MVCF));
  for (int c = 0; c < N; c++) {
    lin1[c] = tb.mc[c].lin1;
    lin2[c] = tb.mc[c].lin2;
    mvcf[c] = tb.min_values_CF[c];
  }
  // (min_values_CF as carried over is also what weave_kernel tests the prior with: that copy goes to the device)
  const float *mvcf_dev = p.min_values_CF;
  RL_HIP(hipMemcpyAsync(p.min_values_CF, mvcf, (size_t)N * 4, hipMemcpyHostToDevice, m.stream));
  if (p.layout != L_GLOBAL) {
    // The worker reads the carried state from the pinned block and leaves it there again together with the merges:
    // 100 KB across PCIe per tree instead of three copies and a stream synchronisation behind the build (16 ms per
    // tree with a hundred sections sharing the hardware queues).  The system-scope fences around a tree in the worker
    // order them with the request and with "done".
    p.io_lin = lin1;
    p.io_mvcf = mvcf;
    p.merge_i = merge_i;
    p.merge_j = merge_j;
  } else {  // (the state lives in these arrays throughout the build: device memory)
    RL_HIP(hipMemcpyAsync(p.mc_lin1, lin1, (size_t)2 * N * 4, hipMemcpyHostToDevice, m.stream));
  }
  float *dD = m.staging->D.as<float>(), *dCF = prior ? m.staging->CF.as<float>() : nullptr;
  if (!resident) {
    RL_HIP(hipMemcpyAsync(dD, d, NN * 4, hipMemcpyHostToDevice, m.stream));
    if (prior) RL_HIP(hipMemcpyAsync(dCF, prior_host, NN * 4, hipMemcpyHostToDevice, m.stream));
  }
  {
    // the row minima (where the penalty / prior passes have not left them already), then the woven matrix and the
    // pair scan of the initialisation in one pass, on the whole chip; the build itself is one workgroup
    if (!m.rowmin_d_ready)
      hipLaunchKernelGGL(rowmin_penalty_kernel, dim3(N), dim3(256), 0, m.stream, dD, N, (const unsigned char *)nullptr, 0.0f,
                         lay.f(m.d_f, lay.F_ROWMIN_D));
    if (prior && !m.rowmin_cf_ready)
      hipLaunchKernelGGL(rowmin_penalty_kernel, dim3(N), dim3(256), 0, m.stream, dCF, N, (const unsigned char *)nullptr, 0.0f,
                         lay.f(m.d_f, lay.F_ROWMIN_CF));
    const dim3 grid((N + WV_ROWS - 1) / WV_ROWS);
    const auto weave = prior ? weave_kernel<true> : weave_kernel<false>;
    hipLaunchKernelGGL(weave, grid, dim3(256), 0, m.stream, dD, dCF, p.M, N, p.rowmin_D, p.rowmin_CF, mvcf_dev, ages ? 1 : 0,
                       p.threshold, p.threshold_CF, lay.hit_cnt(m.d_hits), lay.hit_b(m.d_hits), lay.hit_sym(m.d_hits));
    RL_HIP(hipGetLastError());
  }
  static const bool trace = (timing_level() >= 2);
  if (trace) fprintf(stderr, "[mm trace] N=%d inputs submitted\n", N), fflush(stderr);
  RL_HIP(hipStreamSynchronize(m.stream));  // inputs in place
  if (trace) fprintf(stderr, "[mm trace] N=%d inputs in place\n", N), fflush(stderr);
  if (const char *dump = getenv("RELATE_AMD_TEST_MM_DUMP")) {
    // (tools/bench_builder_variants.py) the matrices of builds first..last of this builder, as the kernel gets them:
    // "<dir>:<first>:<last>"; the process ends behind the last one
    char dir[512];
    int first = 0, last = 0;
    if (sscanf(dump, "%511[^:]:%d:%d", dir, &first, &last) == 3 && m.n_built >= first && m.n_built <= last) {
      std::vector<float> host(NN);
      for (int which = 0; which < (prior ? 2 : 1); which++) {
        RL_HIP(hipMemcpy(host.data(), which ? (const void *)dCF : (const void *)dD, NN * 4, hipMemcpyDeviceToHost));
        const std::string fn = std::string(dir) + (which ? "/cf_" : "/d_") + std::to_string(m.n_built) + ".bin";
        FILE *fp = fopen(fn.c_str(), "wb");
        if (fp) {
          fwrite(host.data(), 4, NN, fp);
          fclose(fp);
        }
      }
      if (m.n_built == last) _exit(0);
    }
  }
  m.n_built++;
  m.drop_staging();                        // (woven: the row-major matrices go back to the pool)
  const auto tb1 = std::chrono::steady_clock::now();
  __atomic_store_n(m.h_done, -1, __ATOMIC_RELEASE);
  if (build_queue_run(queue, p)) {
    set_error("tree builder: the workers of device %d failed", m.device);
    m.abandoned = true;  // a worker may still write this tree's state, merges and completion word
    return -1;
  }
  const auto tb2 = std::chrono::steady_clock::now();
  // (the worker stores the code where it stores "done", behind a system-scope fence: no copy of p.status, which
  //  could still sit in the worker's L2 for a copy engine)
  const int status = __atomic_load_n(m.h_done, __ATOMIC_ACQUIRE);
  if (trace) fprintf(stderr, "[mm trace] N=%d tree out, status %d\n", N, status), fflush(stderr);
  if (status != 0) return status > 0 ? status : -1;
  if (timing) {
    const long long *tk = h_timers;
    fprintf(stderr, "[gpu tree builder] N=%d, us:", N);
    static const char *names[16] = {"row minima", "pair scan", "updates", "rescans", "pair tests", "pair order",
                                    "ordered", "symmetric", "erase", "pairs_x100", "before_draws", "", "rebuilt_x100",
                                    "rescan_only_x100", "merges_none_rebuilt_x100", "merges_with_rescan_only_x100"};
    for (int x = 0; x < 16; x++)
      if (x != 11) fprintf(stderr, " %s %.0f", names[x], tk[x] / 100.0);
    fprintf(stderr, " shader_MHz %lld\n", tk[11]);
  }
  // out: the tree and the carried state
  // (merge_i [N), merge_j [N) lie back to back)
  if (p.layout == L_GLOBAL) {
    RL_HIP(hipMemcpyAsync(merge_i, p.merge_i, ((size_t)2 * N - 1) * 4, hipMemcpyDeviceToHost, m.stream));
    RL_HIP(hipMemcpyAsync(lin1, p.mc_lin1, (size_t)2 * N * 4, hipMemcpyDeviceToHost, m.stream));
    RL_HIP(hipMemcpyAsync(mvcf, p.min_values_CF, (size_t)N * 4, hipMemcpyDeviceToHost, m.stream));
    RL_HIP(hipStreamSynchronize(m.stream));
  }
  for (int c = 0; c < N; c++) tb.min_values_CF[c] = mvcf[c];
  if (const int bad = tree_from_merges(tree, N, merge_i, merge_j); bad >= 0) {
    set_error("tree builder on the device: merge %d names clusters %d and %d", bad, merge_i[bad], merge_j[bad]);
    return -1;
  }
  for (int c = 0; c < N; c++) {
    tb.mc[c].lin1 = lin1[c];
    tb.mc[c].lin2 = lin2[c];
  }
  {
    const auto tb3 = std::chrono::steady_clock::now();
    m.t_prep += std::chrono::duration<double>(tb1 - tb0).count();
    m.t_wait += std::chrono::duration<double>(tb2 - tb1).count();
    m.t_out += std::chrono::duration<double>(tb3 - tb2).count();
    m.n_timed++;
  }
  return 0;
}

}  // namespace rl

// ---- C ABI: a tree builder that keeps MinMatch's state from tree to tree
struct rl_builder {
  int N;
  double theta;
  rl::MinMatch tb;
  rl::DeviceMinMatch *dev;
  rl::MinMatchAges *ages_tb = nullptr;  // rl_builder_set_sample_ages: the builder with the third key and the clock
  std::vector<double> ages;
  int last_on_gpu;
  rl_builder(int n, double th, int device)
      : N(n), theta(th), tb(n, th), dev(device >= 0 ? new rl::DeviceMinMatch(n, device) : nullptr), last_on_gpu(0) {}
  ~rl_builder() {
    delete dev;
    delete ages_tb;
  }
};

extern "C" {

rl_builder *rl_builder_create(int N, double theta, int device) {
  if (N < 2 || !(theta > 0.0 && theta < 1.0)) {
    rl::set_error("rl_builder_create: bad arguments");
    return nullptr;
  }
  return new rl_builder(N, theta, device);
}

void rl_builder_destroy(rl_builder *b) { delete b; }

int rl_builder_build(rl_builder *b, float *d, const float *d_prior, int *parent, int *child_left, int *child_right) {
  if (!b || !d || !parent) {
    rl::set_error("rl_builder_build: bad arguments");
    return RL_EINVAL;
  }
  rl::HostTree t;
  int st = 1;
  if (b->dev) {
    st = b->ages_tb ? b->dev->build(*b->ages_tb, b->ages, d, d_prior, t) : b->dev->build(b->tb, d, d_prior, t);
    if (st < 0) return RL_EHIP;
  }
  b->last_on_gpu = st == 0;
  if (st != 0) {
    if (b->ages_tb) b->ages_tb->quick_build(d, d_prior, b->ages, t);
    else b->tb.quick_build(d, d_prior, t);
  }
  const int N = b->N;
  for (int i = 0; i < 2 * N - 1; i++) parent[i] = t.parent[i];
  for (int i = N; i < 2 * N - 1; i++) {
    if (child_left) child_left[i - N] = t.child_left[i];
    if (child_right) child_right[i - N] = t.child_right[i];
  }
  return RL_OK;
}

int rl_builder_set_sample_ages(rl_builder *b, const double *ages, int n) {
  if (!b || n != b->N || !ages) {
    rl::set_error("rl_builder_set_sample_ages: one age per haplotype");
    return RL_EINVAL;
  }
  b->ages.assign(ages, ages + n);
  delete b->ages_tb;
  b->ages_tb = new rl::MinMatchAges(b->N, b->theta);
  if (b->dev) b->dev->forget_ages();
  return RL_OK;
}

int rl_builder_last_on_gpu(const rl_builder *b) { return b ? b->last_on_gpu : RL_EINVAL; }

int rl_builder_census(const rl_builder *b, long long *out, int n) {
  if (!b || !out || n < 0) {
    rl::set_error("rl_builder_census: bad arguments");
    return RL_EINVAL;
  }
  const rl::BuildCensus &c = b->ages_tb ? b->ages_tb->census : b->tb.census;
  for (int x = 0; x < n && x < rl::BuildCensus::COUNT; x++) out[x] = c.v[x];
  return rl::BuildCensus::COUNT;
}

}  // extern "C"

// minmatch_worker.hip -- the resident workers of the GPU tree builder: the build kernel (minmatch_build.h) as a
// persistent workgroup that pulls trees from a queue in pinned host memory, its variant for a tree size and the host
// thread that keeps enough of them alive.  The project's most expensive kernels compile here and nowhere else.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "common.h"
#include "minmatch.h"
#include "minmatch_build.h"
#include "minmatch_worker.h"

namespace rl {

namespace {

// A tree's parameters as a worker reads them from the queue: one 32-bit word per thread, uncached; from LDS every
// word goes through readfirstlane, so the builder keeps them in scalar registers as it did when they were kernel
// arguments.
__device__ inline void params_from_words(MMParamsDev &p, const unsigned *w) {
  unsigned *out = reinterpret_cast<unsigned *>(&p);
#pragma unroll
  for (int x = 0; x < (int)(sizeof(MMParams) / 4); x++) out[x] = __builtin_amdgcn_readfirstlane(w[x]);
}

// The builders' requests of one device and tree size, in pinned host memory: the host writes a request's words, then
// `tail`; workers claim tickets from `head` (device memory) and read the words of their ticket.
constexpr int MM_QUEUE_CAP = 1024;  // requests in flight <= builders alive (a section has one tree in flight)
constexpr int MM_LAUNCHES = 6;      // worker launches alive at once (a stream, i.e. a hardware queue, each)
constexpr int MM_XCDS = 8;          // a launch's workgroups are dealt to the XCDs in turn
constexpr int MM_WHOLE_ROUNDS = 64; // from this many workers on, launches and the goal are whole rounds of the XCDs
struct WorkQueue {
  unsigned tail;
  unsigned pad[15];
  unsigned gone[16];  // per launch: workers that have left (the host counts a launch's LIVE workers, not its size)
  unsigned words[MM_QUEUE_CAP][MM_PARAM_WORDS];
};
// device memory: the ticket counter, and per launch how many of its workers are building and when one last was
struct WorkerState {
  unsigned head;
  unsigned pad[15];
  struct {
    int busy;           // workers of the launch that are building
    unsigned activity;  // counts its claims and finished trees
    long long pad2[7];
  } launch[MM_LAUNCHES];
};

// One workgroup = one WORKER: it takes the next tree of the queue, builds it, says so in the request's own word of
// pinned memory and takes the next -- a tree starts the moment a worker is free instead of waiting for a launch to
// gather, and no launch lasts as long as its slowest tree.  The workers of a launch leave TOGETHER, when none of
// them has had a tree for `idle_ticks` (100 MHz): a launch holds its stream -- one of a few hardware queues -- until
// its last workgroup is gone, so workers that trickled away one by one would leave streams occupied by a few
// stragglers and no way to bring the others back.  Nothing a worker waits for can fail to arrive: the only loop
// without a tree in it is the idle one, bounded by the clock.
// OCC workgroups per CU: 2 * OCC waves per SIMD, 256 / OCC registers per lane (the plain build at N <= 5120: two).
template <int LAY, int MAXQ, bool AGES, int OCC>
__global__ void __launch_bounds__(MM_BLOCK) __attribute__((amdgpu_waves_per_eu(2 * OCC, 2 * OCC)))
    minmatch_worker(WorkQueue *q, WorkerState *ws, int launch, long long idle_ticks, int trace) {
  __shared__ Shared sh;
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  const int tid = threadIdx.x;
  auto &mine = ws->launch[launch];
  // (progress marks for RELATE_AMD_TIMING=2, in the queue's spare words: workers started / tickets claimed / trees
  //  left / workers gone)
  auto mark = [&](int which) {
    if (trace && tid == 0) __hip_atomic_fetch_add(&q->pad[which], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  };
  mark(0);
  // (one divergent block per turn -- thread 0 settles the accounts of the tree just built and claims the next --,
  //  then barriers and wave-uniform branches only: what follows an `if (tid == 0)` behind the build is laid out by
  //  the compiler as a loop over groups of lanes, and a barrier inside it is passed twice by thread 0's wave)
  bool had_tree = false;
  for (;;) {
    if (tid == 0) {
      if (had_tree) {
        if (trace) __hip_atomic_fetch_add(&q->pad[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_fetch_add(&mine.activity, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&mine.busy, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      unsigned ticket = ~0u;
      // (idle time is measured on this workgroup's own clock, from the last change of the launch's activity count it
      //  has seen: the counters of different XCDs are not one clock)
      unsigned seen = __hip_atomic_load(&mine.activity, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      long long since = wall_clock64();
      for (;;) {
        const unsigned h = __hip_atomic_load(&ws->head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned t = __hip_atomic_load(&q->tail, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
        if ((int)(t - h) > 0) {
          unsigned expected = h;
          if (__hip_atomic_compare_exchange_strong(&ws->head, &expected, h + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT)) {
            ticket = h;
            __hip_atomic_fetch_add(&mine.busy, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&mine.activity, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (trace) __hip_atomic_fetch_add(&q->pad[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
          }
          continue;
        }
        const unsigned act = __hip_atomic_load(&mine.activity, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long now = wall_clock64();
        if (act != seen) {
          seen = act;
          since = now;
        } else if (now - since > idle_ticks &&
                   __hip_atomic_load(&mine.busy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
          break;
        }
        __builtin_amdgcn_s_sleep(127);  // (~3 us: the queue is read across PCIe)
      }
      if (trace && ticket == ~0u) __hip_atomic_fetch_add(&q->pad[3], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (ticket == ~0u) __hip_atomic_fetch_add(&q->gone[launch], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      sh.ticket = ticket;
    }
    __syncthreads();
    const unsigned ticket = __builtin_amdgcn_readfirstlane(sh.ticket);
    if (ticket == ~0u) break;
    if (tid < MM_PARAM_WORDS)
      sh.praw[tid] = __hip_atomic_load(&q->words[ticket % MM_QUEUE_CAP][tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // what the tree's inputs were written with -- kernels of the builder's stream, finished before the request was
    // published -- may sit in other XCDs' L2 or stale in this one's: acquire at system scope, every wave
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    __syncthreads();
    MMParamsDev p;
    params_from_words(p, sh.praw);
    // rows of rebuilt clusters per pass of a merge: two while the registers allow (2: 110 ms per N = 5000 tree, 3: 119,
    // 4: 134 with 256 registers per lane)
    // (three / four rows, possible since a row costs 10 registers instead of 20: 114.2 / 114.4 ms per tree against 115.0
    //  -- the tests gain what the ordered part loses to spills: profiles/r06_rows_per_pass.json)
    build_tree<LAY, MAXQ, AGES, (OCC > 1 || MAXQ > MM_Q_LDS) ? 1 : 2>(p, sh, dyn);
    __syncthreads();  // (sh is the next tree's)
    had_tree = true;
  }
}

}  // namespace

// The restated generator against the library's, on the host: how many of n draws differ (0 expected).
static int rng_restatement_mismatches(unsigned seed, int n) {
  Rng r;
  rng_seed(r, seed);
  std::mt19937 ref(seed);
  std::uniform_real_distribution<double> unif(0.0, 1.0);
  int bad = 0;
  for (int i = 0; i < n; i++) bad += rng_unif(r) != unif(ref);
  return bad;
}

// ---- host side
// The worker kernel for trees of N leaves: where the state lives, register slots per thread, workgroups per CU.
//   plain build: L_HOT for every N -- 13 bytes of LDS per cluster next to ~14 KB of lists: two workgroups per CU up to
//                N = 5120 (4 slots per thread up to N = 2048, 10 above), one with 20 slots up to N = 10,240;
//   AGES build:  everything in LDS (33 bytes per cluster) up to N = 4100, in global memory above.
struct WorkerKind {
  int layout, maxq, occ;
  bool ages;
  const void *fn;
  size_t dyn;  // dynamic LDS per workgroup
};
static size_t lds_state_bytes(int layout, int N) {
  const size_t per = layout == L_LDS ? MM_LDS_PER_CLUSTER_LDS : layout == L_HOT ? MM_LDS_PER_CLUSTER_HOT
                     : layout == L_WARM ? MM_LDS_PER_CLUSTER_WARM : 0;
  return (per * (size_t)N + 255) & ~(size_t)255;
}
static size_t static_lds(const void *fn) {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, fn) == hipSuccess ? a.sharedSizeBytes : (size_t)1 << 30;
}
static WorkerKind worker_kind(int N, bool ages) {
  const size_t lds_cu = (size_t)160 * 1024;
  WorkerKind k{};
  k.ages = ages;
  if (ages) {
    const void *f_lds = reinterpret_cast<const void *>(&minmatch_worker<L_LDS, MM_Q_LDS, true, 1>);
    if (N <= MM_Q_LDS * MM_BLOCK && static_lds(f_lds) + lds_state_bytes(L_LDS, N) <= lds_cu)
      k = WorkerKind{L_LDS, MM_Q_LDS, 1, true, f_lds, lds_state_bytes(L_LDS, N)};
    else if (N <= MM_Q_LDS * MM_BLOCK)
      k = WorkerKind{L_GLOBAL, MM_Q_LDS, 1, true, reinterpret_cast<const void *>(&minmatch_worker<L_GLOBAL, MM_Q_LDS, true, 1>), 0};
    else
      k = WorkerKind{L_GLOBAL, MM_Q_GLOB, 1, true, reinterpret_cast<const void *>(&minmatch_worker<L_GLOBAL, MM_Q_GLOB, true, 1>), 0};
    return k;
  }
  const size_t dyn = lds_state_bytes(L_HOT, N);
  // Two workgroups per CU (128 registers per lane) hold half the CUs for the same workers -- the default where HBM
  // holds hundreds of sections' trees at once (small N; no measurable difference on a C4 chunk either way); at
  // N = 5000 a stage has ~134 sections open and a tree's latency decides: one per CU at 256 registers per lane, 1.33 x
  // faster per tree (profiles/r06_builder_many.jsonl, r06_c4_chunk_occ.json).  RELATE_AMD_BUILD_OCC=1 / 2 decides
  // otherwise.
  static const int occ_env = getenv("RELATE_AMD_BUILD_OCC") ? atoi(getenv("RELATE_AMD_BUILD_OCC")) : 0;
  const int occ_max = occ_env > 0 ? occ_env : (N <= MM_Q_SMALL * MM_BLOCK ? 2 : 1);
  if (N <= MM_Q_SMALL * MM_BLOCK && occ_max >= 2) {
    const void *f = reinterpret_cast<const void *>(&minmatch_worker<L_HOT, MM_Q_SMALL, false, 2>);
    if (2 * (static_lds(f) + dyn) <= lds_cu) return WorkerKind{L_HOT, MM_Q_SMALL, 2, false, f, dyn};
  }
  if (N <= MM_Q_LDS * MM_BLOCK && occ_max >= 2) {
    const void *f = reinterpret_cast<const void *>(&minmatch_worker<L_HOT, MM_Q_LDS, false, 2>);
    if (2 * (static_lds(f) + dyn) <= lds_cu) return WorkerKind{L_HOT, MM_Q_LDS, 2, false, f, dyn};
  }
  if (N <= MM_Q_LDS * MM_BLOCK) {  // one per CU: the row minima in LDS too
    const void *f = reinterpret_cast<const void *>(&minmatch_worker<L_WARM, MM_Q_LDS, false, 1>);
    return WorkerKind{L_WARM, MM_Q_LDS, 1, false, f, lds_state_bytes(L_WARM, N)};  // (107 + 15 KB at N = 5120)
  }
  return WorkerKind{L_HOT, MM_Q_GLOB, 1, false, reinterpret_cast<const void *>(&minmatch_worker<L_HOT, MM_Q_GLOB, false, 1>), dyn};
}
// workgroups of a tree's worker kernel a CU holds
int device_builder_workers_per_cu(int N, bool ages) { return worker_kind(N, ages).occ; }
int debug_worker_kind(int N, bool ages, int *layout, int *slots, int *per_cu) {
  const WorkerKind k = worker_kind(N, ages);
  *layout = k.layout;
  *slots = k.maxq;
  *per_cu = k.occ;
  return 0;
}
int worker_layout(int N, bool ages) { return worker_kind(N, ages).layout; }

// The builders of one device and one tree size hand their trees to WORKERS -- resident workgroups that pull
// requests from a queue in pinned host memory (minmatch_worker).  Why not a launch per tree, or per batch of
// trees: a process has a dozen hardware queues and kernels of one queue run one after the other, so 150 sections
// with a stream each build a dozen trees at a time; batched launches (round 2) waited 10 ms to gather, lasted as
// long as their slowest tree and kept at most 4 x ~15 trees in flight on 256 CUs.
// The launcher thread adds workers when trees wait: up to MM_LAUNCHES launches alive (a lowest-priority stream
// each; more than ~20 hardware queues in all and the device time-slices them), each at least half as large as
// what is alive -- 16, 16, 16, 24, 36, 54 ... -- up to the workers the job can use (the CUs less an eighth, or the
// builders the stage announced, expect()).
class BuildQueue {
 public:
  // (ages: the builders with sample ages have workers of their own -- another kernel)
  static BuildQueue *of(int device, int N, bool ages = false) {
    // (the queues live as long as the process and are never destroyed: their launcher threads wait on them)
    static std::mutex gm;
    static std::vector<BuildQueue *> *all = new std::vector<BuildQueue *>();
    std::lock_guard<std::mutex> lk(gm);
    for (BuildQueue *q : *all)
      if (q->device_ == device && q->N_ == N && q->ages_ == ages) return q;
    BuildQueue *q = new BuildQueue(device, N, ages);
    if (!q->ok_) return nullptr;
    all->push_back(q);
    return q;
  }
  // the most workers the caller wants alive (the stage: its section threads, fewer when RePaint needs the chip); 0: no
  // word
  void expect(int builders) {
    std::lock_guard<std::mutex> lk(m_);
    expected_ = builders;
  }
  // ... of SEVERAL callers that share the device (target ranges as threads of one process, shard.cpp): each adds what
  // it asks for and takes it off again
  void expect_add(int delta) {
    std::lock_guard<std::mutex> lk(m_);
    expected_ = std::max(0, expected_ + delta);
  }
  // Publishes the tree and returns when ITS worker says it is out (p.host_done, -1 until then): 0, or RL_EHIP.
  int run(const MMParams &p) {
    {
      std::lock_guard<std::mutex> lk(m_);
      const unsigned t = published_++;
      MMParams pp = p;
      pp.trace = timing_level() >= 2 ? &q_->pad[8] : nullptr;
      memcpy(q_->words[t % MM_QUEUE_CAP], &pp, sizeof(MMParams));
      __atomic_store_n(&q_->tail, published_, __ATOMIC_RELEASE);
      outstanding_++;
    }
    cv_.notify_one();
    int rc = 0;
    const auto t0 = std::chrono::steady_clock::now();
    static const bool trace = (timing_level() >= 2);
    auto last_trace = t0;
    for (unsigned spins = 0;; spins++) {
      if (__atomic_load_n(p.host_done, __ATOMIC_ACQUIRE) != -1) break;
      if (trace && std::chrono::steady_clock::now() - last_trace > std::chrono::seconds(1)) {
        last_trace = std::chrono::steady_clock::now();
        fprintf(stderr, "[mm trace] N=%d waiting %.0f s: %s, outstanding %d; last mark: %u clusters left, phase %u\n", N_,
                std::chrono::duration<double>(last_trace - t0).count(), trace_counters().c_str(), outstanding_,
                __atomic_load_n(&q_->pad[8], __ATOMIC_ACQUIRE), __atomic_load_n(&q_->pad[9], __ATOMIC_ACQUIRE));
        fflush(stderr);
      }
      if (failed_.load()) {
        rc = RL_EHIP;
        break;
      }
      std::this_thread::sleep_for(std::chrono::microseconds(spins < 50 ? 100 : 250));
      if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(600)) {
        // (the request may still be claimed or finished by a worker: the queue is done for -- every builder's wait
        //  ends with an error -- and the caller keeps this tree's buffers out of circulation, ~DeviceMinMatch)
        set_error("tree builder: the tree was not built within 10 minutes");
        failed_.store(true);
        rc = RL_EHIP;
        break;
      }
    }
    std::lock_guard<std::mutex> lk(m_);
    outstanding_--;
    return rc;
  }

 private:
  BuildQueue(int device, int N, bool ages) : device_(device), N_(N), ages_(ages), kind_(worker_kind(N, ages)) {
    if (hipSetDevice(device) != hipSuccess) return;
    if (hipHostMalloc(reinterpret_cast<void **>(&q_), sizeof(WorkQueue), hipHostMallocCoherent) != hipSuccess) return;
    memset(q_, 0, sizeof(WorkQueue));
    if (d_state_.alloc(sizeof(WorkerState)) || hipMemset(d_state_.p, 0, sizeof(WorkerState)) != hipSuccess) return;
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    // `occ` workers share a CU; an eighth of the chip stays free for the stage's short kernels (RePaint, distance
    // matrices, weave) unless the stage says otherwise (expect())
    cap_ = env_int("RELATE_AMD_BUILD_WORKERS", kind_.occ * (cus - cus / 8), 1, 1024);
    cap_from_env_ = getenv("RELATE_AMD_BUILD_WORKERS") != nullptr;
    ok_ = true;
    std::thread([this] { launcher(); }).detach();
  }
  std::string trace_counters() const {  // (RELATE_AMD_TIMING=2) requests published, the workers' progress marks
    char buf[160];
    snprintf(buf, sizeof(buf), "published %u, workers started %u, tickets claimed %u, trees left %u, workers gone %u",
             __atomic_load_n(&q_->tail, __ATOMIC_ACQUIRE), __atomic_load_n(&q_->pad[0], __ATOMIC_ACQUIRE),
             __atomic_load_n(&q_->pad[1], __ATOMIC_ACQUIRE), __atomic_load_n(&q_->pad[2], __ATOMIC_ACQUIRE),
             __atomic_load_n(&q_->pad[3], __ATOMIC_ACQUIRE));
    return buf;
  }
  void launcher() {
    (void)hipSetDevice(device_);
    // The workers run for as long as there are trees; the short kernels of the stage must not queue up behind a
    // launch in a hardware queue they happen to share: lowest-priority streams, which the runtime maps to hardware
    // queues of their own.
    hipStream_t streams[MM_LAUNCHES];
    int size[MM_LAUNCHES] = {};
    for (auto &st : streams)
      if (make_stream(&st, true) != hipSuccess) {
        failed_.store(true);
        return;
      }
    const size_t dyn = kind_.dyn;
    // (the per-cluster state of a build in LDS: more than the default 64 KB of dynamic LDS)
    if (dyn > 0 && hipFuncSetAttribute(kind_.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) {
      failed_.store(true);
      return;
    }
    const bool verbose = getenv("RELATE_AMD_TIMING") != nullptr;
    auto ended = [&](int l) { size[l] = 0, g_worker_launches.fetch_sub(1); };  // launch l is over: off the count
    for (;;) {
      int demand = 0, goal = 0;
      {
        std::unique_lock<std::mutex> lk(m_);
        static const bool trace = (timing_level() >= 2);
        while (trace && !cv_.wait_for(lk, std::chrono::milliseconds(500), [&] { return outstanding_ > 0; })) {
          fprintf(stderr, "[mm trace] N=%d idle: %s; streams busy:", N_, trace_counters().c_str());
          for (int l = 0; l < MM_LAUNCHES; l++) fprintf(stderr, " %d", hipStreamQuery(streams[l]) == hipSuccess ? 0 : size[l]);
          fprintf(stderr, "\n");
          fflush(stderr);
        }
        // While a launch of workers is alive the loop keeps polling (its workers leave 50 ms after the last tree):
        // the library's memory cache may trim -- hipFree waits for the device -- only when none is (g_worker_launches).
        int launches_alive = 0;
        for (int l = 0; l < MM_LAUNCHES; l++) launches_alive += size[l] > 0;
        if (launches_alive > 0) {
          if (!cv_.wait_for(lk, std::chrono::milliseconds(20), [&] { return outstanding_ > 0; })) {
            lk.unlock();
            for (int l = 0; l < MM_LAUNCHES; l++)
              if (size[l] > 0 && hipStreamQuery(streams[l]) == hipSuccess) ended(l);
            continue;
          }
        } else {
          cv_.wait(lk, [&] { return outstanding_ > 0; });
        }
        demand = outstanding_;
        // (the stage's word, expect(), is a limit -- it knows what RePaint needs of the chip; RELATE_AMD_BUILD_WORKERS
        //  overrides it)
        goal = (expected_ > 0 && !cap_from_env_) ? std::min(cap_, expected_) : cap_;
        // whole rounds of the XCDs (below): the goal too -- where the workers are many enough for their spread over the
        // XCDs to matter (a stage of 43 sections lost 3 of its workers to the rounding: config #5 on one GPU)
        if (goal >= MM_WHOLE_ROUNDS) goal -= goal % MM_XCDS;
      }
      int alive = 0, free_stream = -1;
      for (int l = 0; l < MM_LAUNCHES; l++) {
        if (size[l] > 0 && hipStreamQuery(streams[l]) == hipSuccess) ended(l);
        // (workers decide to leave one by one -- idle past the limit and nobody of the launch building --, so a late
        //  claim can keep one of them at work while its peers are gone: a launch counts for the workers it still has)
        alive += size[l] - std::min(size[l], (int)__atomic_load_n(&q_->gone[l], __ATOMIC_ACQUIRE));
        if (size[l] == 0 && free_stream < 0) free_stream = l;
      }
      // Workers follow the trees that are waiting or being built, not the sections that exist: a section spends half
      // of its time outside the build (distance matrix, RePaint, mapping), and a worker without a tree still holds
      // its CU -- with one per section RePaint had 122 CUs of 256 and was the stage's bottleneck (82 % busy, 0.7 s of
      // queue per launch).  A launch adds what is missing plus a margin, at least half of what is alive (the
      // launches are few: MM_LAUNCHES streams), never past the goal.
      if (demand + 4 > alive && alive < goal && free_stream >= 0) {
        int n = std::max({demand + 8 - alive, alive / 2, 16});
        // Workgroup b of a launch goes to XCD b % 8, every launch starting at XCD 0 again: launches of any size pile
        // their remainders on the low XCDs (six launches: up to six workers more there than on XCD 7), and a RePaint
        // launch -- its workgroups dealt to the XCDs in the same round-robin -- lasts as long as the XCD with the
        // fewest CUs left.  Whole rounds only.
        if (goal >= MM_WHOLE_ROUNDS) {
          n = (n + MM_XCDS - 1) / MM_XCDS * MM_XCDS;
          // (`alive` counts live workers since round 4, so what is missing need not be a whole round: wait until it is)
          n = std::min(n, (goal - alive) / MM_XCDS * MM_XCDS);
          if (n <= 0) {
            std::this_thread::sleep_for(std::chrono::microseconds(300));
            continue;
          }
        } else {
          n = std::max(1, std::min(n, goal - alive));
        }
        const int l = free_stream;
        __atomic_store_n(&q_->gone[l], 0u, __ATOMIC_RELEASE);  // (the stream's previous launch is through)
        const long long idle = (long long)idle_ms_ * 100000LL;
        const int trace_flag = timing_level() >= 2 ? 1 : 0;
        {
          WorkQueue *a_q = q_;
          WorkerState *a_ws = d_state_.as<WorkerState>();
          int a_l = l, a_trace = trace_flag;
          long long a_idle = idle;
          void *args[] = {&a_q, &a_ws, &a_l, &a_idle, &a_trace};
          (void)hipLaunchKernel(kind_.fn, dim3((unsigned)n), dim3(MM_BLOCK), args, dyn, streams[l]);
        }
        if (hipGetLastError() != hipSuccess) {
          // (this thread ends: the launches it still counted alive are nobody's to take off the count any more --
          //  the memory cache would wait for them on every failed allocation, and never trim)
          for (int m = 0; m < MM_LAUNCHES; m++)
            if (size[m] > 0) ended(m);
          failed_.store(true);
          return;
        }
        size[l] = n;
        g_worker_launches.fetch_add(1);
        if (verbose) {
          fprintf(stderr, "[tree builder workers] +%d on stream %d: %d alive, %d trees waiting or being built, goal %d\n", n,
                  l, alive + n, demand, goal);
          fflush(stderr);
        }
      }
      std::this_thread::sleep_for(std::chrono::microseconds(300));
    }
  }
  int device_, N_;
  bool ages_, ok_ = false;
  WorkerKind kind_;
  WorkQueue *q_ = nullptr;
  DevBuf d_state_;
  int cap_ = 224, idle_ms_ = 50;
  bool cap_from_env_ = false;
  std::mutex m_;
  std::condition_variable cv_;
  unsigned published_ = 0;
  int outstanding_ = 0, expected_ = 0;
  std::atomic<bool> failed_{false};
};
BuildQueue *build_queue_of(int device, int N, bool ages) { return BuildQueue::of(device, N, ages); }
int build_queue_run(BuildQueue *q, const MMParams &p) { return q->run(p); }
int device_builder_expect(int device, int N, int builders, bool ages) {
  BuildQueue *q = hipSetDevice(device) == hipSuccess ? BuildQueue::of(device, N, ages) : nullptr;
  if (q) q->expect(builders);
  return q ? 0 : -1;
}
int device_builder_expect_add(int device, int N, int delta, bool ages) {
  BuildQueue *q = hipSetDevice(device) == hipSuccess ? BuildQueue::of(device, N, ages) : nullptr;
  if (q) q->expect_add(delta);
  return q ? 0 : -1;
}

}  // namespace rl

extern "C" int rl_debug_rng_mismatches(unsigned seed, int n) { return rl::rng_restatement_mismatches(seed, n); }

extern "C" int rl_debug_builder_kind(int N, int ages, int *layout, int *slots, int *per_cu) {
  if (N < 2 || N > rl::MM_MAXN || !layout || !slots || !per_cu) {
    rl::set_error("rl_debug_builder_kind: bad arguments (N=%d)", N);
    return RL_EINVAL;
  }
  int devices = 0;  // (the choice depends on the kernels' static LDS, which the runtime tells with a device only)
  if (hipGetDeviceCount(&devices) != hipSuccess || devices < 1) {
    rl::set_error("rl_debug_builder_kind: no usable HIP device");
    return RL_EHIP;
  }
  return rl::debug_worker_kind(N, ages != 0, layout, slots, per_cu);
}

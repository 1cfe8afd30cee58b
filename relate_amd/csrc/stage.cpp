// stage.cpp -- the BuildTopology stage: how the sections of a chunk share one GPU.
//
// The stage driver of pipeline/BuildTopology.cpp:14-167 (and of pipeline/OptimizeParameters.cpp:22-206) for the
// tree-sequence loop of treeseq.cpp.  Sections are independent (the reference's scripts run them as separate
// processes, scripts/RelateParallel/RelateParallel.sh:231-257): here a few host threads each run one section's
// tree-sequence loop and share the GPU.  The stage sizes itself against HBM (stage_plan.h), admits every window
// against the memory that is free when it opens (AdmissionGate) and deals the sections to its threads.
#include <sched.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <mutex>
#include <thread>

#include "common.h"
#include "minmatch.h"
#include "stage_plan.h"
#include "treeseq.h"

using namespace rl;

namespace {
std::mutex g_gpu_mutex;           // admission and closing of the windows of every stage of the process
std::string g_stage_sample_ages;  // rl_stage_set_sample_ages: the --sample_ages file of the following stage calls

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

// (a window's matrices run on the window's own stream; what the windows of a context share -- RePaint's strips --
//  is locked inside, window.cpp)
static int win_matrix(void *user, int snp, float *d) { return rl_window_matrix((rl_window *)user, snp, d, nullptr); }
static int win_matrix_dev(void *user, int snp, void *d_dev) {
  return rl_window_matrix_rows_device((rl_window *)user, snp, d_dev, nullptr);
}
static int win_matrix_dev_ex(void *user, int snp, void *d_dev, const char *carriers, float val, void *d_rowmin) {
  return rl_window_matrix_rows_device_ex((rl_window *)user, snp, d_dev, carriers, val, d_rowmin, nullptr);
}
static int win_advance(void *user, int snp) { return rl_window_advance((rl_window *)user, snp); }

// A stage's knobs: the caller's rl_stage_opts (per call), overridden by the RELATE_AMD_* environment variables --
// those are for experiments (tools/, profiles/): what a consumer of the ABI sets goes through the struct.
static long long knob(const char *env, long long from_opts, bool opts_set, long long fallback) {
  if (const char *e = getenv(env)) return atoll(e);
  return opts_set ? from_opts : fallback;
}

// Host cores that share a last-level cache, as cpu sets this process may run on.  One section (its builder thread
// and the helpers that split a merge, minmatch.h) is kept inside one such group: the helpers hand each other a few
// cache lines per merge, tens of thousands of times a second, and the matrices are first touched -- so placed on
// the NUMA node -- by the thread that builds with them.  RELATE_AMD_PIN=0 leaves placement to the scheduler.
static std::vector<cpu_set_t> cache_groups(int pin_opt) {
  std::vector<cpu_set_t> groups;
  if (knob("RELATE_AMD_PIN", pin_opt, pin_opt >= 0, 1) == 0) return groups;
  cpu_set_t allowed;
  CPU_ZERO(&allowed);
  if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return groups;
  std::vector<std::string> keys;
  for (int cpu = 0; cpu < CPU_SETSIZE; cpu++) {
    if (!CPU_ISSET(cpu, &allowed)) continue;
    char path[128];
    snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", cpu);
    FILE *fp = fopen(path, "r");
    if (!fp) return std::vector<cpu_set_t>();
    char buf[256] = {0};
    const bool ok = fgets(buf, sizeof(buf), fp) != nullptr;
    fclose(fp);
    if (!ok) return std::vector<cpu_set_t>();
    size_t g = 0;
    while (g < keys.size() && keys[g] != buf) g++;
    if (g == keys.size()) {
      keys.push_back(buf);
      cpu_set_t empty;
      CPU_ZERO(&empty);
      groups.push_back(empty);
    }
    CPU_SET(cpu, &groups[g]);
  }
  if (groups.size() < 2) groups.clear();  // one cache for everything: nothing to choose
  return groups;
}

// A section thread inside one cache group for as long as the object lives.  Slots alternate between the two halves
// of the list (= the sockets, as the cpus are numbered); several ranks on the host, one per GPU, each keep to their
// own share of the groups.
class PinnedToGroup {
 public:
  PinnedToGroup(const std::vector<cpu_set_t> &groups, std::atomic<int> &next_slot) {
    CPU_ZERO(&before);
    pinned = !groups.empty() && sched_getaffinity(0, sizeof(before), &before) == 0;
    if (!pinned) return;
    const int LW = std::min(local_world_size(), (int)groups.size()), lr = local_rank() % LW;
    const int g0 = (int)groups.size() * lr / LW, G = (int)groups.size() * (lr + 1) / LW - g0;
    const int slot = next_slot.fetch_add(1), half = (G + 1) / 2;
    const int g = g0 + ((slot % 2) * half + (slot / 2) % half) % G;
    sched_setaffinity(0, sizeof(cpu_set_t), &groups[g]);
  }
  ~PinnedToGroup() {
    if (pinned) sched_setaffinity(0, sizeof(before), &before);
  }

 private:
  cpu_set_t before;
  bool pinned = false;
};

// --sample_ages file (pipeline/BuildTopology.cpp:93-108): the first N numbers of a plain or gzip text file.  A file
// that cannot be opened leaves N zeros (and a warning), one with fewer than N numbers no ages at all -- as there.
static std::vector<double> read_sample_ages(const char *fn, int N) {
  std::vector<double> ages(N, 0.0);
  gzFile gz = gzopen(fn, "rb");  // (plain text passes through zlib unchanged; no shell, whatever the path holds)
  if (!gz) {
    std::cerr << "Warning: unable to open sample ages file" << std::endl;
    return ages;
  }
  std::string text;
  char buf[1 << 16];
  int got;
  while ((got = gzread(gz, buf, sizeof(buf))) > 0) text.append(buf, (size_t)got);
  const bool broken = got < 0;
  gzclose(gz);
  int i = 0;
  const char *p = text.c_str();
  while (i < N) {
    char *e = nullptr;
    const double v = strtod(p, &e);
    if (e == p) break;
    ages[i++] = v;
    p = e;
  }
  if (i < N) {  // (the reference's loop leaves the vector short and the builder then ignores it: no ages)
    std::cerr << "Warning: " << fn << (broken ? " cannot be decompressed: " : " holds ") << i << " of " << N
              << " sample ages; building without sample ages" << std::endl;
    ages.clear();
  }
  return ages;
}

// chunk_<c>.bp / .state (data.cpp:485-516, :307-345): --fb and the mapping of transitions read them; a missing or
// short file would give wrong trees without a word
static int read_chunk_ints(const std::string &fn, int L, std::vector<int> &v) {
  FILE *fp = fopen(fn.c_str(), "rb");
  if (!fp) {
    set_error("cannot open %s", fn.c_str());
    return RL_EIO;
  }
  int n = 0;
  const bool ok = fread(&n, 4, 1, fp) == 1 && n == L && fread(v.data(), 4, (size_t)L, fp) == (size_t)L;
  fclose(fp);
  if (!ok) {
    set_error("%s does not hold %d values", fn.c_str(), L);
    return RL_EFORMAT;
  }
  return RL_OK;
}

// the bp positions and ancestral-state flags of a chunk's L SNPs: what a tree sequence takes when no file says otherwise
struct SnpColumns {
  std::vector<int> bp, state;
  explicit SnpColumns(int L) : bp(L, 0), state(L, 1) {}
  int read(const std::string &chunk_prefix) {  // <out_dir>/chunk_<c>
    const int L = (int)bp.size();
    const int rc = read_chunk_ints(chunk_prefix + ".bp", L, bp);
    return rc ? rc : read_chunk_ints(chunk_prefix + ".state", L, state);
  }
};

// output name = basename of -o (Relate requires -o to be a bare name, Relate.cpp:50-58)
static std::string output_base_name(std::string base) {
  while (!base.empty() && base.back() == '/') base.pop_back();
  const size_t sl = base.find_last_of('/');
  return sl != std::string::npos ? base.substr(sl + 1) : base;
}

// How many resident tree-builder workers a stage asks for.  The reference's unit of parallelism is a section job
// (scripts/RelateParallel/RelateParallel.sh:231-257: one process per section range); here a section has at most ONE tree
// in flight, so:
//   * never more workers than open sections (what HBM admits: ~134 at N = 5000, ~70 at N = 10,000, 256 at N = 2000);
//   * whole windows resident (RePaint runs once per window, then the chip is the trees'): a worker per section, up to
//     7/8 of the worker slots -- an eighth of the CUs stays with the sections' own short kernels;
//   * bounded windows (RePaint runs all through the stage, on the CUs the workers leave, and every section waits in
//     its queue): 29/64 of the CUs.  Measured at C3 over three rounds (profiles/r03..r05_c3_*): 3/8 -> 13/32 -> 29/64
//     as the per-tree kernels got lighter; past ~31/64 the stage is bistable (RePaint's lane saturates and the
//     sections fall into a convoy: 143 s and 185 s from the same 124 workers), so the rule stays a whole XCD round
//     (8 workers) below that edge.  profiles/r06_worker_rule.json: the rule against 0.75x / 1.25x / 1.5x of it at
//     N = 2000, 5000 and 10,000;
//   * `per_cu` worker slots per CU (two for the small-N kernel, minmatch_worker.hip worker_kind): the CU share above is a
//     share of CUs, the slots on them follow.
// (A tree's time in the stage does not depend on the worker count -- 142-150 ms from 116 to 148 workers,
//  profiles/r05_c3_runs.json --; past the share above it is RePaint, on the CUs left, that every section waits for.)
namespace rl {
int stage_worker_goal(int cus, int open_sections, bool bounded_windows, int per_cu) {
  const int share = bounded_windows ? 29 * cus / 64 : cus - cus / 8;
  int goal = std::max(1, std::min(open_sections, share * std::max(1, per_cu)));
  // (whole rounds of the 8 XCDs once the workers are many -- a launch's workgroups go to the XCDs in turn, and RePaint
  //  lasts as long as the XCD with the fewest CUs left: C3's 116 are 112 alive)
  if (goal >= 64) goal -= goal % 8;
  return goal;
}
}  // namespace rl

// ---- admission: which windows are open at once --------------------------------------------------------------------
// A section's window opens when it fits next to the ones that are open or being opened -- against the HBM that is
// free at that moment, not against the plan's estimate -- and an open that fails for memory although admitted (the
// estimate counts bytes, the allocator needs blocks) is asked again while other sections hold memory they will give
// back.  One gate per stage, shared by its section threads.
class AdmissionGate {
 public:
  // Out of memory although admitted: not the stage's failure while other sections hold memory they will give back
  // -- wait for one to close and ask again.  Alone on the device it IS the failure.
  // (bounded: two threads that keep failing while each sees the other's reservation would otherwise retry for
  //  ever -- after 20 admitted-but-failed opens of this section it IS the stage's failure)
  static constexpr int kRetriesWhileOthersHold = 20;
  // (alone by now -- the sections that held memory a moment ago may just have closed, and what they gave back
  //  sits in the cache: twice more before it is the stage's failure)
  static constexpr int kRetriesAlone = 2;
  static constexpr int kClosePolls = 1200;  // polls of kPollMs for another section to close before asking again: a minute
  static constexpr int kPollMs = 50;        // ... and between two looks at the free memory
  static constexpr int kAloneWaitMs = 100;  // before an open is repeated with nothing else open

  AdmissionGate(rl_ctx *ctx, const StagePlan &plan, bool from_files, bool gpu_build, bool ages, int device, int sum_mode,
                const std::atomic<int> &stage_error)
      : ctx(ctx), plan(plan), from_files(from_files), gpu_build(gpu_build), ages(ages), device(device), sum_mode(sum_mode),
        stage_error(stage_error),
        // (test hook, read once per stage: tests/test_stage_gpu.py)
        fail_opens(getenv("RELATE_AMD_TEST_FAIL_OPENS") ? atoi(getenv("RELATE_AMD_TEST_FAIL_OPENS")) : 0) {}

  // The window of `section` (and, on the thread's first section, its device builder in ts), or nullptr with *status:
  // the stage's error if another thread has failed meanwhile, RL_ENOMEM when memory ran out, else RL_EIO.
  rl_window *open(rl_treeseq *ts, int section, const char *paint_file, int start, int *status) {
    // (this thread's builder keeps its buffers from section to section: only the first one asks for them)
    const bool builder_new = gpu_build && !ts->dev_builder;
    const double need = plan.window_bytes(section) + (builder_new ? plan.builder_bytes : 0.0);
    const size_t min_block = plan.min_block(section);
    rl_window *win = nullptr;
    int open_rc = RL_EIO, oom_alone = 0, oom_total = 0;
    for (;;) {  // wait until the window fits next to the ones that are open or being opened
      if (!admit(need, min_block)) {
        if (stage_error.load()) break;
        std::this_thread::sleep_for(std::chrono::milliseconds(kPollMs));
        continue;
      }
      // (reading and decoding the paint file, the uploads and RePaint: outside the lock)
      const unsigned oom_before = tl_alloc_failures;
      win = try_open(ts, section, paint_file, start, builder_new);
      bool others;
      {
        std::lock_guard<std::mutex> lk(g_gpu_mutex);
        reserved_bytes -= need;
        if (win) most_open = std::max(most_open, ++open_sections);
        others = open_sections.load() > 0 || reserved_bytes > 0.0;
      }
      if (win) break;
      const bool oom = tl_alloc_failures != oom_before;
      if (oom) open_rc = RL_ENOMEM;
      if (oom && others && !stage_error.load() && ++oom_total <= kRetriesWhileOthersHold) {
        const int open_then = open_sections.load();
        for (int i = 0; i < kClosePolls && open_sections.load() >= open_then && open_sections.load() > 0 &&
                        !stage_error.load(); i++)
          std::this_thread::sleep_for(std::chrono::milliseconds(kPollMs));
        std::this_thread::sleep_for(std::chrono::milliseconds(kPollMs));
        continue;
      }
      if (oom && !stage_error.load() && ++oom_alone <= kRetriesAlone) {
        std::this_thread::sleep_for(std::chrono::milliseconds(kAloneWaitMs));
        continue;
      }
      break;
    }
    *status = win ? RL_OK : (stage_error.load() ? stage_error.load() : open_rc);
    return win;
  }

  void close(rl_window *win) {
    std::lock_guard<std::mutex> lk(g_gpu_mutex);
    rl_window_close(win);
    open_sections--;
  }

  int most_open_at_once() const { return most_open; }  // (after the section threads have ended)

 private:
  // promises `need` bytes to the caller if they are free next to what is promised already
  bool admit(double need, size_t min_block) {
    std::lock_guard<std::mutex> lk(g_gpu_mutex);
    size_t free_b = 0, total_b = 0;
    const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    // (closed windows give their blocks to the library's cache, not to the driver: what the cache holds in
    //  blocks of a useful size is free for the next window too)
    if (!known || (double)free_b + (double)device_cache_held(device, min_block) - reserved_bytes >= need ||
        (open_sections.load() == 0 && reserved_bytes == 0.0)) {
      reserved_bytes += need;
      return true;
    }
    return false;
  }

  // an admitted open: the window and, while the reservation stands, the thread's device builder
  rl_window *try_open(rl_treeseq *ts, int section, const char *paint_file, int start, bool builder_new) {
    // (test hook, RELATE_AMD_TEST_FAIL_OPENS=k: k > 0 -- the next k admitted opens that happen while another
    //  section is open fail as if the device were out of memory; k < 0 -- the next |k| opens whatever else is
    //  open.  The retry in open() is otherwise reached only when the allocator really runs dry)
    bool injected = false;
    if (fail_opens.load() > 0 && open_sections.load() > 0) injected = fail_opens.fetch_sub(1) > 0;
    else if (fail_opens.load() < 0) injected = fail_opens.fetch_add(1) < 0;
    if (injected) {
      tl_alloc_failures++;
      set_error("hipMalloc failed (injected by RELATE_AMD_TEST_FAIL_OPENS)");
      return nullptr;
    }
    rl_window *win = rl_window_open_bounded(ctx, section, from_files ? paint_file : nullptr, start, sum_mode, plan.cap_rows,
                                            nullptr);
    if (win && builder_new) {
      ts->dev_builder = new DeviceMinMatch(ctx->N, device);
      if (ts->dev_builder->reserve(ages)) {
        rl_window_close(win);
        win = nullptr;
        delete ts->dev_builder;
        ts->dev_builder = nullptr;
        tl_alloc_failures++;
      }
    }
    return win;
  }

  rl_ctx *ctx;
  const StagePlan &plan;
  const bool from_files, gpu_build, ages;
  const int device, sum_mode;
  const std::atomic<int> &stage_error;  // the stage's first error: nobody waits for memory once it is set
  std::atomic<int> fail_opens;
  std::atomic<int> open_sections{0};
  int most_open = 0;            // (under g_gpu_mutex)
  double reserved_bytes = 0.0;  // (under g_gpu_mutex) HBM promised to windows that are being opened
};

// ---- the sections of one call ------------------------------------------------------------------------------------
// owns the context of a stage call unless the caller keeps it (OptimizeParameters: one context for every grid point)
struct ContextGuard {
  rl_ctx *ctx;
  ~ContextGuard() { release(); }
  void release() {
    if (ctx) rl_destroy(ctx);
    ctx = nullptr;
  }
};

// What the plan is made from: the chunk's sizes, the census of posterior rows per section (summed over the context's
// targets) and the knobs, each resolved here once.  (room: reserve_and_plan, after the reservations)
static StageInputs stage_inputs(const rl_ctx *ctx, const rl_stage_opts &o, int first_section, int last_section,
                                bool from_files) {
  StageInputs in;
  const int W = ctx->W;
  in.N = ctx->N;
  in.nloc = ctx->nloc;
  in.S = ctx->S;
  in.waves = ctx->waves;
  in.first_section = first_section;
  in.last_section = last_section;
  in.rows_of.assign(W, 0.0);
  for (int w = first_section; w <= last_section; w++) {
    for (int n = ctx->k0; n < ctx->k0 + ctx->nloc; n++)
      in.rows_of[w] += ctx->plan.ie[(size_t)n * W + w] - ctx->plan.ia[(size_t)n * W + w] + 1;
    in.max_rows = std::max(in.max_rows, in.rows_of[w]);
  }
  in.stones_per_window = from_files || ctx->h_alpha;
  // The trees themselves are built on the GPU too (minmatch_builder.hip) when the call covers several sections: a tree
  // takes one workgroup ~115 ms at N = 5000 against ~85 ms on 8 host threads, but the workgroups of different
  // sections run side by side (40 sections: 98 s against 331 s).  RELATE_AMD_GPU_BUILD=0 / 1 decides otherwise.
  in.gpu_build = knob("RELATE_AMD_GPU_BUILD", o.gpu_build, o.gpu_build >= 0, last_section > first_section) != 0;
  in.host_threads = host_threads();
  in.window_rows_set = getenv("RELATE_AMD_WINDOW_ROWS") || o.window_rows != 0;
  in.window_rows = knob("RELATE_AMD_WINDOW_ROWS", o.window_rows, true, 0);
  in.window_parts = knob("RELATE_AMD_WINDOW_PARTS", o.window_parts, o.window_parts > 0, 32);
  in.section_threads_set = getenv("RELATE_AMD_SECTION_THREADS") || o.section_threads > 0;
  in.section_threads = knob("RELATE_AMD_SECTION_THREADS", o.section_threads, true, 0);
  in.repaint_lanes = knob("RELATE_AMD_REPAINT_LANES", o.repaint_lanes, o.repaint_lanes > 0, 1);
  in.repaint_checkpoint = REPAINT_CHECKPOINT;
  in.repaint_side = REPAINT_SIDE;
  return in;
}

// The stage's reservations and its plan, in the order the admission counts on: the builders' pools, RePaint's strips,
// then what is free, the plan for it, the second lane if the plan wants one.  RL_ENOMEM, or RL_OK and the plan.
static int reserve_and_plan(rl_ctx *ctx, const rl_stage_opts &o, StageInputs &in, StagePlan &plan) {
  if (in.gpu_build && device_builder_reserve_shared(o.device, ctx->N)) return RL_ENOMEM;  // the pools now: the admission sees what is left
  if (ctx->d_k2_scratch.alloc(repaint_scratch_bytes((int64_t)in.max_rows, ctx->nloc, ctx->S, ctx->waves))) return RL_ENOMEM;
  size_t free_b = 0, total_b = 0;
  in.room_known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
  in.room = in.room_known ? 0.9 * (double)free_b : 0.0;
  plan = plan_sections(in);
  if (plan.wants_second_lane && !ctx->two_lanes) {
    auto &ln = ctx->lane2;
    if (ln.scratch.alloc(plan.lane2_scratch_bytes) == 0 && make_stream(&ln.s, false) == hipSuccess &&
        hipEventCreate(&ln.e0) == hipSuccess && hipEventCreate(&ln.e1) == hipSuccess) {
      ctx->two_lanes = true;
    } else {
      (void)hipGetLastError();
      ln.scratch.release();
    }
  }
  return RL_OK;
}

// how many resident workers the stage's section threads ask the device for (0: trees on the host)
static int expect_workers(const rl_ctx *ctx, const rl_stage_opts &o, const StagePlan &plan, bool gpu_build, bool ages) {
  if (!gpu_build) return 0;
  int cus = 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, o.device) != hipSuccess || cus < 8) cus = 256;
  int workers = stage_worker_goal(cus, plan.nthreads, plan.cap_rows > 0, device_builder_workers_per_cu(ctx->N, ages));
  if (o.workers > 0) workers = o.workers;  // (RELATE_AMD_BUILD_WORKERS overrides either, minmatch_worker.hip)
  (void)device_builder_expect(o.device, ctx->N, workers, ages);
  return workers;
}

// The sections are dealt to the threads longest first: with about two sections per thread (C3: 267 on 134) and
// 228 - 496 trees per section, dealing them in index order left the threads with 500 - 950 trees each, and the
// stage ended on a long tail of a few open sections with most of the tree builder's workers idle (the same deal
// replayed with the measured tree counts: 214 s in index order, 176 s longest first, 174 s perfectly even).  How
// many trees a section needs is not known before its SNPs are mapped; its SNP count is (correlation 0.90).
// The files of a section do not depend on when it is built.
static std::vector<int> deal_sections(const rl_ctx *ctx, int first_section, int last_section, int nthreads) {
  std::vector<int> deal(last_section - first_section + 1);
  for (size_t x = 0; x < deal.size(); x++) deal[x] = first_section + (int)x;
  if (nthreads > 1)
    std::stable_sort(deal.begin(), deal.end(), [&](int a, int b) {
      auto snps = [&](int w) { return (w < ctx->W - 1 ? ctx->wb[w + 1] : ctx->L) - ctx->wb[w]; };
      return snps(a) > snps(b);
    });
  return deal;
}

// What the section threads of one call share, and what each of them does.
struct SectionThreads {
  rl_ctx *ctx;
  const rl_stage_opts &o;
  const StagePlan &plan;
  const std::string chunk_prefix, base;  // <out_dir>/chunk_<c>; the files' name
  const SnpColumns &snps;
  const std::vector<double> &sample_ages;
  const bool from_files, gpu_build;
  const int last_section;
  OptRun *opt;
  FebJob *feb;  // rl_stage_opts.find_equivalent_branches: the stage downstream on the trees while they are in memory (equivalent.cpp)
  const std::vector<int> deal;
  const std::vector<cpu_set_t> groups;
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  std::atomic<int> next{0}, next_slot{0}, first_error{0};
  std::mutex err_mutex;
  std::string first_message;  // (rl_last_error is per thread: the failing worker's text is carried to the caller)
  AdmissionGate gate{ctx, plan, from_files, gpu_build, !sample_ages.empty(), o.device, o.sum_mode, first_error};

  void fail(int code) {
    std::lock_guard<std::mutex> lk(err_mutex);
    int expected = 0;
    if (first_error.compare_exchange_strong(expected, code)) first_message = rl_last_error();
  }

  // one section: its window, its trees (or its count, --mode OptimizeParameters), its files
  int section_turn(rl_treeseq *ts, int turn) {
    const int W = ctx->W, L = ctx->L, section = deal[turn];
    const int start = ctx->wb[section];
    int end = (section < W - 1) ? ctx->wb[section + 1] - 1 : L - 1;
    if (end >= L) end = L - 1;
    const std::string pf = chunk_prefix + "/paint/relate_" + std::to_string(section) + ".bin";
    int r = RL_OK;
    rl_window *win = gate.open(ts, section, pf.c_str(), start, &r);
    const double t_open = seconds_since(t0);
    if (!r && opt) r = optimize_section(ts, start, end, win, *opt);  // (--mode OptimizeParameters: counts, no files)
    else if (!r) r = rl_treeseq_build(ts, start, end, win_matrix, win_advance, win, o.flags, o.fb);
    if (timing_level() >= 1)  // (when the sections start and end: the stage's ramp and tail)
      fprintf(stderr, "[section %d] turn %d, %d SNPs: window open %.1f s after the stage began, trees built at %.1f s\n",
              section, turn, end - start + 1, t_open, seconds_since(t0));
    if (win) gate.close(win);
    if (!r && !opt) {
      const std::string b = chunk_prefix + "/" + base + "_" + std::to_string(section);
      // (fused FindEquivalentBranches: the .anc is written at the end, once, with what that stage carries across)
      r = rl_treeseq_write(ts, feb ? nullptr : (b + ".anc").c_str(), (b + ".mut").c_str());
      if (!r && feb) r = feb_job_add_section(feb, section, ts->trees);
    }
    if (!r && !opt) {
      std::cerr << "[" << section << "/" << last_section << "]\r";
      std::cerr.flush();
    }
    return r;
  }

  void thread_main() {
    PinnedToGroup pin(groups, next_slot);
    // (the panel is the context's, immutable for the stage: a copy per section thread would be 0.3 GB each at C3)
    rl_treeseq *ts = treeseq_borrowing(ctx->N, ctx->L, ctx->bits.data(), ctx->row_words, ctx->rpos.data(), snps.bp.data(),
                                       snps.state.data(), ctx->theta);
    if (!ts) return fail(RL_EINVAL);
    if (!sample_ages.empty()) rl_treeseq_set_sample_ages(ts, sample_ages.data(), (int)sample_ages.size());
    if (gpu_build) {
      rl_treeseq_set_build_device(ts, o.device);
      if (ctx->nloc == ctx->N) {
        rl_treeseq_set_device_matrix(ts, win_matrix_dev);
        rl_treeseq_set_device_matrix_ex(ts, win_matrix_dev_ex);
      }
    }
    for (;;) {
      const int turn = next.fetch_add(1);
      if (turn >= (int)deal.size() || first_error.load()) break;
      if (int r = section_turn(ts, turn)) {
        fail(r);
        break;
      }
    }
    rl_treeseq_destroy(ts);
  }

  void run() {
    if (plan.nthreads <= 1) return thread_main();
    std::vector<std::thread> th;
    for (int t = 0; t < plan.nthreads; t++) th.emplace_back([this] { thread_main(); });
    for (auto &x : th) x.join();
  }
};

// The sections [first_section, last_section] of the chunk loaded in ctx: windows from the paint files of the Paint
// stage (from_files) or from the stepping stones the context has just painted, which never leave HBM (the file's
// float / run-length quantisation applied on the device, window.cpp).  Consumes ctx unless `opt` is set.
static int build_sections(rl_ctx *ctx, const char *out_dir, int chunk_index, int first_section, int last_section,
                          const rl_stage_opts &o, bool from_files, OptRun *opt = nullptr) {
  ContextGuard guard{opt ? nullptr : ctx};
  const char *sample_ages_file = (o.sample_ages_path && *o.sample_ages_path) ? o.sample_ages_path : nullptr;
  const auto entry_t0 = std::chrono::steady_clock::now();
  const int W = ctx->W;
  if (first_section >= W) return 1;  // BuildTopology.cpp:45
  last_section = std::min(W - 1, last_section);
  const std::string chunk_prefix = std::string(out_dir) + "/chunk_" + std::to_string(chunk_index);
  std::vector<double> sample_ages;
  if (sample_ages_file) sample_ages = read_sample_ages(sample_ages_file, ctx->N);
  SnpColumns snps(ctx->L);
  if (int rc = snps.read(chunk_prefix)) return rc;
  // rl_stage_opts.find_equivalent_branches: checked before any device or builder set-up
  const bool want_feb = knob("RELATE_AMD_FUSED_FEB", o.find_equivalent_branches, true, 0) != 0;
  if (want_feb && (first_section != 0 || last_section != W - 1 || W < 2)) {
    set_error("find_equivalent_branches needs a call that covers all %d sections of the chunk (and at least two)", W);
    return RL_EINVAL;
  }
  if (!opt) {
    std::cerr << "---------------------------------------------------------" << std::endl;
    std::cerr << "Estimating topologies of AncesTrees in sections " << first_section << "-" << last_section << "..."
              << std::endl;
  }
  if ((!ctx->plan.valid && build_plan(ctx)) || upload_plan(ctx)) return RL_EINVAL;  // (before the section threads open their windows)

  // inputs -> reservations and plan -> the device's workers and the host's helpers
  StageInputs in = stage_inputs(ctx, o, first_section, last_section, from_files);
  StagePlan plan;
  if (int rc = reserve_and_plan(ctx, o, in, plan)) return rc;
  const bool gpu_build = in.gpu_build, ages = !sample_ages.empty();
  const int asked_workers = expect_workers(ctx, o, plan, gpu_build, ages);
  // Host threads left over by the sections help inside each tree build (minmatch.h BuildThreads).  Helpers are the
  // less efficient use of a core (a merge is split 8 ways for a 2.5x shorter build) and a helper that loses its
  // core stalls every merge, so they get a quarter of the physical cores at most: measured on 2 x 64 cores with 8
  // sections open, 4 helpers each finished in 109 s, 8 in 177 s, none in 165 s.
  set_build_threads(std::min(8, std::max(1, host_threads() / (8 * std::max(1, plan.concurrent)))));

  // the section threads
  SectionThreads threads{ctx, o, plan, chunk_prefix, output_base_name(out_dir), snps, sample_ages, from_files, gpu_build,
                         last_section, opt,
                         want_feb ? feb_job_create(ctx->N, W, std::max(4, std::min(32, host_threads() / 8))) : nullptr,
                         deal_sections(ctx, first_section, last_section, plan.nthreads), cache_groups(o.pin_threads)};
  if (timing_level() >= 1)
    fprintf(stderr, "[stage] set-up before the section threads (plan, reservations) %.3f s\n",
            std::chrono::duration<double>(threads.t0 - entry_t0).count());
  threads.run();

  // epilogue
  if (gpu_build) (void)device_builder_expect(o.device, ctx->N, 0, ages);
  int rc = threads.first_error.load();
  if (rc) set_error("%s", threads.first_message.c_str());
  if (FebJob *feb = threads.feb) {
    if (!rc) rc = feb_job_finish(feb, chunk_prefix + "/" + threads.base);
    feb_job_destroy(feb);
    // (as rl_stage_find_equivalent_branches: the last stage that reads chunk_<c>.bits removes it)
    if (!rc) (void)remove((chunk_prefix + ".bits").c_str());
  }
  if (timing_level() >= 1)
    fprintf(stderr, "[stage] sections %d..%d on %d threads, up to %d open at once, %lld of at most %.0f posterior rows "
            "resident per window, %lld RePaint launches (%.1f s on the device), %s tree builder (%d workers asked for), %.1f s\n",
            first_section, last_section, plan.nthreads, threads.gate.most_open_at_once(),
            plan.cap_rows > 0 ? plan.cap_rows : (long long)plan.max_rows, plan.max_rows, ctx->repaint_launches.load(),
            1e-6 * (double)ctx->repaint_us.load(), gpu_build ? "GPU" : "host", asked_workers, seconds_since(threads.t0));
  const auto destroy_t0 = std::chrono::steady_clock::now();
  guard.release();
  if (timing_level() >= 1)
    fprintf(stderr, "[stage] context released in %.3f s\n", seconds_since(destroy_t0));
  if (!rc && !opt) {
    rusage usage;
    getrusage(RUSAGE_SELF, &usage);
    std::cerr << "CPU Time spent: " << usage.ru_utime.tv_sec << "." << std::setfill('0') << std::setw(6)
              << usage.ru_utime.tv_usec << "s; Max Memory usage: " << usage.ru_maxrss / 1000.0 << "Mb."
              << std::endl;
    std::cerr << "---------------------------------------------------------" << std::endl << std::endl;
  }
  return rc;
}

extern "C" {

int rl_debug_stage_worker_goal(int cus, int open_sections, int bounded_windows, int workers_per_cu) {
  return rl::stage_worker_goal(cus, open_sections, bounded_windows != 0, workers_per_cu);
}

int rl_debug_stage_plan(int N, int nloc, int S, int waves, const double *rows_of, int num_windows, int first_section,
                        int last_section, int stones_per_window, int gpu_build, int room_known, double room, int host_threads,
                        int window_rows_set, long long window_rows, long long window_parts, int section_threads_set,
                        long long section_threads, long long repaint_lanes, int probe_section, long long *ints_out,
                        double *doubles_out) {
  if (N < 2 || nloc < 1 || S < 1 || waves < 1 || !rows_of || first_section < 0 || last_section < first_section ||
      last_section >= num_windows || probe_section < first_section || probe_section > last_section || !ints_out ||
      !doubles_out) {
    set_error("rl_debug_stage_plan: bad arguments");
    return RL_EINVAL;
  }
  StageInputs in;
  in.N = N;
  in.nloc = nloc;
  in.S = S;
  in.waves = waves;
  in.first_section = first_section;
  in.last_section = last_section;
  in.rows_of.assign(num_windows, 0.0);
  for (int w = first_section; w <= last_section; w++) {
    in.rows_of[w] = rows_of[w];
    in.max_rows = std::max(in.max_rows, rows_of[w]);
  }
  in.stones_per_window = stones_per_window != 0;
  in.gpu_build = gpu_build != 0;
  in.room_known = room_known != 0;
  in.room = room;
  in.host_threads = host_threads;
  in.window_rows_set = window_rows_set != 0;
  in.window_rows = window_rows;
  in.window_parts = window_parts;
  in.section_threads_set = section_threads_set != 0;
  in.section_threads = section_threads;
  in.repaint_lanes = repaint_lanes;
  in.repaint_checkpoint = REPAINT_CHECKPOINT;
  in.repaint_side = REPAINT_SIDE;
  const StagePlan p = plan_sections(in);
  const long long ints[6] = {p.nthreads, p.concurrent, p.cap_rows, p.wants_second_lane ? 1 : 0,
                             (long long)p.lane2_scratch_bytes, (long long)p.min_block(probe_section)};
  const double doubles[6] = {p.max_rows, p.row_bytes, p.fixed_bytes, p.builder_bytes, p.bstate_bytes,
                             p.window_bytes(probe_section)};
  memcpy(ints_out, ints, sizeof ints);
  memcpy(doubles_out, doubles, sizeof doubles);
  return RL_OK;
}

void rl_stage_opts_init(rl_stage_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->size = sizeof(*o);
  o->sum_mode = RL_SUM_EXACT;
  o->theta = 0.001;
  o->rho = 1.0;
  o->gpu_build = -1;
  o->pin_threads = -1;
  o->paint_windows = -1;
}

// the caller's struct, whatever its age: fields past its `size` keep their defaults
// (a struct that never went through rl_stage_opts_init -- size 0, or a size no version of the header ever had -- is
//  refused: silently running with the defaults instead of the caller's options is the worse answer)
int rl_internal_resolve_opts(const rl_stage_opts *in, rl_stage_opts *out) {
  rl_stage_opts_init(out);
  if (!in) return RL_OK;
  if (in->size < 2 * sizeof(size_t) || in->size > 4096 || in->size % sizeof(int) != 0) {
    set_error("rl_stage_opts.size = %zu: initialise the struct with rl_stage_opts_init()", in->size);
    return RL_EINVAL;
  }
  memcpy(out, in, std::min(in->size, sizeof(*out)));
  out->size = sizeof(*out);
  return RL_OK;
}

int rl_stage_build_topology_ex(const char *out_dir, int chunk_index, int first_section, int last_section,
                               const rl_stage_opts *opts) {
  if (!out_dir) return RL_EINVAL;
  rl_stage_opts o;
  if (int orc = rl_internal_resolve_opts(opts, &o)) return orc;
  rl_ctx *ctx = rl_create(o.device);
  if (!ctx) return RL_ENODEVICE;
  int rc = rl_load_chunk(ctx, out_dir, chunk_index);
  if (!rc && o.use_painting) rc = rl_set_painting(ctx, o.theta, o.rho);
  if (rc) {
    rl_destroy(ctx);
    return rc;
  }
  return build_sections(ctx, out_dir, chunk_index, first_section, last_section, o, true);
}

// (the positional form; --sample_ages through the deprecated process-wide rl_stage_set_sample_ages)
static rl_stage_opts positional_opts(int use_painting, double theta, double rho, int flags, int fb, int sum_mode,
                                     int device) {
  rl_stage_opts o;
  rl_stage_opts_init(&o);
  o.use_painting = use_painting;
  o.theta = theta;
  o.rho = rho;
  o.flags = flags;
  o.fb = fb;
  o.sum_mode = sum_mode;
  o.device = device;
  o.sample_ages_path = g_stage_sample_ages.empty() ? nullptr : g_stage_sample_ages.c_str();
  return o;
}

int rl_stage_build_topology(const char *out_dir, int chunk_index, int first_section, int last_section,
                            int use_painting, double theta, double rho, int flags, int fb, int sum_mode,
                            int device) {
  const rl_stage_opts o = positional_opts(use_painting, theta, rho, flags, fb, sum_mode, device);
  return rl_stage_build_topology_ex(out_dir, chunk_index, first_section, last_section, &o);
}

int rl_stage_set_sample_ages(const char *file) {
  g_stage_sample_ages = file ? file : "";
  return RL_OK;
}

int rl_stage_paint_build_topology_ex(const char *out_dir, int chunk_index, int first_section, int last_section,
                                     const rl_stage_opts *opts) {
  if (!out_dir) return RL_EINVAL;
  rl_stage_opts o;
  if (int orc = rl_internal_resolve_opts(opts, &o)) return orc;
  const int device = o.device, sum_mode = o.sum_mode, use_painting = o.use_painting;
  const double theta = o.theta, rho = o.rho;
  // RELATE_AMD_TIMING=1: wall-clock of what precedes the sections on stderr
  const bool timing = timing_level() >= 1;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t0 = now();
  auto lap = [&](const char *what) {
    const double t1 = now();
    if (timing) fprintf(stderr, "[fused stage] %-36s %8.3f s\n", what, t1 - t0);
    t0 = t1;
  };
  rl_ctx *ctx = rl_create(device);
  if (!ctx) return RL_ENODEVICE;
  lap("device context");
  int rc = rl_load_chunk(ctx, out_dir, chunk_index);
  lap("read chunk files");
  if (!rc && use_painting) rc = rl_set_painting(ctx, theta, rho);
  // rl_stage_opts.paint_windows: a section reads its own window's stones alone (anc_builder.cpp:49-78), so a call for
  // sections a .. b paints windows a .. b -- the passes stop at the range's last stone, the stones take (b - a + 1) / W
  // of the memory (and of the HBM the admission of build_sections finds free, or of pinned host memory at config #5).
  // (ranges build_sections refuses or empties -- first_section >= W, :45 -- are left to it; fused
  // FindEquivalentBranches covers all sections anyway)
  if (!rc && o.paint_windows != 0) {
    const int w_last = std::min(last_section, ctx->W - 1);
    if (first_section >= 0 && first_section <= w_last) rc = rl_set_window_range(ctx, first_section, w_last);
  }
  if (!rc) {
    std::cerr << "---------------------------------------------------------" << std::endl;
    std::cerr << "Painting sequences (stepping stones stay on the device)..." << std::endl;
    rc = rl_paint(ctx, sum_mode, nullptr);
  }
  lap("plan + uploads + masks + paint kernels");
  if (!rc && timing)
    fprintf(stderr, "[fused stage] windows %d-%d of %d painted in %.1f ms: %lld forward + %lld backward steps, %.3f GB of "
            "stones in %s\n", ctx->w_first, ctx->w_last, ctx->W, ctx->ms_paint, ctx->acc_fwd, ctx->acc_bwd,
            1e-9 * (double)ctx->acc_bytes, ctx->h_alpha ? "pinned host memory" : "HBM");
  // RELATE_AMD_PARK_STONES=1: the stones to pinned host memory, their HBM to the sections' windows -- for chunks that
  // would not fit otherwise; at C3 (53 GB of stones) it opens 112 sections instead of 91 and the chunk takes 330 s
  // instead of 291 s: past ~90 trees in flight the build kernels slow each other down
  if (!rc && knob("RELATE_AMD_PARK_STONES", o.park_stones, true, 0) != 0) rc = rl_park_stones(ctx);
  if (!rc) ctx->stones_disposable = true;  // (nobody writes paint files from this context: the windows may edit them)
  if (!rc) {  // (the Paint stage makes this directory for its files; the trees go there)
    const std::string cdir = std::string(out_dir) + "/chunk_" + std::to_string(chunk_index);
    if (mkdir(cdir.c_str(), 0777) != 0 && errno != EEXIST) {
      set_error("cannot create %s", cdir.c_str());
      rc = RL_EIO;
    }
  }
  if (rc) {
    rl_destroy(ctx);
    return rc;
  }
  return build_sections(ctx, out_dir, chunk_index, first_section, last_section, o, false);
}

int rl_stage_paint_build_topology(const char *out_dir, int chunk_index, int first_section, int last_section,
                                  int use_painting, double theta, double rho, int flags, int fb, int sum_mode,
                                  int device) {
  const rl_stage_opts o = positional_opts(use_painting, theta, rho, flags, fb, sum_mode, device);
  return rl_stage_paint_build_topology_ex(out_dir, chunk_index, first_section, last_section, &o);
}

// ---- `--mode OptimizeParameters` (pipeline/OptimizeParameters.cpp:22-206) ------------------------------------------
// (float arguments as the reference's grid holds them, :76-77; data.theta / data.r are doubles made from them, :151-155)
static float opt_log_ratio(float theta) {
  const double th = theta, nth = 1.0 - th;  // :151-152
  return (float)std::log(th / nth);          // anc_builder.cpp:852
}

int rl_optimize_section(rl_ctx *ctx, int section, float theta, float rec_factor, int *count) {
  if (!ctx || !count || !ctx->have_chunk || section < 0 || section >= ctx->W) {
    set_error("rl_optimize_section: bad arguments");
    return RL_EINVAL;
  }
  if (!ctx->painted) {
    set_error("rl_optimize_section: rl_paint has not run (the grid point re-paints from the stepping stones in HBM)");
    return RL_ESTATE;
  }
  if (!(theta > 0.0f && theta < 1.0f) || !(rec_factor > 0.0f)) {
    set_error("rl_optimize_section: theta has to be in (0,1) and the recombination factor positive");
    return RL_EINVAL;
  }
  int rc = RL_OK;
  if (ctx->theta != (double)theta || ctx->rho != (double)rec_factor) rc = replan_painting(ctx, theta, rec_factor);
  if (rc) return rc;
  const int L = ctx->L, start = ctx->wb[section];
  const int end = std::min(L - 1, (section < ctx->W - 1 ? ctx->wb[section + 1] : L) - 1);
  const SnpColumns snps(L);  // (neither is read by this mode)
  rl_treeseq *ts = treeseq_borrowing(ctx->N, L, ctx->bits.data(), ctx->row_words, ctx->rpos.data(), snps.bp.data(),
                                     snps.state.data(), ctx->theta);
  if (knob("RELATE_AMD_GPU_BUILD", 1, true, 1) != 0 && ctx->nloc == ctx->N) {
    rl_treeseq_set_build_device(ts, ctx->device);
    rl_treeseq_set_device_matrix(ts, win_matrix_dev);
  }
  rl_window *win = rl_window_open(ctx, section, nullptr, start, ctx->paint_mode >= 0 ? ctx->paint_mode : RL_SUM_EXACT, nullptr);
  OptRun run;
  run.log_ratio = opt_log_ratio(theta);
  rc = win ? optimize_section(ts, start, end, win, run) : RL_EHIP;
  if (win) rl_window_close(win);
  rl_treeseq_destroy(ts);
  if (!rc) *count = (int)run.count.load();
  if (!rc && timing_level() >= 1)
    fprintf(stderr, "[optimize] section %d: %lld trees (%lld on the GPU, %lld on the host)\n", section, run.trees.load(),
            run.gpu_trees.load(), run.host_trees.load());
  return rc;
}

int rl_stage_optimize_parameters(const char *out_dir, int chunk_index, const float *theta, int n_theta,
                                 const float *factor, int n_factor, const rl_stage_opts *opts, int *counts) {
  if (!out_dir || !theta || !factor || !counts || n_theta < 1 || n_factor < 1) {
    set_error("rl_stage_optimize_parameters: bad arguments");
    return RL_EINVAL;
  }
  for (int i = 0; i < n_theta; i++)
    if (!(theta[i] > 0.0f && theta[i] < 1.0f)) {
      set_error("theta value has to be in (0,1)");  // OptimizeParameters.cpp:92-95
      return RL_EINVAL;
    }
  for (int j = 0; j < n_factor; j++)
    if (!(factor[j] > 0.0f)) {
      set_error("rho value has to be positive");  // :103-106
      return RL_EINVAL;
    }
  rl_stage_opts o;
  if (int orc = rl_internal_resolve_opts(opts, &o)) return orc;
  o.find_equivalent_branches = 0;
  o.sample_ages_path = nullptr;  // (the mode builds without sample ages: `sample_ages` of a fresh AncesTreeBuilder, :163)
  rl_ctx *ctx = rl_create(o.device);
  if (!ctx) return RL_ENODEVICE;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = rl_load_chunk(ctx, out_dir, chunk_index);
  // The stepping stones of EVERY grid point are painted with the chunk's stored recombination distances and the default
  // theta -- or --painting's, Paint.cpp:38-61 --: Paint(options, c) at OptimizeParameters.cpp:159 reads the chunk files
  // into a Data of its own (Paint.cpp:35), the grid's data.theta / data.r (:151-157) never reach it.  So the stones are
  // painted ONCE per chunk and stay in HBM, as in the fused stage; a grid point rebuilds the RePaint plan only.
  if (!rc && o.use_painting) rc = rl_set_painting(ctx, o.theta, o.rho);
  if (!rc) rc = rl_paint(ctx, o.sum_mode, nullptr);
  const auto tpaint1 = std::chrono::steady_clock::now();
  if (!rc) ctx->stones_disposable = true;  // (no paint files from this context: a window quantises its slice once, in place)
  long long trees = 0, gpu_trees = 0, host_trees = 0;
  double t_replan = 0.0;
  const double t_paint = std::chrono::duration<double>(tpaint1 - t0).count();
  for (int i = 0; i < n_theta && !rc; i++)
    for (int j = 0; j < n_factor && !rc; j++) {
      // the grid point's r is the STORED r times the factor (:146, :155), whatever --painting did to the stones' r
      // (the reference's Paint prints its banner for every grid point, Paint.cpp:63-64)
      std::cerr << "---------------------------------------------------------" << std::endl;
      std::cerr << "Painting sequences..." << std::endl;
      const auto tp = std::chrono::steady_clock::now();
      rc = replan_painting(ctx, theta[i], factor[j]);
      t_replan += seconds_since(tp);
      OptRun run;
      run.log_ratio = opt_log_ratio(theta[i]);
      if (!rc) rc = build_sections(ctx, out_dir, chunk_index, 0, ctx->W - 1, o, false, &run);
      if (!rc) counts[(size_t)i * n_factor + j] += (int)run.count.load();
      trees += run.trees.load();
      gpu_trees += run.gpu_trees.load();
      host_trees += run.host_trees.load();
    }
  if (timing_level() >= 1) {
    const double sec = seconds_since(t0);
    fprintf(stderr, "[optimize] chunk %d: %d grid points, %lld trees (%lld on the GPU, %lld on the host) in %.2f s: %.0f "
            "trees per second; chunk files + Paint %.2f s, plan per grid point %.3f s\n", chunk_index, n_theta * n_factor,
            trees, gpu_trees, host_trees, sec, (double)trees / std::max(sec, 1e-9), t_paint, t_replan / (n_theta * n_factor));
  }
  rl_destroy(ctx);
  return rc;
}

}  // extern "C"

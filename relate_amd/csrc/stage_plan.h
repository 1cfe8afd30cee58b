// stage_plan.h -- how a BuildTopology stage sizes itself against HBM: section threads, rows a window keeps, the second
// RePaint lane.  A pure function of numbers -- no device, no environment, no context -- so that a CPU test can hold it
// to its decisions (rl_debug_stage_plan, tests/test_stage_plan_cpu.py).  stage.cpp gathers the inputs and acts on the plan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace rl {

struct StageInputs {
  int N = 0, nloc = 0;    // haplotypes; targets of this context
  int S = 0, waves = 1;   // register tile and wavefronts per target (a posterior row is S * 64 * waves floats)
  int first_section = 0, last_section = 0;
  std::vector<double> rows_of;  // [W] posterior rows of each section's window, summed over the targets (first .. last filled)
  double max_rows = 0;          // the largest of them
  bool stones_per_window = false;  // a window holds decoded stones of its own: a stage from paint files, or stones parked in host memory
  bool gpu_build = false;          // trees on the device (RELATE_AMD_GPU_BUILD / rl_stage_opts, resolved)
  bool room_known = false;         // hipMemGetInfo answered ...
  double room = 0.0;               // ... 0.9 of the free HBM, after the builders' pools and RePaint's strips
  int host_threads = 1;            // this rank's share
  // the knobs, resolved once by the caller (environment, then rl_stage_opts, then fallback)
  bool window_rows_set = false;  // RELATE_AMD_WINDOW_ROWS in the environment or a non-zero rl_stage_opts.window_rows
  long long window_rows = 0;     // (< 0: all of them)
  long long window_parts = 32;
  bool section_threads_set = false;
  long long section_threads = 0;
  long long repaint_lanes = 1;
  int repaint_checkpoint = 0, repaint_side = 0;  // device_types.h REPAINT_CHECKPOINT, REPAINT_SIDE
};

struct StagePlan {
  int nthreads = 1;        // section threads
  int concurrent = 1;      // sections the estimate sees open at once
  long long cap_rows = 0;  // posterior rows a window keeps resident; 0: all
  double max_rows = 0, row_bytes = 0, fixed_bytes = 0, builder_bytes = 0, bstate_bytes = 0;
  bool wants_second_lane = false;
  size_t lane2_scratch_bytes = 0;  // the second lane's strips
  std::vector<double> rows_of;

  bool bounded(int w) const { return cap_rows > 0 && cap_rows < rows_of[w]; }
  double kept_rows(int w) const { return cap_rows > 0 ? std::min(rows_of[w], (double)cap_rows) : rows_of[w]; }
  // HBM of section w's open window
  double window_bytes(int w) const { return kept_rows(w) * row_bytes + fixed_bytes + (bounded(w) ? bstate_bytes : 0.0); }
  // cache_alloc hands out whole cached blocks: of what the cache holds only blocks that can take one of the
  // window's large buffers (a kept state of a bounded window, or else its rows) count as room
  size_t min_block(int w) const {
    return (size_t)(0.85 * (bounded(w) ? std::min(kept_rows(w) * row_bytes, bstate_bytes / 4.0) : kept_rows(w) * row_bytes));
  }
};

// How many sections are open at once is bounded by host threads and by HBM: a window's posterior rows (sum_n D_n
// rows of S*64*waves floats, 20 GB at N = 5000) stay resident while its trees are built.  When the sections the
// host could work on do not fit, every window keeps a part of its rows and repaints as its builder moves on
// (rl_window_open_bounded; RELATE_AMD_WINDOW_ROWS sets the rows per window by hand).  Every open is admitted
// against the HBM that is free at that moment (window_bytes); the estimate here sizes the thread pools.
inline StagePlan plan_sections(const StageInputs &in) {
  StagePlan p;
  p.rows_of = in.rows_of;
  p.max_rows = in.max_rows;
  const int nsec = in.last_section - in.first_section + 1;
  p.row_bytes = 4.0 * in.S * 64 * in.waves;
  // Next to its rows a window holds cursors and small per-target arrays, a stage from paint files also the decoded
  // stones (2 N^2 floats; the fused stage re-paints from the context's own); a tree builder on the device keeps the
  // woven float4 matrix of the build (16 N^2 B, minmatch_builder.hip) -- the row-major matrices of a tree and the
  // symmetric matrix of the fallback come from pools of the device, counted once.  RePaint's strips are one buffer
  // of the context (reserved by the caller).
  const double NN = (double)in.N * (in.N + 64.0);
  p.builder_bytes = in.gpu_build ? 17.0 * NN : 0.0;  // (allocated once per section thread, kept)
  p.fixed_bytes = 4.0 * p.max_rows + 48e6 + (in.stones_per_window ? 8.0 * in.N * in.nloc : 0.0) +
                  (in.gpu_build && in.nloc == in.N ? 0.0 : 4.0 * in.N * in.nloc);
  // (a bounded window also keeps one state of RePaint's backward pass per target, doubles: window.cpp)
  p.bstate_bytes = 2.0 * (2.0 * p.row_bytes * in.nloc + 24.0 * in.nloc);  // (one of each pass)
  // (section threads of device builds mostly wait for their tree: as many as there are CUs to build on)
  p.nthreads = in.gpu_build ? 256 : std::max(1, std::min(in.host_threads / 2, 64));  // (host_threads: this rank's share)
  p.nthreads = std::max(1, (int)(in.section_threads_set ? in.section_threads : p.nthreads));
  p.nthreads = std::min(p.nthreads, nsec);
  p.concurrent = p.nthreads;
  if (in.window_rows_set) {  // (rows per window by hand; < 0 in the struct: all of them)
    p.cap_rows = std::max(0LL, in.window_rows);
  } else if (in.room_known) {
    // The trees of different sections are what fills the chip (a workgroup per tree), so as many sections as HBM
    // holds should be open -- but a window that keeps 1/P of its rows runs RePaint P times, about half a window's
    // pass each time, on the CUs the builders leave free: not below a P-th of the largest window,
    // P <= RELATE_AMD_WINDOW_PARTS (32).  And the sections go in WAVES of whatever is open at once: 267 sections
    // 112 at a time are three waves, the last one a third full; 134 at a time are two full ones.  So: the fewest
    // waves the memory allows at P_max, the sections spread evenly over them, and the smallest P that opens
    // that many (C3: 2 waves of 134, P = 20: 234 s -> see DESIGN_NOTES.md 6).
    const int parts_max = std::max(1, (int)in.window_parts);
    auto fits = [&](int parts) {
      return (int)(in.room / (p.max_rows / parts * p.row_bytes + p.fixed_bytes + p.builder_bytes + (parts > 1 ? p.bstate_bytes : 0.0)));
    };
    const int most = std::max(1, std::min(p.nthreads, fits(parts_max)));
    const int waves = (nsec + most - 1) / most;
    p.nthreads = std::min(p.nthreads, (nsec + waves - 1) / waves);
    int parts = 1;
    while (parts < parts_max && fits(parts) < p.nthreads) parts++;
    if (parts > 1) p.cap_rows = (long long)std::max({p.max_rows / parts, 3.0 * in.nloc + 64.0});
  }
  // A SECOND lane of RePaint launches for bounded windows (common.h; RELATE_AMD_REPAINT_LANES / rl_stage_opts decide
  // otherwise): a launch is a forward and a backward kernel of one workgroup per target, each as long as its longest
  // target, on the CUs the tree builder's workers leave -- two windows' launches side by side fill each other's
  // tails, and no section waits for its turn behind a hundred others.  Round 3 sized its strips like the first
  // lane's, for a window's first whole pass (7 GB at C3: 45 sections' worth of rows); a partial launch addresses its
  // strips compactly (window.cpp place_rows) and the second lane takes partial launches only: kept rows / 6 + 2 per
  // target rows of doubles + the side records, 0.7 GB.  NOT the default all the same: with all 134 sections open the
  // two lanes' launches share the CUs the workers leave and each takes as much longer as it overlaps (C3, 104
  // workers: 162.6 s with two lanes, 161.9 s with one; 116 workers 166.5 s; 128 workers 219 s,
  // profiles/r04_c3_workers.json) -- RePaint is bound by the CUs it gets, not by its queue.
  if (in.last_section > in.first_section && p.cap_rows > 0 && in.repaint_lanes == 2) {
    p.wants_second_lane = true;
    const size_t row_doubles = (size_t)in.S * 64 * in.waves;
    p.lane2_scratch_bytes = (size_t)(((double)p.cap_rows / in.repaint_checkpoint + 2.0 * in.nloc + 64.0) * (double)row_doubles +
                                     p.max_rows * in.repaint_side) * sizeof(double);
  }
  if (in.room_known) {
    const double per_window = p.window_bytes((in.first_section + in.last_section) / 2) + p.builder_bytes;
    p.concurrent = std::max(1, std::min(p.nthreads, (int)(in.room / std::max(per_window, 1.0))));
    p.nthreads = std::min(p.nthreads, p.concurrent);
  }
  return p;
}

}  // namespace rl

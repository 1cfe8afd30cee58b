// selection.cpp -- Selection, host only (include/relate_amd.h has the definition; the reference:
// include/evaluate/selection/RelateSelection.cpp:136-178 log_pvalue, :190-328 Selection).
//
// out.freq + out.lin of the mode Frequency (this library's or the reference's) -> out.sele: per SNP and epoch boundary
// the log10 p-value of seeing the derived allele on fN of N lineages today given it was on fk of k lineages at the
// boundary.  A cell is up to N - k iterations of log and exp in the float / double mix of the reference, with a table
// of log(k!) in floats; its bytes are libm's, so the mode stays on the host.  The rows are independent: they are
// computed on RELATE_AMD_THREADS threads and written in order.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "anc_text.h"
#include "common.h"

namespace rl {

namespace {

const char *const kMode = "Selection";

// logFactorial (:44-58): logF[k] = log(k!) accumulated in floats, the logarithm in double
std::vector<float> log_factorials(int N) {
  std::vector<float> logF((size_t)N + 1);
  logF[0] = 0;
  for (int k = 1; k <= N; k++) logF[k] = logF[k - 1] + std::log(k);
  return logF;
}

// log_pvalue (:136-178), its promotions kept.  The reference's asserts and the bounds of its table are *bad
bool log_pvalue(int k, float fk, int N, float fN, const std::vector<float> &logF, float *out, const char **bad) {
  const float log_10 = std::log(10);
  float logp = 0.0, px = 0.0;
  *out = 1.0;
  if (fk < 2) return true;
  if (k == -1) return true;
  const char *failed = !(fN < N) ? "fN < N" : !(fk < k) ? "fk < k" : !(fN > 0) ? "fN > 0" : nullptr;
  const float at[9] = {N - fN - 1, k - fk - 1, N - k + fk - fN, fN - 1, fk - 1, fN - fk, (float)(N - 1), (float)(k - 1), (float)(N - k)};
  for (int i = 0; i < 9 && !failed; i++)
    if (!(at[i] >= 0.0f && at[i] <= (float)N)) failed = "0 <= index of log(k!) <= N";
  if (failed) {
    *bad = failed;
    return false;
  }
  const auto F = [&](float i) { return logF[(size_t)i]; };
  px = F(at[0]) - F(at[1]) - F(at[2]);
  px += F(at[3]) - F(at[4]) - F(at[5]);
  px -= F(at[6]) - F(at[7]) - F(at[8]);
  logp = px;
  float x = fN - fk;
  const int y = N - k, c = N - 1;
  int var;
  while (x < N - k) {
    var = fk + x;
    px += std::log((y - x) / (x + 1.0) * var / ((float)(c - var)));
    logp = std::log(1.0 + std::exp(px - logp)) + logp;  // (the float overload, as the reference's unqualified call resolves)
    x++;
  }
  if (logp > 0.0) logp = 0.0;
  logp /= log_10;
  *out = logp;
  return true;
}

// operator<< of a float with the stream's defaults
void append_float(std::string &s, float v) {
  char buf[48];
  snprintf(buf, sizeof buf, "%g ", (double)v);
  s += buf;
}

// the numbers of a row behind `pos rs_id`, as operator>> into a float reads them
bool row_numbers(const std::string &line, std::string *pos, std::string *rs_id, std::vector<float> &v) {
  std::istringstream s(line);
  if (!(s >> *pos >> *rs_id)) return false;
  v.clear();
  for (float x; s >> x;) v.push_back(x);
  return true;
}

}  // namespace
}  // namespace rl

using namespace rl;

extern "C" int rl_selection_logp(int k, float fk, int N, float fN, float *logp) {
  if (!logp) return null_args("rl_selection_logp");
  if (N < 1 || N > (1 << 26)) {
    set_error("rl_selection_logp: N=%d lineages", N);
    return RL_EINVAL;
  }
  static thread_local std::vector<float> logF;  // (a caller asks for many cells of one N)
  if ((int)logF.size() != N + 1) logF = log_factorials(N);
  const char *bad = nullptr;
  if (!log_pvalue(k, fk, N, fN, logF, logp, &bad)) {
    set_error("rl_selection_logp: k=%d fk=%g N=%d fN=%g: the reference's check `%s` fails", k, (double)fk, N, (double)fN, bad);
    return RL_EINVAL;
  }
  return RL_OK;
}

extern "C" int rl_selection_files(const char *in_prefix, const char *out_path) {
  if (!in_prefix || !out_path) return null_args("rl_selection_files");
  const std::string fn_freq = std::string(in_prefix) + ".freq", fn_lin = std::string(in_prefix) + ".lin";
  std::ifstream is_freq, is_lin;
  if (const int rc = open_text(kMode, fn_freq, is_freq)) return rc;
  if (const int rc = open_text(kMode, fn_lin, is_lin)) return rc;
  std::string head_freq, head_lin, line;
  getline(is_freq, head_freq);
  getline(is_lin, head_lin);
  std::vector<std::string> freq, lin;
  while (getline(is_freq, line)) freq.push_back(line);
  while (getline(is_lin, line) && lin.size() < freq.size()) lin.push_back(line);
  if (lin.size() != freq.size()) {
    set_error("%s: %s has %zu rows, %s %zu", kMode, fn_freq.c_str(), freq.size(), fn_lin.c_str(), lin.size());
    return RL_EFORMAT;
  }
  std::ofstream os(out_path);
  if (os.fail()) {
    set_error("%s: error while opening file %s", kMode, out_path);
    return RL_EIO;
  }
  os << head_lin << "\n";
  const size_t rows = freq.size();
  // the first row sets the number of cells and N: the lineages at the boundary 0 (:265-275)
  int cells = 0, N = 0;
  if (rows) {
    std::string pos, id;
    std::vector<float> v;
    if (!row_numbers(lin[0], &pos, &id, v) || v.size() < 3 || v.size() - 2 > 4096 || !(v[v.size() - 3] >= 1.0f && v[v.size() - 3] <= (float)(1 << 26))) {
      set_error("%s: %s: the first row is not `pos rs_id`, the lineages per boundary, when_DAF_is_half, when_mutation_has_freq2", kMode, fn_lin.c_str());
      return RL_EFORMAT;
    }
    cells = (int)v.size() - 2;
    N = (int)v[cells - 1];
  }
  const std::vector<float> logF = log_factorials(N);
  std::vector<std::string> out(rows);
  std::vector<long long> bad_row;
  std::vector<std::string> bad_text;
  const int threads = (int)std::max<size_t>(1, std::min<size_t>((size_t)host_threads(), rows / 64 + 1));
  bad_row.assign(threads, -1);
  bad_text.resize(threads);
  const auto work = [&](int w) {
    std::string pos, id, pos_lin, id_lin;
    std::vector<float> num_freq, num_lin;
    for (size_t r = w; r < rows; r += threads) {
      std::string &o = out[r];
      const auto fail = [&](const std::string &why) {
        if (bad_row[w] < 0) bad_row[w] = (long long)r, bad_text[w] = why;
      };
      if (!row_numbers(freq[r], &pos, &id, num_freq) || !row_numbers(lin[r], &pos_lin, &id_lin, num_lin) ||
          (int)num_freq.size() < cells || (int)num_lin.size() < cells + 2) {
        fail("the row has fewer numbers than the first");
        continue;
      }
      o = pos + " " + id + " ";
      const float fN = num_freq[cells - 1];  // the carriers when all N lineages remain
      if (fN <= 2) {
        for (int i = 0; i < cells; i++) o += "1 ";
        o += "1 1\n";
        continue;
      }
      const char *bad = nullptr;
      float p = 0.0f;
      bool ok = true;
      for (int i = 0; i < cells && ok; i++) {
        ok = log_pvalue((int)num_lin[i], num_freq[i], N, fN, logF, &p, &bad);
        append_float(o, p);
      }
      ok = ok && log_pvalue((int)num_lin[cells], (float)(int)((fN + 1.0) / 2.0), N, fN, logF, &p, &bad);
      append_float(o, p);
      ok = ok && log_pvalue((int)num_lin[cells + 1], 2.0f, N, fN, logF, &p, &bad);
      append_float(o, p);
      o.back() = '\n';
      if (!ok) fail(std::string("the reference's check `") + bad + "` fails");
    }
  };
  std::vector<std::thread> pool;
  for (int w = 1; w < threads; w++) pool.emplace_back(work, w);
  work(0);
  for (std::thread &th : pool) th.join();
  long long first_bad = -1;
  std::string why;
  for (int w = 0; w < threads; w++)
    if (bad_row[w] >= 0 && (first_bad < 0 || bad_row[w] < first_bad)) first_bad = bad_row[w], why = bad_text[w];
  if (first_bad >= 0) {
    set_error("%s: %s, row %lld: %s", kMode, in_prefix, first_bad, why.c_str());
    return RL_EINVAL;
  }
  for (const std::string &o : out) os << o;
  os.close();
  if (os.fail()) {
    set_error("%s: writing %s failed", kMode, out_path);
    return RL_EIO;
  }
  return RL_OK;
}

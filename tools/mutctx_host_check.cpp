// mutctx_host_check.cpp -- the host code of MutationRateWithContext under AddressSanitizer and UBSan, as a program of
// its own (tools/mutctx_host_check.sh builds and runs it on the CPU; it never touches a GPU and is not loaded into
// Python).  Linked with mutctx.cpp, mutrate.cpp and tree_host.cpp; what those ask of the rest of the library is stubbed
// here.
//   mutctx_host_check DIR case[:bins[:years_per_gen[:dist]]] ...
// 1. every case named: DIR/<case>.anc, .mut, _mask.fa, _ancestor.fa (and .dist) through rl_mutctx_anc on the host,
//    rl_mutctx_write, rl_mutctx_read, rl_mutctx_sum of the case with itself and rl_mutctx_finalize;
// 2. a few thousand small inputs from an integer LCG through rl_mutctx_count_bases: sequences around the lengths at
//    which the walk changes phase (0, the first window of 1001, two windows), masks shorter, longer and empty, SNPs
//    at the very ends, position lists with and without extra positions.  A call may succeed or be refused; the
//    counts of one that succeeds are checked against the bases the SNPs can own.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "mutctx.h"
#include "relate_amd.h"

namespace rl {
static std::string g_error;
thread_local unsigned tl_alloc_failures = 0;
void set_error(const char *fmt, ...) {
  char buf[2048];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_error = buf;
}
void *device_cache_alloc(size_t, size_t *) { return nullptr; }
void device_cache_release(void *, size_t) {}
static int no_device() {
  set_error("no device in this program");
  return RL_ENODEVICE;
}
int mutrate_device(const int *, const double *, int, int, const double *, int, int, double *, int *) { return no_device(); }
int mutctx_device_begin(MutctxDevice **, int, const double *, int, int) { return no_device(); }
int mutctx_device_add(MutctxDevice *, const int *, const double *, int, const int *, const uint32_t *, long long, float *, int *) {
  return no_device();
}
int mutctx_device_finish(MutctxDevice *, double *) { return no_device(); }
void mutctx_device_seconds(const MutctxDevice *, double *) {}
void mutctx_device_free(MutctxDevice *) {}
}  // namespace rl

static unsigned g_x = 12345;
static unsigned below(unsigned n) {
  g_x = g_x * 1664525u + 1013904223u;
  return (g_x >> 8) % n;
}

static void write_fasta(const std::string &fn, const std::string &seq) {
  FILE *fp = fopen(fn.c_str(), "w");
  fprintf(fp, ">x\n");
  for (size_t i = 0; i < seq.size(); i += 60) fprintf(fp, "%s\n", seq.substr(i, 60).c_str());
  fclose(fp);
}

static int fail(const char *what, const std::string &detail) {
  fprintf(stderr, "mutctx_host_check: %s: %s\n", what, detail.c_str());
  return 1;
}

int main(int argc, char **argv) {
  if (argc < 2) return fail("usage", "mutctx_host_check DIR case[:bins[:years_per_gen[:dist]]] ...");
  const std::string dir = argv[1];
  for (int a = 2; a < argc; a++) {
    std::vector<std::string> f(1);
    for (const char *p = argv[a]; *p; p++) {
      if (*p == ':') f.emplace_back();
      else f.back() += *p;
    }
    f.resize(4);
    const std::string p = dir + "/" + f[0];
    std::vector<double> ep(4096);
    int E = (int)ep.size();
    if (rl_mutrate_epochs(f[2].empty() ? 28.0f : (float)atof(f[2].c_str()), f[1].empty() ? nullptr : f[1].c_str(), ep.data(), &E))
      return fail("rl_mutrate_epochs", rl::g_error);
    std::vector<double> m((size_t)E * 96), o((size_t)E * 96), m2(m.size()), o2(o.size()), ep2(64);
    long long snps[3];
    if (rl_mutctx_anc((p + ".anc").c_str(), (p + ".mut").c_str(), (p + "_mask.fa").c_str(), (p + "_ancestor.fa").c_str(),
                      f[3].empty() ? nullptr : (p + ".dist").c_str(), ep.data(), E, -1, m.data(), o.data(), snps))
      return fail("rl_mutctx_anc", rl::g_error);
    const std::string out = dir + "/check_" + std::to_string(a);
    int E2 = 64;
    if (rl_mutctx_write((out + "_chr1").c_str(), ep.data(), E, m.data(), o.data()) ||
        rl_mutctx_write((out + "_chr2").c_str(), ep.data(), E, m.data(), o.data()) ||
        rl_mutctx_read((out + "_chr1").c_str(), ep2.data(), &E2, m2.data(), o2.data()) ||
        rl_mutctx_sum(out.c_str(), "1\n2\n", out.c_str()) || rl_mutctx_finalize(out.c_str(), (out + ".rate").c_str()))
      return fail("the .bin files", rl::g_error);
    if (E2 != E || memcmp(m.data(), m2.data(), m.size() * 8) || memcmp(o.data(), o2.data(), o.size() * 8))
      return fail("rl_mutctx_read", "not what rl_mutctx_write wrote");
    if (!rl_mutctx_read((dir + "/none").c_str(), ep2.data(), &E2, m2.data(), o2.data())) return fail("rl_mutctx_read", "read a missing file");
    printf("%s: %lld SNPs, %lld qualifying, %d epochs\n", f[0].c_str(), snps[0], snps[2], E);
  }
  // ---- small inputs
  const std::string fa = dir + "/small_anc.fa", fm = dir + "/small_mask.fa";
  long long accepted = 0, refused = 0, counted = 0;
  const int bases_at[] = {0, 1, 2, 40, 1000, 1001, 1002, 1003, 1100, 2001, 2002, 2003, 2100, 3300};
  for (int round = 0; round < 4000; round++) {
    const int len_a = bases_at[below(14)] + (int)below(3), len_m = below(4) == 0 ? (int)below(30) : bases_at[below(14)] + (int)below(3);
    std::string anc((size_t)len_a, 'A'), mask((size_t)len_m, 'P');
    for (char &c : anc) c = "ACGTacgtNn-"[below(11)];
    const int holes = (int)below(4);
    for (int h = 0; h < holes && len_m; h++) {
      const size_t at = below(len_m), ln = below(4) == 0 ? 1500 : 1 + below(40);
      for (size_t i = at; i < at + ln && i < mask.size(); i++) mask[i] = "NnCp"[below(4)];
    }
    write_fasta(fa, anc);
    write_fasta(fm, mask);
    const int S = std::max(len_a, len_m), L = 1 + (int)below(6);
    std::vector<int> snp_pos, pos;
    std::vector<unsigned char> one;
    int at = below(3) == 0 ? 0 : (int)below(S + 2);
    for (int s = 0; s < L; s++) {
      snp_pos.push_back(at);
      one.push_back(below(5) != 0);
      at += below(4) == 0 ? (S > at ? S - at - (int)below(3) : 1) : 1 + (int)below(S / 2 + 2);
    }
    const int style = (int)below(4);  // the .mut's own positions | with extra ones | one short | one extra behind
    for (int s = 0; s < L; s++) {
      if (style == 1 && below(2)) pos.push_back(snp_pos[s] > 0 ? snp_pos[s] - (int)below(2) : 0);
      if (!(style == 2 && s == L - 1 && L > 1)) pos.push_back(snp_pos[s]);
    }
    if (style == 3) pos.push_back(snp_pos.back() + 1 + (int)below(50));
    for (size_t j = 1; j < pos.size(); j++)
      if (pos[j] < pos[j - 1]) pos[j] = pos[j - 1];
    std::vector<uint32_t> counts((size_t)L * 96, 0xdeadbeefu);
    const int rc = rl_mutctx_count_bases(fa.c_str(), fm.c_str(), pos.data(), (long long)pos.size(), snp_pos.data(), one.data(), L, counts.data());
    if (rc) {
      if (rl::g_error.empty()) return fail("rl_mutctx_count_bases", "refused without a message");
      refused++;
      continue;
    }
    accepted++;
    for (int s = 0; s < L; s++) {
      unsigned long long row = 0;
      for (int c = 0; c < 96; c++) row += counts[(size_t)s * 96 + c];
      counted += row;
      if (row % 3 || row > 3ull * (unsigned long long)S || (!one[s] && row) || (s == L - 1 && row))
        return fail("rl_mutctx_count_bases", "round " + std::to_string(round) + ": SNP " + std::to_string(s) + " counts " + std::to_string(row) + " bases x 3");
    }
  }
  printf("small inputs: %lld accepted, %lld refused, %lld bases counted\n", accepted, refused, counted / 3);
  if (accepted < 200 || refused < 200 || counted == 0) return fail("small inputs", "too few calls of one kind to mean anything");
  return 0;
}

// main.cpp -- `Relate` drop-in for the stages of this path (plus their input producer):
//   Relate --mode FindEquivalentBranches --chunk_index c -o out
//   Relate --mode MakeChunks    --haps x.haps --sample x.sample --map x.map [--memory 5] [--dist f] [--transversion] -o out
//   Relate --mode Paint         --chunk_index c -o out [--painting theta,rho]
//   Relate --mode BuildTopology --chunk_index c --first_section a --last_section b -o out
//          [--painting theta,rho] [--seed s] [--fb x] [--no_consistency]
//   Relate --mode OptimizeParameters --haps x.haps --sample x.sample --map x.map [--memory 5] [--dist f]
//          [-i grid.txt] [--painting theta,rho] -o out      (writes out.opt: `theta factor not-mapping-SNPs` per pair)
//   Relate --mode CompareTopology -i a.anc,b.anc [-o out] [--device d]
//          (no reference counterpart: the clade distance of the two files' trees position by position, the summary on
//           stdout as `key value` lines; with -o, out.cmp: `snp_begin snp_end treeA treeB d` per interval; --device -1:
//           on the host)
//   Relate --mode PairwiseCoalescence -i a.anc[,b.anc,...] -o out [--metric size|time] [--device d]
//   Relate --mode CopyingMatrix --chunk_index c -o out [--first_section a --last_section b] [--painting t,r]
//          [--sum_mode m] [--device d]
//          (no reference counterpart: for every pair of haplotypes the size (leaves below) or the time (height) of
//           their most recent common ancestor, SNP-weighted over the files' trees; out.pwc: int32 N, int32 metric
//           (0 size, 1 time), int64 W (SNPs), then the N x N sums (uint64 / double) row-major; the summary on stdout
//           as `key value` lines; --device -1: on the host)
//   Relate --mode CoalescentRateForSection -i prefix -o out [--bins lower,upper,step] [--years_per_gen g] [--device d]
//          (RelateCoalescentRate --mode CoalescentRateForSection of the reference: reads prefix.anc (text) and
//           prefix.mut, writes out.bin, the reference's bytes; --device -1: on the host; --mask, --dist, .gz inputs
//           and sample ages are refused)
//   Relate --mode FinalizePopulationSize -o out [--poplabels f]
//          (RelateCoalescentRate --mode FinalizePopulationSize: out.bin -> out.coal; --poplabels hap is refused)
//   Relate --mode Frequency -i prefix -o out [--bins lower,upper,step] [--years_per_gen g] [--device d]
//          (RelateSelection --mode Frequency of the reference: reads prefix.anc (text) and prefix.mut, writes out.freq
//           and out.lin, the reference's bytes; --device -1: on the host; .gz inputs, sample ages and a .mut with
//           population-frequency columns are refused; no --first_snp / --last_snp)
//   Relate --mode Selection -i prefix -o out
//          (RelateSelection --mode Selection: prefix.freq + prefix.lin -> out.sele, on the host)
//   Relate --mode AvgMutationRate -i prefix -o out [--dist file] [--bins lower,upper,step] [--years_per_gen g] [--device d]
//   Relate --mode CoalRateForTree -i prefix -o out [--bins lower,upper,step] [--years_per_gen g] [--device d]
//          (RelateMutationRate --mode Avg of the reference: reads prefix.anc (text) and prefix.mut, writes
//           out_avg.rate, the reference's bytes; --device -1: on the host; .gz inputs, sample ages and --chr /
//           --first_chr / --last_chr are refused)
//   Relate --mode SubTreesForSubpopulation --anc a.anc --mut a.mut --poplabels f --pop_of_interest A,B -o out [--device d]
//          (RelateExtract --mode SubTreesForSubpopulation of the reference: the subtrees of the groups' haplotypes as
//           out.anc (text), out.mut and out.poplabels, the reference's bytes; --device -1: on the host; .gz inputs and
//           sample ages are refused)
//   Relate --mode MutationRateWithContext -i prefix -o out --mask m.fa --ancestor a.fa [--dist file]
//          [--bins lower,upper,step] [--years_per_gen g] [--device d]
//          (RelateMutationRate --mode WithContextForChromosome of the reference: reads prefix.anc (text) and
//           prefix.mut, writes out_mut.bin and out_opp.bin, the reference's bytes; --device -1: on the host; .gz inputs
//           and sample ages are refused)
//   Relate --mode FinalizeMutationRate -i prefix -o out [--first_chr a --last_chr b | --chr file]
//          (RelateMutationRate --mode Finalize: prefix_mut.bin + prefix_opp.bin -> out.rate; with chromosomes first
//           out_chr<c>_{mut,opp}.bin summed into out_{mut,opp}.bin, the per-chromosome files kept; on the host)
// Same options, files and stderr banners as include/pipeline/Relate.cpp:19-115,
// Paint.cpp, BuildTopology.cpp of the reference; every other --mode is refused
// (use the reference binary for them).  Extra options: --device n,
// --sum_mode exact|lanes|lanes32, --find_equivalent_branches (with PaintBuildTopology / BuildTopology over all
// sections of a chunk: the stage downstream fused in, every .anc written once), --paint_all_windows (PaintBuildTopology
// of a section range paints the range's windows only, RelateParallel.sh:231-257; with it, every window as --mode Paint
// does, which ignores the section options as in the reference).
#include <sys/resource.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "relate_amd.h"

static void usage_line() {
  rusage usage;
  getrusage(RUSAGE_SELF, &usage);
  std::cerr << "CPU Time spent: " << usage.ru_utime.tv_sec << "." << std::setfill('0') << std::setw(6)
            << usage.ru_utime.tv_usec << "s; Max Memory usage: " << usage.ru_maxrss / 1000.0 << "Mb." << std::endl;
  std::cerr << "---------------------------------------------------------" << std::endl << std::endl;
}

static const char *kModes = "MakeChunks|Paint|BuildTopology|PaintBuildTopology|FindEquivalentBranches|OptimizeParameters|CompareTopology|PairwiseCoalescence|CopyingMatrix|CoalescentRateForSection|FinalizePopulationSize|Frequency|Selection|AvgMutationRate|CoalRateForTree|SubTreesForSubpopulation|MutationRateWithContext|FinalizeMutationRate";

// `Relate --mode OptimizeParameters` (pipeline/OptimizeParameters.cpp:22-206): MakeChunks, then for every chunk the
// grid of (theta, recombination factor) through rl_stage_optimize_parameters, the temporary files removed as the
// reference's Clean leaves them (pipeline/Clean.cpp:16-138), and <output>.opt next to (not inside) the directory.
static int optimize_parameters(std::map<std::string, std::string> &opt, rl_stage_opts &so) {
  if (!opt.count("haps") || !opt.count("sample") || !opt.count("map") || !opt.count("output") || opt.count("help")) {
    if (!opt.count("help")) {
      std::cout << "Not enough arguments supplied." << std::endl;
      std::cout << "Needed: haps, sample, map, output. Optional: dist." << std::endl;
    }
    std::cout << "Usage: Relate --mode " << kModes << " [options]" << std::endl;
    std::cout << "  OptimizeParameters: --haps x.haps --sample x.sample --map x.map -o out [--memory GB] [--dist f] "
                 "[-i,--input grid] [--painting theta,rho]" << std::endl;
    std::cout << "Use to make smaller chunks from the data." << std::endl;
    return 0;  // (exit(0), OptimizeParameters.cpp:30-34)
  }
  const std::string out = opt["output"];
  std::cerr << "############" << std::endl;
  std::cerr << "Optimizing Parameters..." << std::endl;
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Using:" << std::endl;
  std::cerr << "  " << opt["haps"] << std::endl;
  std::cerr << "  " << opt["sample"] << std::endl;
  std::cerr << "  " << opt["map"] << std::endl;
  {  // (printed whether or not the options are given, OptimizeParameters.cpp:49-53; neither is read by the mode)
    const float mu = opt.count("mutation_rate") ? std::stof(opt["mutation_rate"]) : 0.0f;
    std::cerr << "with mu = " << mu << " and ";
    if (!opt.count("coal")) std::cerr << "2Ne = " << (opt.count("effectiveN") ? std::stof(opt["effectiveN"]) : 0.0f) << "." << std::endl;
    else std::cerr << "coal = " << opt["coal"] << "." << std::endl;
  }
  std::cerr << "---------------------------------------------------------" << std::endl << std::endl;
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Parsing data.." << std::endl;
  const float memory = opt.count("memory") ? std::stof(opt["memory"]) : 5.0f;
  if (rl_stage_make_chunks(opt["haps"].c_str(), opt["sample"].c_str(), opt["map"].c_str(),
                           opt.count("dist") ? opt["dist"].c_str() : nullptr, out.c_str(),
                           opt.count("transversion") ? 1 : 0, memory) != 0) {
    std::cerr << rl_last_error() << std::endl;
    return 1;
  }
  usage_line();
  int N = 0, L = 0, num_chunks = 0;
  double memory_size = 0.0;
  {
    FILE *fp = fopen((out + "/parameters.bin").c_str(), "rb");
    const bool ok = fp && fread(&N, 4, 1, fp) == 1 && fread(&L, 4, 1, fp) == 1 && fread(&num_chunks, 4, 1, fp) == 1 &&
                    fread(&memory_size, 8, 1, fp) == 1;
    if (fp) fclose(fp);
    if (!ok) {
      std::cerr << "Error: cannot read " << out << "/parameters.bin" << std::endl;
      return 1;
    }
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Read " << N << " haplotypes with " << L << " SNPs per haplotype." << std::endl;
  std::cerr << "Expected minimum memory usage: " << memory_size << "Gb." << std::endl;
  std::cerr << "---------------------------------------------------------" << std::endl << std::endl;
  std::vector<float> theta = {1e-4, 1e-3, 1e-2, 1e-1};       // :76
  std::vector<float> rec_factor = {0.001, 0.1, 1, 10, 100};  // :77
  if (opt.count("input")) {  // line 1: thetas, line 2: factors (:81-112)
    std::ifstream is(opt["input"]);
    theta.clear();
    rec_factor.clear();
    std::string line;
    float val;
    getline(is, line);
    std::istringstream itheta(line);
    while (itheta >> val) {
      if (val >= 1.0 || val <= 0) {
        std::cerr << "Error: theta value has to be in (0,1)" << std::endl;
        return 1;
      }
      theta.push_back(val);
    }
    line.clear();
    getline(is, line);
    std::istringstream irec(line);
    while (irec >> val) {
      if (val <= 0) {
        std::cerr << "Error: rho value has to be positive" << std::endl;
        return 1;
      }
      rec_factor.push_back(val);
    }
  }
  std::vector<int> counts(theta.size() * rec_factor.size(), 0);
  for (int c = 0; c < num_chunks; c++) {
    std::cerr << "---------------------------------------------------------" << std::endl;
    std::cerr << "Starting chunk " << c << " of " << num_chunks - 1 << "." << std::endl;
    std::cerr << "---------------------------------------------------------" << std::endl << std::endl;
    if (counts.empty()) continue;
    if (rl_stage_optimize_parameters(out.c_str(), c, theta.data(), (int)theta.size(), rec_factor.data(),
                                     (int)rec_factor.size(), &so, counts.data()) != 0) {
      std::cerr << "Error: " << rl_last_error() << std::endl;
      return 1;
    }
  }
  // Clean (pipeline/Clean.cpp:31-120) for what this mode leaves: the chunk files (and the bit-packed panel of this
  // build's MakeChunks), the parameter files, the directories if a stage made them
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Cleaning directory..." << std::endl;
  for (int c = 0; c < num_chunks; c++) {
    const std::string cs = std::to_string(c), base = out + "/chunk_" + cs;
    for (const char *ext : {".hap", ".r", ".rpos", ".state", ".dist", ".bp", ".bits"}) std::remove((base + ext).c_str());
    std::remove((out + "/parameters_c" + cs + ".bin").c_str());
    (void)rmdir((base + "/paint").c_str());
    (void)rmdir(base.c_str());
  }
  std::remove((out + "/parameters.bin").c_str());
  std::remove((out + "/props.bin").c_str());
  (void)rmdir(out.c_str());
  usage_line();
  std::ofstream os(out + ".opt");  // :183-189 (operator<< of float / int)
  for (size_t i = 0; i < theta.size(); i++)
    for (size_t j = 0; j < rec_factor.size(); j++)
      os << theta[i] << " " << rec_factor[j] << " " << counts[i * rec_factor.size() + j] << std::endl;
  os.close();
  usage_line();
  return 0;
}

// `Relate --mode CompareTopology -i a.anc,b.anc [-o out] [--device d]` (rl_compare_anc)
static int compare_topology(std::map<std::string, std::string> &opt) {
  const std::string in = opt.count("input") ? opt["input"] : std::string();
  const size_t c = in.find(',');
  if (c == std::string::npos || c == 0 || c + 1 == in.size()) {
    std::cerr << "Not enough arguments supplied." << std::endl;
    std::cerr << "Needed: -i,--input a.anc,b.anc. Optional: output, device." << std::endl;
    return 1;
  }
  const std::string a = in.substr(0, c), b = in.substr(c + 1);
  const std::string cmp = opt.count("output") ? opt["output"] + ".cmp" : std::string();
  rl_compare_summary s;
  if (rl_compare_anc(a.c_str(), b.c_str(), opt.count("device") ? atoi(opt["device"].c_str()) : 0, &s,
                     cmp.empty() ? nullptr : cmp.c_str()) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  char line[512];
  snprintf(line, sizeof line,
           "haplotypes %d\ntrees_a %d\ntrees_b %d\nintervals %d\nsnp_begin %d\nsnp_end %d\nmean_normalised_distance %.17g\n"
           "max_distance %d\nsnps_identical %lld\nshare_identical %.17g\n",
           s.N, s.trees_a, s.trees_b, s.intervals, s.snp_begin, s.snp_end, s.mean_normalised, s.max_distance,
           s.snps_identical, s.share_identical);
  std::cout << line;
  return 0;
}

// `Relate --mode PairwiseCoalescence -i a.anc[,b.anc,...] -o out [--metric size|time] [--device d]` (rl_pairwise_anc)
static int pairwise_coalescence(std::map<std::string, std::string> &opt) {
  std::vector<std::string> files;
  {
    std::istringstream in(opt.count("input") ? opt["input"] : std::string());
    for (std::string f; getline(in, f, ',');)
      if (!f.empty()) files.push_back(f);
  }
  if (files.empty() || !opt.count("output")) {
    std::cerr << "Not enough arguments supplied." << std::endl;
    std::cerr << "Needed: -i,--input a.anc[,b.anc,...], output. Optional: metric, device." << std::endl;
    return 1;
  }
  const std::string name = opt.count("metric") ? opt["metric"] : std::string("size");
  if (name != "size" && name != "time") {
    std::cerr << "--metric must be size or time" << std::endl;
    return 1;
  }
  const int metric = name == "time" ? RL_PAIRWISE_TIME : RL_PAIRWISE_SIZE;
  const int device = opt.count("device") ? atoi(opt["device"].c_str()) : 0;
  std::vector<const char *> paths;
  for (const std::string &f : files) paths.push_back(f.c_str());
  int N = 0;
  long long W = 0;
  if (rl_pairwise_anc(paths.data(), (int)paths.size(), metric, device, nullptr, nullptr, &N) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  std::vector<uint64_t> S((size_t)N * N);  // (the bits of doubles for --metric time)
  if (rl_pairwise_anc(paths.data(), (int)paths.size(), metric, device, S.data(), &W, &N) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  long long trees = 0;
  for (const std::string &f : files) {  // header of a .anc file: bool ages, uint32 N, [N doubles], uint32 trees
    FILE *fp = fopen(f.c_str(), "rb");
    unsigned char ages = 0;
    unsigned n = 0, t = 0;
    const bool ok = fp && fread(&ages, 1, 1, fp) == 1 && fread(&n, 4, 1, fp) == 1 &&
                    (!ages || fseek(fp, (long)n * 8, SEEK_CUR) == 0) && fread(&t, 4, 1, fp) == 1;
    if (fp) fclose(fp);
    if (!ok) {
      std::cerr << "Error: cannot read the header of " << f << std::endl;
      return 1;
    }
    trees += t;
  }
  const std::string out = opt["output"] + ".pwc";
  {
    FILE *fp = fopen(out.c_str(), "wb");
    const int32_t head[2] = {N, metric};
    const int64_t w = W;
    const bool ok = fp && fwrite(head, 4, 2, fp) == 2 && fwrite(&w, 8, 1, fp) == 1 && fwrite(S.data(), 8, S.size(), fp) == S.size();
    if ((fp && fclose(fp) != 0) || !ok) {
      std::cerr << "Error: writing " << out << " failed" << std::endl;
      return 1;
    }
  }
  // the mean matrix S / W: its off-diagonal mean (row order, double) and its extreme pairs (the first in row order)
  auto mean_of = [&](size_t k) {
    double s;
    if (metric == RL_PAIRWISE_TIME) memcpy(&s, &S[k], 8);
    else s = (double)S[k];
    return s / (double)W;
  };
  double sum = 0.0, lo = 0.0, hi = 0.0;
  int lo_i = -1, lo_j = -1, hi_i = -1, hi_j = -1;
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++) {
      if (i == j) continue;
      const double v = mean_of((size_t)i * N + j);
      sum += v;
      if (j < i) continue;
      if (lo_i < 0 || v < lo) lo = v, lo_i = i, lo_j = j;
      if (hi_i < 0 || v > hi) hi = v, hi_i = i, hi_j = j;
    }
  char line[768];
  snprintf(line, sizeof line,
           "haplotypes %d\nfiles %d\ntrees %lld\nsnps %lld\nmetric %s\nmean %.17g\nmin_pair %d %d %.17g\nmax_pair %d %d %.17g\n",
           N, (int)files.size(), trees, W, name.c_str(), sum / ((double)N * (double)(N - 1)), lo_i, lo_j, lo, hi_i, hi_j, hi);
  std::cout << line;
  return 0;
}

// `Relate --mode CopyingMatrix --chunk_index c -o out [--first_section a --last_section b] [--painting t,r]
// [--sum_mode m] [--device d]` (rl_stage_copying_matrix): out.cpy and a summary of the copying shares C / W
static int copying_matrix(const std::string &out, int chunk, int first_section, int last_section, const rl_stage_opts &so) {
  const std::string path = out + ".cpy";
  if (rl_stage_copying_matrix(out.c_str(), chunk, first_section, last_section, &so, path.c_str()) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  int32_t head[4] = {0, 0, 0, 0};
  int64_t W = 0;
  std::vector<double> C;
  {
    FILE *fp = fopen(path.c_str(), "rb");
    bool ok = fp && fread(head, 4, 4, fp) == 4 && fread(&W, 8, 1, fp) == 1 && head[0] > 0;
    if (ok) {
      C.resize((size_t)head[0] * head[0]);
      ok = fread(C.data(), 8, C.size(), fp) == C.size();
    }
    if (fp) fclose(fp);
    if (!ok) {
      std::cerr << "Error: cannot read back " << path << std::endl;
      return 1;
    }
  }
  const int N = head[0];
  int windows = 0;
  {  // parameters_c<c>.bin: int32 N, L, W + 1, then the window boundaries
    FILE *fp = fopen((out + "/parameters_c" + std::to_string(chunk) + ".bin").c_str(), "rb");
    int32_t h3[3] = {0, 0, 0};
    if (fp && fread(h3, 4, 3, fp) == 3 && h3[2] > 0) {
      std::vector<int32_t> wb((size_t)h3[2]);
      if (fread(wb.data(), 4, wb.size(), fp) == wb.size())
        for (size_t w = 0; w + 1 < wb.size(); w++) windows += wb[w] >= head[2] && wb[w + 1] <= head[3];
    }
    if (fp) fclose(fp);
  }
  // shares in row order, sums in double in column order
  double top = -1.0, worst = 0.0, donors = 0.0;
  int top_i = -1, top_j = -1;
  for (int i = 0; i < N; i++) {
    double rowsum = 0.0, sq = 0.0;
    for (int j = 0; j < N; j++) {
      const double c = C[(size_t)i * N + j], share = c / (double)W;
      rowsum += c;
      sq += share * share;
      if (i != j && share > top) top = share, top_i = i, top_j = j;
    }
    worst = std::max(worst, std::fabs(rowsum / (double)W - 1.0));
    donors += 1.0 / sq;
  }
  char line[768];
  snprintf(line, sizeof line,
           "haplotypes %d\nwindows %d\nsnps %lld\nmax_share %d %d %.17g\nmax_rowsum_error %.17g\nmean_effective_donors %.17g\n",
           N, windows, (long long)W, top_i, top_j, top, worst, donors / (double)N);
  std::cout << line;
  return 0;
}

// `Relate --mode CoalescentRateForSection -i prefix -o out [--bins l,u,s] [--years_per_gen g] [--device d]`
// (evaluate/coalescent_rate/CoalescentRateForSection.cpp:227-602 without sample ages: rl_coalrate_epochs,
// rl_coalrate_anc, rl_coalrate_write_bin)
static int coalescent_rate_for_section(std::map<std::string, std::string> &opt) {
  if (!opt.count("input") || !opt.count("output")) {
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: input, output. Optional: years_per_gen, bins, device." << std::endl;
    std::cout << "Reads .anc file and calculates pairwise coalescence rate. Output is bin file." << std::endl;
    return 0;  // (exit(0), :234-243)
  }
  for (const char *o : {"mask", "dist"})
    if (opt.count(o)) {
      std::cerr << "Error: --" << o << " is not part of this build's CoalescentRateForSection; run the reference's RelateCoalescentRate for it." << std::endl;
      return 1;
    }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating coalescence rate for " << opt["input"] << " ..." << std::endl;
  float years_per_gen = 28.0f;
  try {
    if (opt.count("years_per_gen")) years_per_gen = std::stof(opt["years_per_gen"]);
  } catch (...) {
    std::cerr << "Error: --years_per_gen expects a number" << std::endl;
    return 1;
  }
  std::vector<float> epochs(4096);
  int E = (int)epochs.size(), N = 0;
  const int device = opt.count("device") ? atoi(opt["device"].c_str()) : 0;
  const std::string anc = opt["input"] + ".anc", mut = opt["input"] + ".mut", bin = opt["output"] + ".bin";
  bool ok = rl_coalrate_epochs(years_per_gen, opt.count("bins") ? opt["bins"].c_str() : nullptr, epochs.data(), &E) == 0 &&
            rl_coalrate_anc(anc.c_str(), mut.c_str(), epochs.data(), E, device, nullptr, &N) == 0;
  std::vector<float> D;
  if (ok) {
    D.resize((size_t)E * N * N);
    ok = rl_coalrate_anc(anc.c_str(), mut.c_str(), epochs.data(), E, device, D.data(), &N) == 0 &&
         rl_coalrate_write_bin(bin.c_str(), epochs.data(), E, D.data(), N) == 0;
  }
  if (!ok) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  usage_line();
  return 0;
}

// `Relate --mode FinalizePopulationSize -o out [--poplabels f]` (FinalizePopulationSize.cpp:13-136, :138-291:
// rl_coalrate_finalize_files)
static int finalize_population_size(std::map<std::string, std::string> &opt) {
  if (!opt.count("output")) {
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed:output. Optional: poplabels." << std::endl;
    std::cout << "Estimate population size." << std::endl;
    return 0;  // (exit(0), RelateCoalescentRate.cpp:109-119)
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Finalizing coalescence rate..." << std::endl;
  const std::string bin = opt["output"] + ".bin", coal = opt["output"] + ".coal";
  if (rl_coalrate_finalize_files(bin.c_str(), opt.count("poplabels") ? opt["poplabels"].c_str() : nullptr, coal.c_str()) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  usage_line();
  return 0;
}

// `Relate --mode Frequency -i prefix -o out [--bins l,u,s] [--years_per_gen g] [--device d]`
// (evaluate/selection/RelateSelection.cpp:330-814: rl_coalrate_epochs, rl_frequency_anc)
static int frequency(std::map<std::string, std::string> &opt) {
  if (!opt.count("input") || !opt.count("output")) {
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: input, output. Optional: years_per_gen, bins, device." << std::endl;
    return 0;  // (exit(0), :335-345)
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating frequency through time for " << opt["input"] << "." << std::endl;
  float years_per_gen = 28.0f;
  try {
    if (opt.count("years_per_gen")) years_per_gen = std::stof(opt["years_per_gen"]);
  } catch (...) {
    std::cerr << "Error: --years_per_gen expects a number" << std::endl;
    return 1;
  }
  std::vector<float> epochs(4096);
  int E = (int)epochs.size(), host_trees = 0;
  long long rows = 0;
  const int device = opt.count("device") ? atoi(opt["device"].c_str()) : 0;
  const std::string anc = opt["input"] + ".anc", mut = opt["input"] + ".mut", freq = opt["output"] + ".freq", lin = opt["output"] + ".lin";
  if (rl_coalrate_epochs(years_per_gen, opt.count("bins") ? opt["bins"].c_str() : nullptr, epochs.data(), &E) != 0 ||
      rl_frequency_anc(anc.c_str(), mut.c_str(), epochs.data(), E, device, freq.c_str(), lin.c_str(), &rows, &host_trees) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  if (device >= 0 && host_trees) std::cerr << host_trees << " trees with tied node times were walked on the host." << std::endl;
  usage_line();
  return 0;
}

// `Relate --mode Selection -i prefix -o out` (RelateSelection.cpp:190-328: rl_selection_files)
static int selection(std::map<std::string, std::string> &opt) {
  if (!opt.count("input") || !opt.count("output")) {
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: input, output." << std::endl;
    std::cout << "Calculating pvalue for selection using output of mode Frequency." << std::endl;
    return 0;  // (exit(0), :195-205)
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating evidence of selection for " << opt["input"] << "." << std::endl;
  const std::string sele = opt["output"] + ".sele";
  if (rl_selection_files(opt["input"].c_str(), sele.c_str()) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  usage_line();
  return 0;
}

// `Relate --mode AvgMutationRate -i prefix -o out [--dist file] [--bins l,u,s] [--years_per_gen g] [--device d]`
// (evaluate/mutation_rate/AvgMutationRate.cpp:830-1013, RelateMutationRate --mode Avg: rl_mutrate_epochs,
// rl_mutrate_anc, rl_mutrate_write; a summary on stdout in place of the reference's terminal plot)
static int avg_mutation_rate(std::map<std::string, std::string> &opt) {
  if (!opt.count("input") || !opt.count("output")) {
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: input, output. Optional: dist, years_per_gen, bins, device." << std::endl;
    std::cout << "Calculate avg mutation rate through time." << std::endl;
    return 0;  // (exit(0), :833-842)
  }
  for (const char *o : {"chr", "first_chr", "last_chr"})
    if (opt.count(o)) {
      std::cerr << "Error: --" << o << " is not part of this build's AvgMutationRate: one chromosome per run; run the reference's RelateMutationRate for it." << std::endl;
      return 1;
    }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating average mutation rate for " << opt["input"] << " ..." << std::endl;
  float years_per_gen = 28.0f;
  try {
    if (opt.count("years_per_gen")) years_per_gen = std::stof(opt["years_per_gen"]);
  } catch (...) {
    std::cerr << "Error: --years_per_gen expects a number" << std::endl;
    return 1;
  }
  std::vector<double> epochs(4096);
  int E = (int)epochs.size();
  long long mapped = 0;
  const int device = opt.count("device") ? atoi(opt["device"].c_str()) : 0;
  const std::string anc = opt["input"] + ".anc", mut = opt["input"] + ".mut", rate = opt["output"] + "_avg.rate";
  if (rl_mutrate_epochs(years_per_gen, opt.count("bins") ? opt["bins"].c_str() : nullptr, epochs.data(), &E) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  std::vector<double> mutation(E), opportunity(E);
  if (rl_mutrate_anc(anc.c_str(), mut.c_str(), opt.count("dist") ? opt["dist"].c_str() : nullptr, epochs.data(), E, device,
                     mutation.data(), opportunity.data(), &mapped) != 0 ||
      rl_mutrate_write(rate.c_str(), epochs.data(), E, mutation.data(), opportunity.data()) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  double mutations = 0.0, chances = 0.0;
  for (int e = 0; e < E; e++) mutations += mutation[e], chances += opportunity[e];
  std::cout << mapped << " mapped SNPs, " << E << " epochs, average rate " << (chances > 0.0 ? mutations / chances / 1e9 : 0.0)
            << " per base per generation; " << rate << " written." << std::endl;
  usage_line();
  return 0;
}

// `Relate --mode MutationRateWithContext -i prefix -o out --mask m.fa --ancestor a.fa [--dist file] [--bins l,u,s]
// [--years_per_gen g] [--device d]` (MutationRateWithContext, evaluate/mutation_rate/RelateMutationRate.cpp:578-949,
// RelateMutationRate --mode WithContextForChromosome: rl_mutrate_epochs, rl_mutctx_anc, rl_mutctx_write; a summary on
// stdout)
static int mutation_rate_with_context(std::map<std::string, std::string> &opt) {
  if (!opt.count("mask") || !opt.count("ancestor") || !opt.count("input") || !opt.count("output")) {
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: mask, ancestor, input, output. Optional: years_per_gen, bins, dist, device." << std::endl;
    std::cout << "Calculate mutation rate for 96 categories (Do not apply after using RemoveTreesWithFewMutations).." << std::endl;
    return 0;  // (exit(0), :580-590)
  }
  for (const char *o : {"chr", "first_chr", "last_chr"})
    if (opt.count(o)) {
      std::cerr << "Error: --" << o << " is not part of this build's MutationRateWithContext: one chromosome per run (-i prefix_chr<c> -o out_chr<c>), then FinalizeMutationRate with --" << o << "." << std::endl;
      return 1;
    }
  std::cerr << "------------------------------------------------------" << std::endl;
  std::cerr << "Calculating mutation rate for 96 categories " << opt["input"] << " ..." << std::endl;
  float years_per_gen = 28.0f;
  try {
    if (opt.count("years_per_gen")) years_per_gen = std::stof(opt["years_per_gen"]);
  } catch (...) {
    std::cerr << "Error: --years_per_gen expects a number" << std::endl;
    return 1;
  }
  std::vector<double> epochs(4096);
  int E = (int)epochs.size();
  const int device = opt.count("device") ? atoi(opt["device"].c_str()) : 0;
  const std::string anc = opt["input"] + ".anc", mut = opt["input"] + ".mut";
  if (rl_mutrate_epochs(years_per_gen, opt.count("bins") ? opt["bins"].c_str() : nullptr, epochs.data(), &E) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  std::vector<double> mutation((size_t)E * 96), opportunity((size_t)E * 96);
  long long snps[3] = {0, 0, 0};
  if (rl_mutctx_anc(anc.c_str(), mut.c_str(), opt["mask"].c_str(), opt["ancestor"].c_str(),
                    opt.count("dist") ? opt["dist"].c_str() : nullptr, epochs.data(), E, device, mutation.data(),
                    opportunity.data(), snps) != 0 ||
      rl_mutctx_write(opt["output"].c_str(), epochs.data(), E, mutation.data(), opportunity.data()) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  std::cout << snps[0] << " SNPs, " << snps[2] << " qualifying SNPs of " << snps[1] << " with one branch, " << E << " epochs; "
            << opt["output"] << "_mut.bin and " << opt["output"] << "_opp.bin written." << std::endl;
  usage_line();
  return 0;
}

// `Relate --mode FinalizeMutationRate -i prefix -o out [--first_chr a --last_chr b | --chr file]` (RelateMutationRate
// --mode Finalize, RelateMutationRate.cpp:3568-3579: with chromosomes SummarizeWholeGenome :445-576, which reads
// OUT_chr<c>_{mut,opp}.bin and writes OUT_{mut,opp}.bin -- rl_mutctx_sum; the per-chromosome files are not removed --,
// then FinalizeMutationRate :344-443, which reads IN_{mut,opp}.bin and writes OUT.rate -- rl_mutctx_finalize)
static int finalize_mutation_rate(std::map<std::string, std::string> &opt) {
  if (!opt.count("input") || !opt.count("output")) {
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: input, output. Optional: chr, first_chr, last_chr." << std::endl;
    std::cout << "Extract mutation rate of 96 categories from .bin file." << std::endl;
    return 0;  // (exit(0), :350-360)
  }
  std::string chromosomes;
  if (opt.count("chr")) {
    std::ifstream is(opt["chr"]);
    if (is.fail()) {
      std::cerr << "Error while opening file " << opt["chr"] << std::endl;
      return 1;
    }
    for (std::string line; getline(is, line);) chromosomes += line + "\n";
  } else if (opt.count("first_chr") && opt.count("last_chr")) {
    const int first = atoi(opt["first_chr"].c_str()), last = atoi(opt["last_chr"].c_str());
    if (first < 0 || last < 0) {
      std::cerr << "Do not use negative chr indices." << std::endl;
      return 1;
    }
    for (int chr = first; chr <= last; chr++) chromosomes += std::to_string(chr) + "\n";
  }
  if (opt.count("chr") || (opt.count("first_chr") && opt.count("last_chr"))) {
    std::cerr << "------------------------------------------------------" << std::endl;
    std::cerr << "Summarizing mutation rates..." << std::endl;
    if (rl_mutctx_sum(opt["output"].c_str(), chromosomes.c_str(), opt["output"].c_str()) != 0) {
      std::cerr << "Error: " << rl_last_error() << std::endl;
      return 1;
    }
  }
  std::cerr << "------------------------------------------------------" << std::endl;
  std::cerr << "Finalizing mutation rate..." << std::endl;
  const std::string rate = opt["output"] + ".rate";
  if (rl_mutctx_finalize(opt["input"].c_str(), rate.c_str()) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  std::cout << rate << " written." << std::endl;
  usage_line();
  return 0;
}

// `Relate --mode CoalRateForTree -i prefix -o out [--bins l,u,s] [--years_per_gen g] [--device d]`
// (CoalescenceRateForTree, evaluate/coalescent_rate/CoalescentRateForSection.cpp:605-858, RelateCoalescentRate --mode
// CoalRateForTree: rl_mutrate_epochs -- :630-713 is the text of AvgMutationRate.cpp:373-456 --, rl_coaltree_anc,
// rl_coaltree_rates, rl_coaltree_write; a summary on stdout)
static int coal_rate_for_tree(std::map<std::string, std::string> &opt) {
  if (!opt.count("input") || !opt.count("output")) {
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: input, output. Optional: years_per_gen, bins, device." << std::endl;
    std::cout << "Calculate coalescence rates for sample." << std::endl;
    return 0;  // (exit(0), :611-620)
  }
  for (const char *o : {"dist", "chr"})
    if (opt.count(o)) {
      std::cerr << "Error: --" << o << " is not part of this build's CoalRateForTree: one chromosome per run with the .mut's own distances; run the reference's RelateCoalescentRate for it." << std::endl;
      return 1;
    }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating coalescence rates for " << opt["input"] << "..." << std::endl;
  float years_per_gen = 28.0f;
  try {
    if (opt.count("years_per_gen")) years_per_gen = std::stof(opt["years_per_gen"]);
  } catch (...) {
    std::cerr << "Error: --years_per_gen expects a number" << std::endl;
    return 1;
  }
  std::vector<double> epochs(4096);
  int E = (int)epochs.size(), ntrees = 0;
  const int device = opt.count("device") ? atoi(opt["device"].c_str()) : 0;
  const std::string anc = opt["input"] + ".anc", mut = opt["input"] + ".mut", coal = opt["output"] + ".coal";
  if (rl_mutrate_epochs(years_per_gen, opt.count("bins") ? opt["bins"].c_str() : nullptr, epochs.data(), &E) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  std::vector<double> num(E), denom(E), rates(E);
  if (rl_coaltree_anc(anc.c_str(), mut.c_str(), epochs.data(), E, device, num.data(), denom.data(), &ntrees) != 0 ||
      rl_coaltree_rates(num.data(), denom.data(), E, rates.data()) != 0 ||
      rl_coaltree_write(coal.c_str(), epochs.data(), E, rates.data()) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  int with_rate = 0;
  for (int e = 0; e < E; e++) with_rate += denom[e] != 0;
  std::cout << ntrees << " trees in " << rl_coaltree_num_blocks(ntrees, 1000) << " blocks of 1000, " << with_rate << " of " << E
            << " epochs with a rate of their own; " << coal << " written." << std::endl;
  usage_line();
  return 0;
}

// `Relate --mode SubTreesForSubpopulation --anc a.anc --mut a.mut --poplabels f --pop_of_interest A,B -o out [--device d]`
// (CreateAncesTreeFileForSubpopulation, extract/CreateAncesTreeFileForSubpopulation.cpp:284-401, RelateExtract --mode
// SubTreesForSubpopulation: rl_subtrees_poplabels for the banner, rl_subtrees_files; a summary on stdout)
static int sub_trees_for_subpopulation(std::map<std::string, std::string> &opt) {
  if (!opt.count("pop_of_interest") || !opt.count("poplabels") || !opt.count("anc") || !opt.count("mut") || !opt.count("output")) {
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: pop_of_interest, poplabels, anc, mut, output." << std::endl;
    std::cout << "Estimate population size using coalescent rate." << std::endl;
    return 0;  // (exit(0), :290-300)
  }
  {  // (:306-309; the frequency columns follow the thirteen of the standard header)
    std::ifstream is(opt["mut"]);
    std::string line;
    if (getline(is, line) && getline(is, line) && std::count(line.begin(), line.end(), ';') <= 13)
      std::cerr << "We recommend to first add population annotation to .mut using RelateFileFormats --mode GenerateSNPAnnotations" << std::endl;
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating anc file for " << opt["anc"] << " and subpopulation(s) ";
  int haplotypes = 0, num_groups = 0, names_bytes = 0;
  if (rl_subtrees_poplabels(opt["poplabels"].c_str(), opt["pop_of_interest"].c_str(), nullptr, &haplotypes, nullptr, &num_groups, nullptr, &names_bytes) != 0) {
    std::cerr << std::endl << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  std::vector<int> of_interest(num_groups);
  std::string names(names_bytes, ' ');
  if (rl_subtrees_poplabels(opt["poplabels"].c_str(), opt["pop_of_interest"].c_str(), nullptr, &haplotypes, of_interest.data(), &num_groups, &names[0], &names_bytes) != 0) {
    std::cerr << std::endl << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  if (opt["pop_of_interest"] != "All") {
    std::istringstream ns(names);
    std::string group;
    for (int g = 0; g < num_groups && getline(ns, group); g++)
      if (of_interest[g]) std::cerr << group << " ";
    std::cerr << std::endl;
  } else {
    std::cerr << "All" << std::endl;
  }
  const int device = opt.count("device") ? atoi(opt["device"].c_str()) : 0;
  rl_subtrees_summary sum;
  if (rl_subtrees_files(opt["anc"].c_str(), opt["mut"].c_str(), opt["poplabels"].c_str(), opt["pop_of_interest"].c_str(),
                        opt["output"].c_str(), device, &sum) != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  std::cout << sum.M << " of " << sum.N << " haplotypes; " << sum.trees_kept << " of " << sum.trees_read << " trees and " << sum.snps_kept
            << " of " << sum.snps_read << " SNPs kept; " << opt["output"] << ".anc, .mut and .poplabels written." << std::endl;
  usage_line();
  return 0;
}

int main(int argc, char **argv) {
  // BuildTopology keeps several tree-builder launches and window kernels in flight from its section threads: more
  // hardware queues than HIP's default four (read when the runtime starts; an explicit setting wins) -- but not more
  // than the device keeps resident: past 16 the queues are time-sliced and every build kernel, preempted with its
  // 150 KB of LDS, ran 1.37x longer (C3, 80 sections open: 135 s with 24 queues, 121 s with 20, 91 s with 12 or 16,
  // 96 s with 4 to 8)
  setenv("GPU_MAX_HW_QUEUES", "12", 0);
  // This process runs one stage and ends: the blocks its contexts release stay in the library's cache until the
  // process is gone instead of going back to the driver one hipFree at a time (C3: ~3000 blocks, 4 s)
  rl_keep_cache_until_exit(1);
  // option table of Relate.cpp:19-45 restricted to what the two modes read
  const std::map<std::string, bool> known = {  // name -> takes a value
      {"mode", true}, {"chunk_index", true}, {"first_section", true}, {"last_section", true},
      {"output", true}, {"painting", true}, {"seed", true}, {"fb", true}, {"sample_ages", true},
      {"no_consistency", false}, {"device", true}, {"sum_mode", true}, {"help", false},
      {"find_equivalent_branches", false},  // (PaintBuildTopology / BuildTopology of a whole chunk: the next stage fused in)
      {"paint_all_windows", false},  // (PaintBuildTopology of a section range: Paint keeps every window, not the range's)
      {"input", true},  // (OptimizeParameters: the grid, Relate.cpp:43)
      {"metric", true},  // (PairwiseCoalescence: size | time)
      // (CoalescentRateForSection / FinalizePopulationSize, RelateCoalescentRate.cpp:14-34; mask is named to be refused;
      //  Frequency / Selection read input, output, bins and years_per_gen of RelateSelection.cpp:1586-1596)
      {"bins", true}, {"years_per_gen", true}, {"poplabels", true}, {"mask", true},
      // (AvgMutationRate reads input, output, dist, bins and years_per_gen of RelateMutationRate.cpp; the three that
      //  name several chromosomes are named to be refused; CoalRateForTree reads input, output, bins and years_per_gen
      //  of RelateCoalescentRate.cpp and refuses dist and chr)
      {"chr", true}, {"first_chr", true}, {"last_chr", true},
      // (SubTreesForSubpopulation reads anc, mut, poplabels, pop_of_interest and output of RelateExtract.cpp)
      {"anc", true}, {"mut", true}, {"pop_of_interest", true},
      // (MutationRateWithContext reads mask, ancestor, input, output, dist, bins and years_per_gen of
      //  RelateMutationRate.cpp; FinalizeMutationRate input, output, chr, first_chr and last_chr)
      {"ancestor", true},
      // accepted and ignored by these two modes in the reference as well
      {"haps", true}, {"sample", true}, {"map", true}, {"mutation_rate", true}, {"effectiveN", true},
      {"memory", true}, {"dist", true}, {"annot", true}, {"coal", true}, {"transversion", false}};
  std::map<std::string, std::string> opt;
  for (int a = 1; a < argc; a++) {
    std::string s = argv[a], name;
    if (s == "-o") name = "output";
    else if (s == "-m") name = "mutation_rate";
    else if (s == "-N") name = "effectiveN";
    else if (s == "-h") name = "help";
    else if (s == "-i") name = "input";
    else if (s.rfind("--", 0) == 0) name = s.substr(2);
    else {
      std::cerr << "Unexpected argument " << s << std::endl;
      return 1;
    }
    auto it = known.find(name);
    if (it == known.end()) {  // cxxopts throws option_not_exists_exception (cxxopts.hpp:1041)
      std::cerr << "Option '" << name << "' does not exist" << std::endl;
      return 1;
    }
    if (it->second) {
      if (a + 1 >= argc) {
        std::cerr << "Option '" << name << "' is missing an argument" << std::endl;
        return 1;
      }
      opt[name] = argv[++a];
    } else {
      opt[name] = "1";
    }
  }
  if ((opt.count("help") && !(opt.count("mode") && opt["mode"] == "OptimizeParameters")) || !opt.count("mode")) {
    std::cerr << "Usage: Relate --mode " << kModes << " [--chunk_index c] -o out [options]" << std::endl;
    std::cerr << "  CompareTopology: -i,--input a.anc,b.anc [-o out] [--device d]" << std::endl;
    std::cerr << "  PairwiseCoalescence: -i,--input a.anc[,b.anc,...] -o out [--metric size|time] [--device d]" << std::endl;
    std::cerr << "  CopyingMatrix: --chunk_index c -o out [--first_section a --last_section b] [--painting theta,rho] [--sum_mode m] [--device d]" << std::endl;
    std::cerr << "  CoalescentRateForSection: -i,--input prefix -o out [--bins lower,upper,step] [--years_per_gen g] [--device d]" << std::endl;
    std::cerr << "  FinalizePopulationSize: -o out [--poplabels f]" << std::endl;
    std::cerr << "  Frequency: -i,--input prefix -o out [--bins lower,upper,step] [--years_per_gen g] [--device d]" << std::endl;
    std::cerr << "  Selection: -i,--input prefix -o out" << std::endl;
    std::cerr << "  AvgMutationRate: -i,--input prefix -o out [--dist file] [--bins lower,upper,step] [--years_per_gen g] [--device d]" << std::endl;
    std::cerr << "  CoalRateForTree: -i,--input prefix -o out [--bins lower,upper,step] [--years_per_gen g] [--device d]" << std::endl;
    std::cerr << "  SubTreesForSubpopulation: --anc a.anc --mut a.mut --poplabels f --pop_of_interest A,B -o out [--device d]" << std::endl;
    std::cerr << "  MutationRateWithContext: -i,--input prefix -o out --mask m.fa --ancestor a.fa [--dist file] [--bins lower,upper,step] [--years_per_gen g] [--device d]" << std::endl;
    std::cerr << "  FinalizeMutationRate: -i,--input prefix -o out [--first_chr a --last_chr b | --chr file]" << std::endl;
    return opt.count("help") ? 0 : 1;
  }
  const std::string mode = opt["mode"];
  if (mode == "CoalescentRateForSection") return coalescent_rate_for_section(opt);
  if (mode == "FinalizePopulationSize") return finalize_population_size(opt);
  if (mode == "Frequency") return frequency(opt);
  if (mode == "Selection") return selection(opt);
  if (mode == "AvgMutationRate") return avg_mutation_rate(opt);
  if (mode == "CoalRateForTree") return coal_rate_for_tree(opt);
  if (mode == "MutationRateWithContext") return mutation_rate_with_context(opt);
  if (mode == "FinalizeMutationRate") return finalize_mutation_rate(opt);
  for (const char *m : {"MutationRateForCategory", "ForCategoryForChromosome", "ForCategoryForPopForChromosome", "MutationRateForPattern",
                        "ForPatternForChromosome", "FinalizeForCategory", "FinalizeForPattern", "XY", "MutationDensity"})
    if (mode == m) {
      std::cerr << "Error: mode " << mode << " of RelateMutationRate is not part of this build: of the per-category analyses it offers MutationRateWithContext and FinalizeMutationRate; run the reference's RelateMutationRate for this one." << std::endl;
      return 1;
    }
  if (mode == "SubTreesForSubpopulation") return sub_trees_for_subpopulation(opt);
  if (mode == "CompareTopology") return compare_topology(opt);
  if (mode == "PairwiseCoalescence") return pairwise_coalescence(opt);
  if (mode == "OptimizeParameters" && opt.count("output") && opt["output"].find('/') != std::string::npos) {
    std::cerr << "Output needs to be in working directory." << std::endl;  // Relate.cpp:50-58
    return 1;
  }
  if (mode == "OptimizeParameters" && (!opt.count("haps") || !opt.count("sample") || !opt.count("map") ||
                                       !opt.count("output") || opt.count("help"))) {
    rl_stage_opts none;
    rl_stage_opts_init(&none);
    return optimize_parameters(opt, none);  // (the reference's two lines and the help, exit status 0)
  }
  if (!opt.count("output")) {
    std::cerr << "Not enough arguments supplied." << std::endl;
    std::cerr << "Needed: output." << std::endl;
    return 1;
  }
  const std::string out = opt["output"];
  if (out.find('/') != std::string::npos) {  // Relate.cpp:50-58
    std::cerr << "Output needs to be in working directory." << std::endl;
    return 1;
  }
  if (mode == "MakeChunks") {  // pipeline/MakeChunks.cpp:13-114
    if (!opt.count("haps") || !opt.count("sample") || !opt.count("map")) {
      std::cerr << "Not enough arguments supplied." << std::endl;
      std::cerr << "Needed: haps, sample, map, output. Optional: memory, dist, transversion." << std::endl;
      return 1;
    }
    std::cerr << "---------------------------------------------------------" << std::endl;
    std::cerr << "Parsing data.." << std::endl;
    const float memory = opt.count("memory") ? std::stof(opt["memory"]) : 5.0f;
    const int rc = rl_stage_make_chunks(opt["haps"].c_str(), opt["sample"].c_str(), opt["map"].c_str(),
                                        opt.count("dist") ? opt["dist"].c_str() : nullptr, out.c_str(),
                                        opt.count("transversion") ? 1 : 0, memory);
    if (rc != 0) {
      std::cerr << rl_last_error() << std::endl;
      return 1;
    }
    usage_line();
    return 0;
  }
  if (!opt.count("chunk_index") && mode != "OptimizeParameters") {
    std::cerr << "Not enough arguments supplied." << std::endl;
    std::cerr << "Needed: chunk_index, output." << std::endl;
    return 1;
  }
  if (mode == "FindEquivalentBranches") {  // pipeline/FindEquivalentBranches.cpp:13-167
    std::cerr << "---------------------------------------------------------" << std::endl;
    std::cerr << "Propagating mutations across AncesTrees..." << std::endl;
    if (rl_stage_find_equivalent_branches(out.c_str(), std::stoi(opt["chunk_index"])) != 0) {
      std::cerr << rl_last_error() << std::endl;
      return 1;
    }
    usage_line();
    return 0;
  }
  const int chunk = atoi(opt["chunk_index"].c_str());
  const int device = opt.count("device") ? atoi(opt["device"].c_str()) : 0;
  int sum_mode = RL_SUM_EXACT;
  if (opt.count("sum_mode")) {
    if (opt["sum_mode"] == "lanes") sum_mode = RL_SUM_LANES;
    else if (opt["sum_mode"] == "lanes32") sum_mode = RL_SUM_LANES32;
    else if (opt["sum_mode"] != "exact") {
      std::cerr << "--sum_mode must be exact, lanes or lanes32" << std::endl;
      return 1;
    }
  }
  int use_painting = 0;
  double theta = 0.001, rho = 1.0;
  if (opt.count("painting")) {  // Paint.cpp:38-61: "theta,rho" parsed with std::stof
    const std::string p = opt["painting"];
    const size_t c = p.find(',');
    if (c == std::string::npos) {
      std::cerr << "--painting expects theta,rho" << std::endl;
      return 1;
    }
    theta = std::stof(p.substr(0, c));
    rho = std::stof(p.substr(c + 1));
    use_painting = 1;
  }
  int rc;
  // every option of the stage in one struct, per call (include/relate_amd.h rl_stage_opts)
  rl_stage_opts so;
  rl_stage_opts_init(&so);
  so.sum_mode = sum_mode;
  so.device = device;
  so.use_painting = use_painting;
  so.theta = theta;
  so.rho = rho;
  so.flags = opt.count("no_consistency") ? 1 : 0;
  so.fb = opt.count("fb") ? (int)std::stof(opt["fb"]) : 0;  // BuildTopology.cpp:111-114
  const std::string ages = opt.count("sample_ages") ? opt["sample_ages"] : std::string();
  so.sample_ages_path = ages.empty() ? nullptr : ages.c_str();  // BuildTopology.cpp:93-108
  so.find_equivalent_branches = opt.count("find_equivalent_branches") ? 1 : 0;
  if (opt.count("paint_all_windows")) so.paint_windows = 0;  // (read by PaintBuildTopology alone)
  if (mode == "OptimizeParameters") {
    return optimize_parameters(opt, so);
  } else if (mode == "CopyingMatrix") {
    return copying_matrix(out, chunk, opt.count("first_section") ? atoi(opt["first_section"].c_str()) : 0,
                          opt.count("last_section") ? atoi(opt["last_section"].c_str()) : 1 << 30, so);
  } else if (mode == "Paint") {
    std::cerr << "---------------------------------------------------------" << std::endl;
    std::cerr << "Painting sequences..." << std::endl;
    rc = rl_stage_paint_ex(out.c_str(), chunk, &so);
    if (rc == 0) usage_line();
  } else if (mode == "PaintBuildTopology") {
    // Paint + BuildTopology of the chunk in one process, the stepping stones kept in HBM: what `--mode All` does per
    // chunk (Relate.cpp:257-283) without the paint files.  Sections default to all of the chunk's.
    rc = rl_stage_paint_build_topology_ex(out.c_str(), chunk, opt.count("first_section") ? atoi(opt["first_section"].c_str()) : 0,
                                          opt.count("last_section") ? atoi(opt["last_section"].c_str()) : 1 << 30, &so);
    if (rc == 1) return 1;
  } else if (mode == "BuildTopology") {
    if (!opt.count("first_section") || !opt.count("last_section")) {
      std::cerr << "Not enough arguments supplied." << std::endl;
      std::cerr << "Needed: first_section, last_section." << std::endl;
      return 1;
    }
    rc = rl_stage_build_topology_ex(out.c_str(), chunk, atoi(opt["first_section"].c_str()),
                                    atoi(opt["last_section"].c_str()), &so);
    if (rc == 1) return 1;  // first_section >= num_windows (BuildTopology.cpp:45)
  } else {
    std::cerr << "Mode " << mode << " is not part of this build: it replaces --mode MakeChunks, Paint, BuildTopology, FindEquivalentBranches, "
              << "OptimizeParameters, CoalescentRateForSection, FinalizePopulationSize, Frequency, Selection, AvgMutationRate, CoalRateForTree, SubTreesForSubpopulation, MutationRateWithContext and FinalizeMutationRate only; run the reference Relate for the other stages." << std::endl;
    return 1;
  }
  if (rc != 0) {
    std::cerr << "Error: " << rl_last_error() << std::endl;
    return 1;
  }
  return 0;
}

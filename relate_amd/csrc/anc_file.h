// anc_file.h -- the binary .anc file (AncesTree::DumpBin / ReadBin of the reference) in memory: read by
// FindEquivalentBranches (equivalent.cpp), which rewrites it, by CompareTopology (compare.cpp) and by
// PairwiseCoalescence (pairwise.cpp).
#pragma once
#include <string>
#include <vector>

namespace rl {

struct AncTree {
  int pos = 0;
  std::vector<int> parent, snp_begin, snp_end;
  std::vector<double> branch_length;
  std::vector<float> num_events;
  std::vector<int> child_left, child_right;  // as Tree::ReadTreeBin assigns them: first / second child in node order
};

struct AncFile {
  bool has_ages = false;
  unsigned N = 0;
  std::vector<double> ages;
  std::vector<AncTree> trees;
};

// AncesTree::ReadBin (src/anc.cpp:941-968) + Tree::ReadTreeBin (:83-125)
int read_anc(const std::string &fn, AncFile &a);
// AncesTree::DumpBin (src/anc.cpp:1104-1167)
int write_anc(const std::string &fn, const AncFile &a);
// the SNPs a file covers: [*first, *last], from its first tree's position to the largest SNP_end of its last tree (a
// tree covers from its position to the next tree's); RL_EFORMAT for a file without trees or with positions not rising
int anc_coverage(const AncFile &a, const char *fn, int *first, int *last);
// FindEquivalentBranches on a sequence in memory (equivalent.cpp): BranchAssociation of every pair of neighbours at
// N leaves, then AssociateTrees -- num_events and SNP_begin carried forward along equivalent branches, num_events and
// SNP_end back.  The trees carry child_left / child_right as the reference's trees would
void associate_sequence(std::vector<AncTree> &trees, int N);
// the header alone: haplotypes, trees, whether sample ages follow
int read_anc_header(const std::string &fn, unsigned *N, unsigned *trees, bool *has_ages);

}  // namespace rl

"""The inputs of the MutationRateWithContext tests (test_mutctx_cpu.py, test_mutctx_gpu.py) and of
tools/make_golden_mutctx.py.  Nothing here calls the library.  The trees come from tests/golden/coalrate_ref.npz (case
a: a real dated tree sequence, N = 8, 355 trees, with the rows of its real .mut; case c: 40 synthetic trees at N =
300); the positions, alleles, flanks, the ancestor and the mask come from an integer LCG, so no library's random stream
decides a byte of them.  tests/golden/mutctx_ref.npz holds what the reference's RelateMutationRate wrote for every
case (_mut.bin, _opp.bin, .rate) and what its CountBasesByType counted."""
import os

import numpy as np

import coalrate_cases as cc
import frequency_cases as fc
from frequency_cases import MUT_HEAD, max_times

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mutctx_ref.npz")
C96 = 96
# case -> the inputs it is made from, and (--bins, --years_per_gen, with a --dist file)
#   a, a2   the real trees; the first SNP above position 1001; the mask longer than the ancestor.  a2: other positions
#           and sequences: the second "chromosome" of the sum
#   s...    N = 300; the first SNP below position 1001; the mask shorter than the ancestor; --years_per_gen 8 puts the
#           boundaries 125 and 12,500,000 on floats (an age_begin on a boundary)
CASES = {"a": ("a", None, None, False), "a2": ("a2", None, None, False), "s": ("s", None, "8", False),
         "s_dist": ("s", None, "8", True), "s_bins": ("s", "2,6.5,0.5", "12.5", False)}
CHROMOSOMES = {"1": "a", "2": "a2"}  # the sum of FinalizeMutationRate: case `sum`


def fixture():
    return np.load(FIXTURE)


class Lcg:
    """x -> 1664525 x + 1013904223 mod 2^32 (Numerical Recipes); the upper bits are used"""

    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFF

    def below(self, n):
        self.x = (self.x * 1664525 + 1013904223) & 0xFFFFFFFF
        return (self.x >> 8) % n


def ancestor_sequence(n, seed):
    """ACGT with 7% lower case and 3% N"""
    g = Lcg(seed)
    out = []
    for _ in range(n):
        r, b = g.below(100), "ACGT"[g.below(4)]
        out.append("N" if r < 3 else (b.lower() if r < 10 else b))
    return "".join(out)


def mask_sequence(n, seed, main_at):
    """P, with 40 short runs of other characters (`p` among them: the reader upper-cases); a run of 6000 N from main_at
    with P at +480..+519 and +5480..+5519 (their windows reach the P outside the run: counted) and a single P at +3000
    (its window of 2002 holds 2001 others, above the main phase's threshold of 2000: not counted); and a run of N over
    [n - 2000, n - 700) with single P at n - 995 and n - 720, then 10 P, 10 N and P from n - 680: the tail phase's
    count is above its threshold of 1000 up to the second run and below it from n - 680"""
    g = Lcg(seed)
    m = ["P"] * n
    for _ in range(40):
        at, ln, ch = g.below(n), 1 + g.below(25), "NCnp0"[g.below(5)]
        m[at:at + ln] = [ch] * len(m[at:at + ln])
    m[main_at:main_at + 6000] = ["N"] * 6000
    for off in list(range(480, 520)) + list(range(5480, 5520)) + [3000]:
        m[main_at + off] = "P"
    m[n - 2000:n - 400] = ["N"] * 1300 + ["P"] * 10 + ["N"] * 10 + ["P"] * 280
    for off in (995, 720):
        m[n - off] = "P"
    return "".join(m)


def main_run_at(anc_len):
    """where the mask's run of 6000 starts"""
    return (anc_len // 2000) * 1000 - 1000


def fasta_text(name, seq, width=60):
    return (">" + name + "\n" + "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))).encode()


def case_trees(src):
    """-> (N, trees [(pos, parent, bl)], .anc bytes)"""
    co = cc.fixture()
    if src in ("a", "a2"):
        anc = co["a/anc"].tobytes()
        N, parents, bl = cc.parse_anc_text(anc)
        return N, [(0, p, b) for p, b in zip(parents, bl)], anc
    N, trees = fc.case_s_rows(co)
    return N, trees, cc.anc_text(N, trees)


def base_rows(src, N, trees):
    """[(tree, branches, flipped, age_begin, age_end)]: the rows of case a's real .mut, or six SNPs on LCG-chosen
    branches of every synthetic tree but those of trees 7, 8 and 21 (trees without a SNP between trees with one)"""
    if src in ("a", "a2"):
        rows = []
        for ln in cc.fixture()["a/mut"].tobytes().decode().splitlines()[1:]:
            f = ln.split(";")
            rows.append((int(f[4]), [int(b) for b in f[5].split()], int(f[7]), float(f[8]), float(f[9])))
        return rows[::2] if src == "a2" else rows
    g = Lcg(300)
    rows = []
    for t, (_, parent, bl) in enumerate(trees):
        if t in (7, 8, 21):
            continue
        times = max_times(parent, bl)
        for _ in range(6):
            b = g.below(2 * N - 2)
            rows.append((t, [b], 0, float(times[b]), float(times[parent[b]])))
    return rows


def make_case(src):
    """-> dict(N, trees, anc, mut, dist, ancestor, mask: the files' bytes; rows: the SNPs as the .mut holds them)"""
    N, trees, anc = case_trees(src)
    seed = {"a": 11, "a2": 29, "s": 47}[src]
    g = Lcg(seed)
    rows = base_rows(src, N, trees)
    gap = 30 if src == "s" else 5
    pos, p = [], {"a": 1203, "a2": 1001, "s": 412}[src]
    for _ in rows:
        pos.append(p)
        p += gap + g.below(6 * gap)
    anc_len = pos[-1] + 4
    mask_len = anc_len - 37 if src == "s" else anc_len + 500
    seq = ancestor_sequence(anc_len, seed + 1)
    main_at = main_run_at(anc_len)
    for at in (main_at + 3000, mask_len - 995, mask_len - 720):  # nucleotides under the single P of the runs
        seq = seq[:at - 1] + "CAg" + seq[at + 2:]
    mask = mask_sequence(mask_len, seed + 2, main_at)
    roots = [float(max_times(parent, bl)[-1]) for _, parent, bl in trees]
    out = []
    for k, (tree, br, flipped, a0, a1) in enumerate(rows):
        x = seq[pos[k]].upper()
        x = x if x in "ACGT" else "A"
        y = "ACGT".replace(x, "")[g.below(3)]
        up, down = seq[pos[k] - 1].upper(), seq[pos[k] + 1].upper()
        up, down = (up if up in "ACGT" else "ACGT"[g.below(4)]), (down if down in "ACGT" else "ACGT"[g.below(4)])
        tail = "%s/%s;%s;%s;" % (x, y, up, down)
        kind = k % 23
        if kind == 0 and len(br) == 1:
            br = [br[0], (br[0] + 1) % (2 * N - 2)]  # several branches
        elif kind == 1:
            flipped = 1
        elif kind == 2:
            tail = "%s/%s;NA;NA;" % (x, y)
        elif kind == 3:
            tail = "%s/%s;%s;%s;" % (x, x, up, down)  # equal alleles
        elif kind == 4:
            tail = "%s/N;%s;%s;" % (x, up, down)  # an allele outside ACGT
        elif kind == 5:
            tail = "%s/%s;N;%s;" % (x, y, down)  # a flank outside ACGT: category 0
        elif kind == 6:
            a1 = float(np.float32(roots[tree] * 1.5 + 1.0))  # age_end above the root's time: the clamp
        elif kind == 7 and a0 < 125.0 < a1:
            a0 = 125.0  # (with --years_per_gen 8: on the boundary of epochs 0 and 1)
        elif kind == 8:
            tail = ""  # neither alleles nor flanks
        elif kind == 9:
            tail = "%s/%s;" % (x, y)  # no flanks
        elif kind == 10:
            tail = "%s/%s;%s;%s;3;5;" % (x, y, up, down)  # with frequencies behind the flanks
        dist = pos[k + 1] - pos[k] if k + 1 < len(rows) else 1
        out.append((pos[k], dist, tree, br, flipped, a0, a1, tail))
    mut = (MUT_HEAD + "".join("%d;%d;%d;rs%d;%d;%s;%d;%d;%s;%s;%s\n" % (
        k, p_, d, k, t, " ".join(str(b) for b in br), len(br) != 1, fl, repr(a0), repr(a1), tail)
        for k, (p_, d, t, br, fl, a0, a1, tail) in enumerate(out))).encode()
    # the --dist file: positions the .mut lacks in front of, between and behind its own
    lines = ["#pos dist", "%d %d" % (pos[0] - 300, 200), "%d %d" % (pos[0] - 100, 100)]
    for k, p_ in enumerate(pos):
        nxt = pos[k + 1] if k + 1 < len(pos) else p_ + 2
        if nxt - p_ >= 2 and g.below(3) == 0:
            cut = 1 + g.below(nxt - p_ - 1)
            lines += ["%d %d" % (p_, cut), "%d %d" % (p_ + cut, nxt - p_ - cut)]
        else:
            lines.append("%d %d" % (p_, nxt - p_))
    lines.append("%d %d" % (pos[-1] + 2, 1))
    return dict(N=N, trees=trees, anc=anc, mut=mut, dist=("\n".join(lines) + "\n").encode(),
                ancestor=fasta_text("ancestor", seq), mask=fasta_text("mask", mask), rows=out)


_made = {}


def case_inputs(key):
    """the files of a fixture case (made once per process) and its options"""
    src, bins, ypg, with_dist = CASES[key]
    if src not in _made:
        _made[src] = make_case(src)
    return _made[src], bins, ypg, with_dist


def write_inputs(folder, prefix, c):
    """prefix.anc / .mut / .dist / _ancestor.fa / _mask.fa in folder"""
    for ext, name in ((".anc", "anc"), (".mut", "mut"), (".dist", "dist"), ("_ancestor.fa", "ancestor"), ("_mask.fa", "mask")):
        with open(os.path.join(str(folder), prefix + ext), "wb") as f:
            f.write(c[name])


def cli_options(prefix, key):
    """the options both programs take for a case, behind -i and -o"""
    _, bins, ypg, with_dist = CASES[key]
    return ["--mask", prefix + "_mask.fa", "--ancestor", prefix + "_ancestor.fa"] + (["--bins", bins] if bins else []) \
        + (["--years_per_gen", ypg] if ypg else []) + (["--dist", prefix + ".dist"] if with_dist else [])


def mut_columns(c):
    """-> (snp_pos [L], one_branch [L]) of a case's .mut"""
    return (np.array([r[0] for r in c["rows"]], np.int32), np.array([len(r[3]) == 1 for r in c["rows"]], np.uint8))


def dist_positions(c):
    return np.array([int(ln.split()[0]) for ln in c["dist"].decode().splitlines()[1:]], np.int32)


def counts_key(key):
    """the case under which the fixture holds a case's counts: they depend on the files, not on the epochs"""
    return "s" if key == "s_bins" else key


def dense_counts(fx, key):
    """the harness's counts of a case -> [L][96] uint32"""
    L = int(fx[key + "/snps"][0])
    key = counts_key(key)
    out = np.zeros(L * C96, np.uint32)
    out[np.cumsum(fx[key + "/count_step"].astype(np.int64))] = fx[key + "/count"]
    return out.reshape(L, C96)


def owner(snp_pos, base):
    """the SNP between whose midpoints to its neighbours a base lies (the .mut's positions as the list)"""
    mids = 0.5 * (snp_pos[:-1].astype(np.float64) + snp_pos[1:])
    return int(np.searchsorted(mids, base, side="right"))

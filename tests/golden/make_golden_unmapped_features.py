#!/usr/bin/env python3
"""Generate tests/golden/unmapped_features/ by running the REFERENCE's own ``generate_featureFiles`` and ``get_precursors``
(mirge/libs/generate_featureFiles.py, with mirge/classes/readCluster.py) on a genome and on ``<sample>_modified_selected_sorted.tsv``
tables made here, the way make_golden_unmapped_align.py made tests/golden/unmapped_align/.

Runs only where the reference checkout exists (never on the GPU box, never from a test); what is committed is data: the genome
FASTA, the input tables and the three files per sample the reference's functions wrote.  No reference source is copied.

Recipe:
  * the input tables are built directly, one cluster per condition listed in KINDS below (at least two of each on S1): the step
    under test starts from the table, not from the runs that make it in a pipeline.  A cluster's sequence is the genome's at its
    coordinates (reverse-complemented on '-'), its reads are windows of that stretch and its flanks with the changes named;
  * Bio stand-ins (tests/golden/stubs): ``Seq.reverse_complement`` and ``Seq.transcribe`` are given minimal bodies here, at
    generation time; ``Bio.pairwise2`` is the committed stand-in;
  * every row is asserted to reach its best score on ONE diagonal (the stand-in's ``diagonals_at_best``), so the committed bytes do
    not depend on the order in which pairwise2 lists equal alignments, and to satisfy ``best > 2 * min(L, C) - 20``: the fixture
    has no row a gap could win.

usage: python tests/golden/make_golden_unmapped_features.py
"""
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_unmapped as front  # noqa: E402  (paths, the stand-in modules)
import numpy as np  # noqa: E402

rc = front.rc
import Bio.Seq  # noqa: E402
from Bio import pairwise2  # noqa: E402
Bio.Seq.Seq.reverse_complement = lambda self: Bio.Seq.Seq(rc(str(self)))
Bio.Seq.Seq.transcribe = lambda self: Bio.Seq.Seq(str(self).replace("T", "U").replace("t", "u"))
from mirge.classes.readCluster import ReadCluster  # noqa: E402  (the reference)
from mirge.libs.generate_featureFiles import generate_featureFiles, get_precursors  # noqa: E402  (the reference)

OUT = os.path.join(HERE, "unmapped_features")
SAMPLES = ["S1", "S2"]
FLANK = 8
FULL = ((0, 24, 12), (0, 22, 3), (2, 22, 3))  # (shift, length, count[, changes]): every column of a 24-nt cluster at 0.8 or more
KINDS = ("plus", "minus", "low_count", "few_rows", "near_start", "near_end", "no_stable", "short_stable", "head_pad", "head_no_pad",
         "tail_pad", "tail_no_pad", "tail_minus1", "overhang_head", "overhang_tail", "mismatch", "read_N", "base_tie", "majority_tie",
         "Good", "Bad_strand", "Bad_distance", "Null", "clamped_precursor", "repeated_name")


def make_genome(rng):
    names = ["chr1", "chr2", "chr10", "chr3", "chr4", "chr5"]  # sorted as strings: chr1 < chr10 < chr2
    refs = ["".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=3000 if n in ("chr4", "chr5") else 10000)) for n in names]
    refs[0] = refs[0][:2950] + "N" * 12 + refs[0][2962:]  # inside the precursor windows of the clusters at 3000
    return names, refs


class Table:
    def __init__(self, sample, genome):
        self.sample, self.genome, self.lines, self.n, self.k = sample, genome, [], 0, 0
        self.tags = {}

    def cluster(self, tag, chrom, start, strand="+", reads=FULL, length=24, scale=1):
        """one cluster at [start, start + length) (1-based, inclusive end) with its rows"""
        ref = self.genome[chrom]
        end = start + length - 1
        lo = start - 1 - FLANK
        assert lo >= 0 and end + FLANK <= len(ref)
        ext = ref[lo:end + FLANK]
        ext = rc(ext) if strand == "-" else ext
        cseq = ext[FLANK:FLANK + length]
        self.k += 1
        name = f"{self.sample}:miRCluster_{self.k}_{length}:{chrom}:{start}_{end}{strand}"
        self.tags.setdefault(tag, []).append(name)
        self.rows(name, cseq, ext, reads, scale)
        return name, cseq, ext

    def rows(self, name, cseq, ext, reads, scale=1):
        for r in reads:
            shift, ln, count = r[:3]
            s = list(ext[FLANK + shift:FLANK + shift + ln])
            for at, ch in (r[3] if len(r) > 3 else ()):  # a letter, or k: the k-th next base of ACGT
                ch = other(s[at], ch) if isinstance(ch, int) else ch
                assert s[at] != ch
                s[at] = ch
            s = "".join(s)
            self.n += 1
            count *= scale
            self.lines.append("\t".join([f"mir{self.n}_{count}", str(count), s, cseq, "0", name, str(max(1, shift + 1)), "255", f"{ln}M", "*", "0",
                                         "0", s, "I" * ln, "NM:i:0"]) + "\n")


def other(ch, k=1):
    return "ACGT"[("ACGT".index(ch) + k) % 4]


def build(sample, genome, small=False):
    t = Table(sample, genome)
    sc = 2 if small else 1
    # chr1: seven clusters with a stable head and tail.  A, B: 30 apart on one strand (Good).  C (+), D (-), E (-): C and D 30 apart
    # on different strands, D and E 5 apart (Bad by strand, Bad by distance).  F, G: far from everything (Null)
    t.cluster("A", "chr1", 1000, scale=sc)
    t.cluster("B", "chr1", 1054, scale=sc)
    t.cluster("C", "chr1", 3000, scale=sc)
    t.cluster("D", "chr1", 3054, "-", scale=sc)
    t.cluster("E", "chr1", 3083, "-", scale=sc)
    # F: reads that start late and end early: 3 unstable columns in front, 6 behind: no padding on either side
    t.cluster("F", "chr1", 5000, reads=((3, 15, 9), (3, 14, 6), (0, 24, 2), (2, 18, 1)), scale=sc)
    t.cluster("G", "chr1", 7000, "-", reads=((4, 14, 8), (4, 13, 7), (0, 24, 2), (1, 20, 1)), scale=sc)
    if small:
        t.cluster("lone", "chr2", 4000, "-", scale=sc)
        return t
    # chr4: one cluster with a stable head and tail; chr5: two (44 apart: still Good; 45 would be Null); chr10: the rejected ones
    t.cluster("lone", "chr4", 1500, "-", reads=((0, 24, 7), (0, 23, 7), (1, 23, 4)))
    t.cluster("pair1", "chr5", 2000)
    t.cluster("pair2", "chr5", 2068, reads=((0, 24, 7), (0, 22, 7), (2, 22, 4)))  # two reads share the top count: the larger row wins
    for k in (0, 1):
        t.cluster("low_count", "chr10", 3000 + 300 * k, reads=((0, 24, 4), (0, 22, 3), (2, 22, 2)))
        t.cluster("few_rows", "chr10", 4000 + 300 * k, "-" if k else "+", reads=((0, 24, 40), (1, 22, 30)))
        t.cluster("near_start", "chr10", 12 + 8 * k)  # start 12 and 20: not > 20
        t.cluster("near_end", "chr10", 10000 - 20 - 23 + 5 * k)  # end 9980 and 9985: not < 10000 - 20
        t.cluster("no_stable", "chr10", 5000 + 300 * k, "-" if k else "+", length=30, reads=((0, 16, 4), (16, 14, 4), (8, 16, 4)))
        t.cluster("short_stable", "chr10", 6000 + 300 * k, "-" if k else "+", reads=((0, 15, 4), (9, 15, 4), (4, 16, 4)))
    # chr2: clusters with reads that overhang, differ and carry N; a lone stretch of them, far apart
    for k, strand in enumerate("+-"):
        t.cluster("overhang", "chr2", 1000 + 500 * k, strand, reads=((-3, 25, 6), (0, 27, 5), (-2, 28, 4), (0, 24, 3)))
        t.cluster("mismatch", "chr2", 3000 + 500 * k, strand,
                                 reads=((0, 24, 9), (0, 24, 3, ((10, 1),)), (1, 22, 2, ((0, "N"),)), (0, 23, 2, ((15, "N"),))))
        # column 23 is covered by two reads of equal count with different bases: the majority base is the tie rule's
        t.cluster("base_tie", "chr2", 5000 + 500 * k, strand,
                                 reads=((0, 24, 5, ((23, 1 + k),)), (0, 24, 5), (0, 23, 6), (1, 22, 4)))
    # chr3: one cluster near the start: its first precursor window clamps at base 0, its template window does not; and a name that
    # comes twice in the table with another cluster of the chromosome between its rows (two entries, both with features)
    t.cluster("clamped", "chr3", 40)
    t.cluster("clamped", "chr3", 60, "-", reads=((0, 24, 9), (0, 22, 5), (3, 21, 4)))
    name, cseq, ext = t.cluster("repeated", "chr3", 2000)
    t.cluster("between", "chr3", 2500)
    t.rows(name, cseq, ext, ((0, 23, 6), (1, 23, 5), (1, 22, 4)))
    name, cseq, ext = t.cluster("repeated", "chr3", 4000, "-")
    t.cluster("between", "chr3", 4500, "-")
    t.rows(name, cseq, ext, ((0, 24, 6), (2, 22, 5), (1, 22, 4)))
    return t


def ungapped_best(a, b):
    best = 0
    for d in range(-(len(b) - 1), len(a)):
        h = 0
        for i in range(max(0, d), min(len(a), len(b) + d)):
            h = max(0, h + (2 if a[i] == b[i - d] else -1))
            best = max(best, h)
    return best


def check(sample, table, chr_seq, chr_len):
    """the conditions on S1, from the reference's own objects and the files it wrote"""
    kinds = dict.fromkeys(KINDS, 0)
    groups = {}
    order = []
    for line in table.lines:
        f = line.rstrip("\n").split("\t")
        ds = pairwise2.align.diagonals_at_best(f[3], f[2], 2, -1, -20, -20)
        assert len(ds) == 1, (f[5], f[2], ds)
        assert ungapped_best(f[3], f[2]) > 2 * min(len(f[2]), len(f[3])) - 20, (f[5], f[2])
        if not order or order[-1] != f[5]:
            order.append(f[5])
            groups[len(order) - 1] = (f[5], f[3], [], [], [])
        g = groups[len(order) - 1]
        g[2].append(f[0]); g[3].append(f[2]); g[4].append(int(f[1]))
    feat = open(os.path.join(OUT, f"{sample}_features.tsv")).read().split("\n")
    head = feat[0].split("\t")
    in_feat = [ln.split("\t") for ln in feat[1:] if ln]
    feat_names = [f[5] for f in in_feat]
    in_cluster_txt = [ln[len("Cluster Name: "):] for ln in open(os.path.join(OUT, f"{sample}_cluster.txt")).read().split("\n")
                      if ln.startswith("Cluster Name: ")]
    for name, cseq, names, seqs, counts in groups.values():
        chrom, span, strand = name.split(":")[2], name.split(":")[3][:-1].split("_"), name[-1]
        start, end = int(span[0]), int(span[1])
        if sum(counts) < 10:
            kinds["low_count"] += 1
            continue
        if len(seqs) < 3:
            kinds["few_rows"] += 1
            continue
        if not start > 20:
            kinds["near_start"] += 1
            continue
        if not end < chr_len[chrom] - 20:
            kinds["near_end"] += 1
            continue
        inst = ReadCluster(chr_seq, chrom, strand, start, end, name, cseq, names, seqs, counts)
        rows, _, padded, _, _, ratios, h, t = inst.locateStartPosition()
        if h is None or t is None:
            kinds["no_stable"] += 1
            assert name not in in_cluster_txt
            continue
        assert name in in_cluster_txt
        if name not in feat_names:
            kinds["short_stable"] += 1
            continue
        kinds["plus" if strand == "+" else "minus"] += 1
        kinds["head_pad" if h < 3 else "head_no_pad"] += 1
        kinds["tail_pad" if -t - 1 < 6 else "tail_no_pad"] += 1
        kinds["tail_minus1"] += t == -1
        kinds["overhang_head"] += padded.startswith("-")
        kinds["overhang_tail"] += padded.endswith("-")
        kinds["mismatch"] += any(a != b and "-" not in (a, b) and b != "N" for r in rows[1:] for a, b in zip(padded, r))
        kinds["read_N"] += any("N" in s for s in seqs)
        for i in range(len(padded)):
            n = {x: sum(c for r, c in zip(rows[1:], counts) if r[i] == x) for x in "ATCG"}
            top = sorted(n.values(), reverse=True)
            if top[0] == top[1] and top[0] > 0:
                kinds["base_tie"] += 1
                break
        top = sorted(zip(counts, rows[1:]), reverse=True)
        kinds["majority_tie"] += top[0][0] == top[1][0] and top[0][1] != top[1][1]
    k_state, k_up, k_down = head.index("neighborState"), head.index("upstreamDistance"), head.index("downstreamDistance")
    for f in in_feat:
        near = [int(x) for x in (f[k_up], f[k_down]) if x != "None"]
        if f[k_state] == "Bad":
            kinds["Bad_strand"] += any(9 <= d <= 44 for d in near)
            kinds["Bad_distance"] += any(d < 9 for d in near)
        else:
            kinds[f[k_state]] += 1
    assert {"None"} < {f[k_up] for f in in_feat} and {"None"} < {f[k_down] for f in in_feat}
    per_chr = {}
    for name in dict.fromkeys(in_cluster_txt):
        per_chr[name.split(":")[2]] = per_chr.get(name.split(":")[2], 0) + in_cluster_txt.count(name)
    assert {1, 2} <= set(per_chr.values()) and max(per_chr.values()) >= 3, per_chr
    kinds["repeated_name"] = sum(1 for n in set(feat_names) if feat_names.count(n) > 1)
    fa = open(os.path.join(OUT, f"{sample}_precursor.fa")).read().split("\n")
    heads = [ln for ln in fa if ln.startswith(">")]
    assert len(heads) == len(set(heads)) == 2 * len(set(feat_names))
    k_tpl, k_hu = head.index("templateSeq"), head.index("headUnstableLength")
    for f in in_feat:
        span = f[5].split(":")[3][:-1].split("_")
        if int(span[0]) - 1 - 70 + int(f[k_hu]) < 0 and len(f[k_tpl]) == len(f[head.index("adjustedClusterSeq")]):
            kinds["clamped_precursor"] += 1
    assert any("N" in ln for ln in fa if not ln.startswith(">")), "no precursor window over the ambiguous stretch"
    for k in KINDS:
        assert kinds[k] >= 2, (k, kinds)
    return kinds


def main():
    rng = np.random.default_rng(33)
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    names, refs = make_genome(rng)
    with open(os.path.join(OUT, "genome.fa"), "w") as fh:
        fh.write("".join(f">{n}\n{r}\n" for n, r in zip(names, refs)))
    chr_seq = dict(zip(names, refs))
    chr_len = {n: len(r) for n, r in chr_seq.items()}
    for s in SAMPLES:
        table = build(s, chr_seq, small=s != "S1")
        with open(os.path.join(OUT, f"{s}_modified_selected_sorted.tsv"), "w") as fh:
            fh.write("".join(table.lines))
        generate_featureFiles(OUT, s, chr_seq, chr_len, {}, {})
        n_pre = get_precursors(OUT, s, chr_seq)
        kinds = check(s, table, chr_seq, chr_len) if s == "S1" else {}
        n_rows = open(os.path.join(OUT, f"{s}_features.tsv")).read().count("\n") - 1
        n_txt = open(os.path.join(OUT, f"{s}_cluster.txt")).read().count("Cluster Name: ")
        print(f"{s}: {len(table.lines)} rows, {table.k} clusters, {n_txt} in _cluster.txt, {n_rows} feature rows, {n_pre} precursors {kinds}")


if __name__ == "__main__":
    main()

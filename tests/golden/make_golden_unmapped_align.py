#!/usr/bin/env python3
"""Generate tests/golden/unmapped_align/ by running the REFERENCE's own ``preTrimClusteredSeq`` (mirge/libs/novel_mir.py:152),
``split_fasta_from_sam``, ``combineSam``, ``decorateSam`` and ``parse_refine_sam`` (mirge/libs/processSam.py) on a frame made
here, the way make_golden_unmapped.py made tests/golden/unmapped/.

Runs only where the reference checkout exists (never on the GPU box, never from a test); what is committed is data: the inputs
(per-sample FASTA, genome SAM, <sample>_clusters.tsv, the repeat intervals as text) and the files the reference's functions
wrote.  No reference source is copied.

Recipe:
  * the frame is larger than tests/golden/unmapped's (13 clusters there): a genome of four chromosomes with one locus per
    condition below, three reads piled on each, and reads planted for the second cluster run.  ``convert2Fasta`` and
    ``cluster_basedon_location`` (the reference's) make the FASTA files and <sample>_clusters.tsv from it as in
    make_golden_unmapped.py: the genome run is the stand-in bowtie, -m is not applied to it, so the locus copied four times
    becomes four clusters and its reads are over -m in the first cluster run;
  * novel_mir.py's unused imports are empty stand-in modules as before -- but scipy is the real one: the repeat table is
    {chromosome: [[cKDTree over (start, 0)], [(start, end, name), ...]]}, built here from repeats.txt; the pickle is not
    committed, tests rebuild it from that text;
  * Bio stand-ins: ``Seq.reverse_complement`` and ``SeqIO.parse`` are given minimal bodies here, at generation time;
  * the two cluster runs: tests/golden/fake_bowtie/bowtie in its default-output mode on the cluster FASTA copied to <index>.fa.
    It lists every alignment and does not read -l or -m, so run 1 is asked as the reference asks it (-n 0: exact) and -m is
    applied HERE; run 2 is asked for every alignment with at most two mismatches (-v 2 -5 1 -3 3 --norc) and the policy of
    ``-n 1 -l 15`` (at most one mismatch in the first 15 bases, two in all) and the stratum rule (a stratum = the mismatches in
    the seed; only the best one is kept) are applied HERE from the mismatch descriptors.  SAM lines are written HERE in
    ``unmapped_align.cluster_sam_text``'s format: reads in FASTA order, a read's alignments by (reference, offset), flag 4 in
    place.  The fixture pins the reference's Python around these files, not bowtie;
  * the two sorted tables are ``LC_ALL=C sort -k6,6 -k1,1``;
  * the long files that follow from the committed ones (HASHED below) are committed as SHA-256 sums in derived.sha256: a test
    compares the bytes it produced with the sum.

"Best stratum 1 with a worse alignment elsewhere that must be dropped": under -n 1 the strata are 0 and 1, so an alignment
of a worse stratum exists only beside a best stratum of 0.  The frame has both halves: reads whose best stratum is 1, and
reads with a stratum-0 alignment and a stratum-1 alignment elsewhere, which is dropped.

usage: python tests/golden/make_golden_unmapped_align.py
"""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scipy.spatial  # noqa: E402,F401  (first: make_golden_unmapped replaces modules it has not seen by empty stand-ins, scipy among them)
from scipy.spatial import cKDTree  # noqa: E402
import make_golden_unmapped as front  # noqa: E402  (paths, the stand-in modules, the reference's convert2Fasta / cluster_basedon_location)
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

rc, default_lines_to_sam, convert2Fasta, cluster_basedon_location = front.rc, front.default_lines_to_sam, front.convert2Fasta, \
    front.cluster_basedon_location


def _fasta_records(path, fmt="fasta"):
    out = []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if line.startswith(">"):
                out.append(types.SimpleNamespace(id=line[1:].split()[0], seq=""))
            elif out:
                out[-1].seq += line
    return out


import Bio.Seq  # noqa: E402
import Bio.SeqIO  # noqa: E402
Bio.Seq.Seq.reverse_complement = lambda self: rc(str(self))
Bio.SeqIO.parse = _fasta_records
from mirge.libs.novel_mir import preTrimClusteredSeq  # noqa: E402  (the reference)
from mirge.libs.processSam import combineSam, decorateSam, parse_refine_sam, split_fasta_from_sam  # noqa: E402  (the reference)

OUT = os.path.join(HERE, "unmapped_align")
FAKE = os.path.join(HERE, "fake_bowtie", "bowtie")
SAMPLES = ["S1", "S2"]
MINL, MAXL, CUTOFF, MLOC, SEEDLEN, OLC, CLC = 16, 25, 2, 3, 25, 14, 30  # mirge/libs/parse.py:130-136
SPACING = 300
PILE3 = ((0, 2, 4), (22, 21, 20))
PILE, PILE_LONG, PILE_26 = ((0, 4), (22, 20)), ((0, 8), (22, 23)), ((0, 4), (22, 22))  # clusters of 24, 31 and 26 nt
# S2 is a small second sample (its own cluster numbers, its own kept set): the reads of these loci and planted kinds only.  The
# conditions below are asserted on S1.
S2_LOCI = ("kept1", "kept2", "long1", "nearest1", "minus1", "absent1", "dup1", "dup2", "quad1", "quad2", "quad3", "quad4", "one_hit")
S2_PLANTED = ("stratum0", "two_best", "unaligned")
# files that are long and follow from the others: committed as their SHA-256 (derived.sha256), not as text
HASHED = ("{s}.sam", "{s}_modified.sam", "{s}_RepSeq_modified.sam", "{s}_selected.tsv", "{s}_selected_reverseKept.tsv",
          "{s}_modified_selected_reverseKept_sorted.tsv", "{s}_imperfectMath2Cluster.fa")
HASHED_S2 = ("{s}_modified_selected_sorted.tsv",)  # the small second sample: this one as a sum as well


def mut(s, *at):
    s = list(s)
    for k in at:
        s[k] = "ACGT"[("ACGT".index(s[k]) + 1) % 4]
    return "".join(s)


def make_frame(rng):
    names = ["chr1", "chr2", "chr3", "chr4"]
    refs = {n: list("".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=9000))) for n in names}
    nxt = {n: SPACING for n in names}
    loci, repeats, rows = {}, [], {}

    def place(tag, chrom, minus=False, pile=PILE, seq=None):
        at = nxt[chrom]
        nxt[chrom] += SPACING
        if seq is not None:
            refs[chrom][at:at + len(seq)] = seq
        loci[tag] = (chrom, at, minus, pile)
        if chrom in ("chr1", "chr2"):  # a background element between this locus and the next: never overlaps, never a tie
            repeats.append((chrom, at + 1 + 140, at + 1 + 160, f"bg_{tag}"))
        return at

    def window(chrom, at, n):
        return "".join(refs[chrom][at:at + n])

    for k in range(1, 5):
        place(f"kept{k}", "chr1" if k % 2 else "chr2")
    for k, ch in ((1, "chr1"), (2, "chr2")):
        place(f"long{k}", ch, pile=PILE_LONG)
        at = place(f"polyA{k}", ch)
        refs[ch][at + 18:at + 24] = "AAAAAA"
        at = place(f"polyT{k}", ch)
        refs[ch][at:at + 6] = "TTTTTT"
        at = place(f"nearest{k}", ch)
        repeats.append((ch, at + 1 + 3, at + 1 + 60, f"LINE_near{k}"))
        at = place(f"second{k}", ch)
        repeats += [(ch, at + 1 + 40, at + 1 + 70, f"SINE_beside{k}"), (ch, at + 1 - 90, at + 1 + 5, f"LTR_second{k}")]
    place("minus1", "chr1", minus=True)
    place("minus2", "chr2", minus=True)
    place("minus4", "chr4", minus=True)
    at = place("one_hit", "chr3")
    repeats.append(("chr3", at + 1 + 2, at + 1 + 30, "tRNA_only"))
    place("one_free1", "chr3")
    for k in range(1, 3):
        place(f"absent{k}", "chr4")
    dup = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=30))
    place("dup1", "chr1", pile=PILE3, seq=dup)  # three reads in two clusters
    place("dup2", "chr2", pile=PILE3, seq=dup)
    quad = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=30))
    for k, ch in enumerate(("chr1", "chr2", "chr4", "chr1")):
        place(f"quad{k + 1}", ch, pile=PILE3, seq=quad)  # three reads over -m
    p = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=30))
    place("pairP", "chr1", seq=p)
    place("pairP_1mm", "chr2", seq=mut(p, 8))
    a = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=30))
    place("totalA", "chr1", pile=PILE_26, seq=a)
    place("totalB", "chr2", pile=PILE_26, seq=mut(a, 6, 18, 20))
    u = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=12))
    place("tandem", "chr1", seq=u + u)

    def put(seq, c1, c2):
        assert seq not in rows, seq
        rows[seq] = (c1, c2)

    for tag, (chrom, at, minus, (shifts, lens)) in loci.items():
        for sh, ln in zip(shifts, lens):
            w = window(chrom, at + sh, ln)
            if (rc(w) if minus else w) in rows:
                continue  # the copies of one locus share their reads
            c2 = int(rng.integers(2, 30)) if tag in S2_LOCI else 0
            put(rc(w) if minus else w, int(rng.integers(2, 40)), c2)
    planted = {}

    def plant(kind, seq):
        put(seq, int(rng.integers(2, 20)), int(rng.integers(2, 20)) if kind in S2_PLANTED else 0)
        planted.setdefault(kind, []).append(seq)

    for k, ln in ((1, 16), (2, 19), (3, 22)):  # exact only after -5 1 -3 3
        s = window(*loci[f"kept{k}"][:2], 24)
        plant("stratum0", mut(s[0:ln], 0))
        plant("stratum0", mut(s[1:1 + ln], ln - 1))
        plant("stratum0", mut(s[2:24], 0, 19, 21))
    for k, (ln, at) in ((4, (22, 6)), (1, (20, 3)), (2, (18, 10))):  # one mismatch in the seed, nothing better anywhere
        s = window(*loci[f"kept{k}"][:2], 24)
        plant("stratum1", mut(s[1:1 + ln], at))
    for sh in (0, 1, 2):
        plant("worse_dropped", mut(p[sh:sh + 22], 0))  # exact at pairP, one seed mismatch at pairP_1mm
        plant("two_best", mut(dup[sh:22 - sh], 0))
    b = mut(a, 6, 18, 20)
    r = a[:18] + b[18] + a[19] + b[20] + a[21:]  # against A: two mismatches past the seed; against B: one in the seed
    for lo, hi in ((0, 25), (0, 24), (1, 26)):
        plant("total_in_worse_stratum", r[lo:hi])
    plant("tandem", mut(u[11], 0) + u + mut(u[:3], 0, 1, 2))  # 12 nt after trimming, twice in one cluster
    for ln in (16, 18, 20, 25):
        plant("unaligned", "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=ln)))
    seqs = sorted(rows)  # the sorted union of several samples (digest.py:243)
    return names, ["".join(refs[n]) for n in names], seqs, np.array([rows[s] for s in seqs], dtype=np.int64), repeats, planted


def repeat_table(repeats):
    table = {}
    for chrom, start, end, name in repeats:
        table.setdefault(chrom, [[], []])[1].append((start, end, name))
    for chrom in table:
        table[chrom][0] = [cKDTree([(e[0], 0) for e in table[chrom][1]])]
    return table


def fake_alignments(index, fasta, policy):
    """{read: [(reference order, offset, reference, printed sequence, [mismatch offsets])]} from the stand-in's default output"""
    r = subprocess.run([sys.executable, FAKE, index, fasta, "-f"] + policy + ["-a", "--norc", "--threads", "1"], check=True,
                       capture_output=True, text=True)
    out = {}
    for line in r.stdout.split("\n"):
        f = line.split("\t")
        if f == [""]:
            continue
        assert f[1] == "+"
        mm = [int(d.split(":")[0]) for d in f[7].split(",")] if len(f) > 7 and f[7] else []
        out.setdefault(f[0], []).append((f[2], int(f[3]), f[4], mm))
    return out


def write_cluster_sam(path, q_names, q_seqs, hits, c_names, c_lens, command, trim5=0, trim3=0, capped=()):
    order = {n: k for k, n in enumerate(c_names)}
    out = ["@HD\tVN:1.0\tSO:unsorted"] + [f"@SQ\tSN:{n}\tLN:{ln}" for n, ln in zip(c_names, c_lens)]
    out.append(f"@PG\tID:mirge3.0_amd\tPN:mirge_genome_align_loci\tCL:\"{command}\"")
    for n, full in zip(q_names, q_seqs):
        s = full[trim5:len(full) - trim3]
        mine = sorted(hits.get(n, []), key=lambda h: (order[h[0]], h[1]))
        for ref, off, printed, mm in mine:
            assert printed == s
            out.append(f"{n}\t0\t{ref}\t{off + 1}\t255\t{len(s)}M\t*\t0\t0\t{s}\t{'I' * len(s)}\tNM:i:{len(mm)}")
        if not mine:
            out.append(f"{n}\t4\t*\t0\t0\t*\t*\t0\t0\t{s}\t{'I' * len(s)}\tXM:i:{1 if n in capped else 0}")
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")


def check_clusters(sample, tsv, repeats):
    """the conditions on the clusters, from the file the reference wrote and a brute-force look at the intervals"""
    kinds = {}
    by_chr = {}
    for chrom, start, end, name in repeats:
        by_chr.setdefault(chrom, []).append((start, end, name))
    for line in open(tsv).read().split("\n")[1:]:
        if not line:
            continue
        f = line.split("\t")
        orig, flag, name, chrom, strand, start, end, length = f[1], f[2], f[3], f[4], f[5], int(f[6]), int(f[7]), int(f[9])
        els = sorted(by_chr.get(chrom, []), key=lambda e: abs(e[0] - start))
        d = [abs(e[0] - start) for e in els[:3]]
        assert len(set(d)) == len(d), f"{f[0]}: equidistant repeat starts {d}"
        hit = [max(e[0], start) <= min(e[1], end) for e in els[:2]]
        if length > CLC:
            k = "long"
        elif orig.endswith("AAAAAA"):
            k = "polyA"
        elif orig.startswith("TTTTTT"):
            k = "polyT"
        elif chrom not in by_chr:
            k = "absent"
        elif len(els) == 1:
            k = "one_element"
        elif hit[0]:
            k = "nearest"
        elif hit[1]:
            k = "second_only"
        else:
            k = "kept"
        assert (flag == "1") == (k in ("absent", "kept") or (k == "one_element" and not hit[0])), (f[0], k, flag)
        if k == "nearest":
            assert name == els[0][2]
        if k == "second_only":
            assert name == els[1][2]
        kinds[k] = kinds.get(k, 0) + 1
        if strand == "-":
            kinds["minus"] = kinds.get("minus", 0) + 1
        if flag == "1" and k == "kept":
            kinds["kept_flag"] = kinds.get("kept_flag", 0) + 1
    for k in ("long", "polyA", "polyT", "nearest", "second_only", "one_element", "absent", "minus", "kept", "kept_flag"):
        assert kinds.get(k, 0) >= 2, (sample, k, kinds)
    return kinds


def main():
    rng = np.random.default_rng(21)
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    names, refs, seqs, counts, repeats, planted = make_frame(rng)
    with open(os.path.join(OUT, "repeats.txt"), "w") as fh:
        fh.write("".join(f"{c}\t{s}\t{e}\t{n}\n" for c, s, e, n in repeats))
    table = repeat_table(repeats)
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "human_genome")
        with open(base + ".fa", "w") as fh:
            fh.write("".join(f">{n}\n{r}\n" for n, r in zip(names, refs)))
        frame = pd.DataFrame({"Sequence": seqs, "annotFlag": 0, **{s: counts[:, k] for k, s in enumerate(SAMPLES)}}).set_index("Sequence")
        raw, filtered = {}, {}
        convert2Fasta(frame, "unmapped.log", MINL, MAXL, CUTOFF, tmp, "human", {}, SAMPLES, raw, filtered)
        ref_order = {n: k for k, n in enumerate(names)}
        for s in SAMPLES:
            fa = os.path.join(OUT, f"unmapped_mirna_{s}.fa")
            shutil.copy(os.path.join(tmp, f"unmapped_mirna_{s}.fa"), fa)
            r = subprocess.run([sys.executable, FAKE, base, fa, "-f", "-n", "0", "--best", "-a", "--threads", "1", "-m", str(MLOC), "-l",
                                str(SEEDLEN)], check=True, capture_output=True, text=True)
            sam = os.path.join(OUT, f"unmapped_mirna_{s}_vs_genome_sorted.sam")
            with open(sam, "w") as fh:
                fh.write("@HD\tVN:1.0\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{len(x)}\n" for n, x in zip(names, refs)))
                fh.write("".join(ln + "\n" for ln in default_lines_to_sam(r.stdout, ref_order)))
            clusters = os.path.join(OUT, f"{s}_clusters.tsv")
            cluster_basedon_location(sam, OLC, s, OUT, clusters)
            trimmed, cfa = os.path.join(OUT, f"{s}clusters_trimmed.tsv"), os.path.join(OUT, f"{s}_clusters_trimmed_orig.fa")
            n_kept = preTrimClusteredSeq(table, clusters, s, CLC, trimmed, cfa) - 1
            kinds = check_clusters(s, trimmed, repeats) if s == "S1" else {}
            q = _fasta_records(fa)
            q_names, q_seqs = [x.id for x in q], [x.seq for x in q]
            name_of = dict(zip(q_seqs, q_names))
            c = _fasta_records(cfa)
            c_names, c_lens = [x.id for x in c], [len(x.seq) for x in c]
            assert len(c_names) == n_kept
            index = os.path.join(tmp, f"{s}_representative_seq")
            shutil.copy(cfa, index + ".fa")
            # ---- run 1: -n 0 --best -a --norc -m 3 -l 25
            hits1 = fake_alignments(index, fa, ["-n", "0", "-m", str(MLOC), "-l", str(SEEDLEN)])
            capped = {n for n, h in hits1.items() if len(h) > MLOC}
            hits1 = {n: h for n, h in hits1.items() if n not in capped}
            tmp1 = os.path.join(OUT, f"{s}_tmp1.sam")
            write_cluster_sam(tmp1, q_names, q_seqs, hits1, c_names, c_lens, f"-f -n 0 --best -a --norc -m {MLOC} -l {SEEDLEN} -S", capped=capped)
            n_hits = [len(hits1.get(n, [])) for n in q_names]
            assert s != "S1" or sum(1 for k in n_hits if k == 1) >= 3 and sum(1 for k in n_hits if k >= 2) >= 3 and len(capped) >= 3
            assert s != "S1" or sum(1 for n, k in zip(q_names, n_hits) if k == 0 and n not in capped) >= 3
            imperfect = os.path.join(OUT, f"{s}_imperfectMath2Cluster.fa")
            split_fasta_from_sam(tmp1, fa, imperfect)
            qi = _fasta_records(imperfect)
            i_names, i_seqs = [x.id for x in qi], [x.seq for x in qi]
            assert capped <= set(i_names)
            # ---- run 2: -n 1 -l 15 -5 1 -3 3 --best --strata -a --norc
            every = fake_alignments(index, imperfect, ["-v", "2", "-5", "1", "-3", "3"])
            hits2, seen = {}, {}
            for n, hs in every.items():
                valid = [(h, sum(1 for k in h[3] if k < 15)) for h in hs]
                valid = [(h, sd) for h, sd in valid if sd <= 1 and len(h[3]) <= 2]
                if valid:
                    best = min(sd for _, sd in valid)
                    hits2[n] = [h for h, sd in valid if sd == best]
                    seen[n] = dict(best=best, kept=len(hits2[n]), dropped=len(valid) - len(hits2[n]),
                                   kept_mm=min(len(h[3]) for h in hits2[n]),
                                   dropped_mm=min([len(h[3]) for h, sd in valid if sd != best], default=None))
            tmp2 = os.path.join(OUT, f"{s}_tmp2.sam")
            write_cluster_sam(tmp2, i_names, i_seqs, hits2, c_names, c_lens, "-f -n 1 -l 15 -5 1 -3 3 --best --strata -a --norc -S", 1, 3)
            info = lambda kind: [seen.get(name_of[x]) for x in planted[kind] if x in name_of and name_of[x] in set(i_names)]
            ok = lambda kind, pred: s != "S1" or sum(1 for v in info(kind) if v is not None and pred(v)) >= 3
            assert ok("stratum0", lambda v: v["best"] == 0 and v["kept_mm"] == 0), info("stratum0")
            assert ok("stratum1", lambda v: v["best"] == 1 and v["dropped"] == 0), info("stratum1")
            assert ok("worse_dropped", lambda v: v["best"] == 0 and v["dropped"] >= 1), info("worse_dropped")
            assert ok("two_best", lambda v: v["kept"] >= 2), info("two_best")
            assert ok("total_in_worse_stratum", lambda v: v["best"] == 0 and v["kept_mm"] == 2 and v["dropped_mm"] == 1), \
                info("total_in_worse_stratum")
            assert sum(1 for v in info("unaligned") if v is None) >= 3
            lens2 = {len(x) - 4 for x, n in zip(i_seqs, i_names) if n in hits2}
            assert s != "S1" or (min(lens2) == 12 and max(lens2) == 21), lens2
            # ---- the text around it: the reference's functions
            combined, modified = os.path.join(OUT, f"{s}.sam"), os.path.join(OUT, f"{s}_modified.sam")
            combineSam(tmp1, tmp2, combined)
            decorateSam(combined, fa, modified, cfa)
            decorateSam(sam, fa, os.path.join(OUT, f"{s}_RepSeq_modified.sam"))
            sel, rev = os.path.join(OUT, f"{s}_selected.tsv"), os.path.join(OUT, f"{s}_selected_reverseKept.tsv")
            parse_refine_sam(modified, sel, rev)
            for src, dst in ((sel, f"{s}_modified_selected_sorted.tsv"), (rev, f"{s}_modified_selected_reverseKept_sorted.tsv")):
                with open(os.path.join(OUT, dst), "wb") as fh:
                    subprocess.run(["sort", "-k6,6", "-k1,1", src], check=True, stdout=fh, env=dict(os.environ, LC_ALL="C"))
                lines = open(os.path.join(OUT, dst)).read().split("\n")[:-1]
                keys = [(ln.split("\t")[5], ln.split("\t")[0]) for ln in lines]
                assert s != "S1" or any(a == b for a, b in zip(keys, keys[1:])), "no pair of lines that only the last-resort comparison orders"
            print(f"{s}: {filtered[s]} reads, {n_kept} clusters kept of {open(clusters).read().count(chr(10)) - 1} {kinds}; run 1: "
                  f"{sum(1 for k in n_hits if k)} aligned, {len(capped)} over -m; run 2: {len(i_names)} reads, {len(hits2)} aligned")
    with open(os.path.join(OUT, "derived.sha256"), "w") as fh:
        for s in SAMPLES:
            for f in HASHED + (HASHED_S2 if s != "S1" else ()):
                path = os.path.join(OUT, f.format(s=s))
                fh.write(f"{hashlib.sha256(open(path, 'rb').read()).hexdigest()}  {f.format(s=s)}\n")
                os.remove(path)


if __name__ == "__main__":
    main()

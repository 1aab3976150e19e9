#!/usr/bin/env python3
"""Generate tests/golden/sam_out/ -- the fixture of ``--sam-out`` -- with the REFERENCE's own code: ``bwtAlign`` with ``bam_out`` set
(mirge/libs/manifoldAlign.py:12-146; it keeps bowtie's lines in miRge3_<class>.sam) and then ``bow2bam`` (mirge/libs/bamFmt.py:
115-170) called class by class in the order of ``summarize`` (mirge/libs/summary.py:841-880), behind the header its ``sam_header``
writes for a library set it has no built-in header for.  ``createBAM`` is not run: there is no samtools, and the fixture is the
text it would be handed.  `bowtie` / `bowtie-inspect` are the stand-ins of tests/golden/fake_bowtie, ``Bio.Seq.Seq`` a stand-in whose
``complement`` swaps A/T and C/G and leaves everything else (N) as it is, which is what Biopython does with these letters.

Committed: the inputs (libs/, collapsed_input.csv) and the two files the reference wrote (S1.sam, S2.sam).  Runs only where the
reference is installed next to this repository; never from a test.

usage: python tests/golden/make_golden_sam_out.py
"""
import os
import shutil
import sys
import tempfile
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "stubs"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, ROOT)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

import Bio.Seq as _bioseq  # noqa: E402  (the stub)


class _Seq(str):
    def complement(self):
        return _Seq(self.translate(str.maketrans("ACGTacgt", "TGCAtgca")))


_bioseq.Seq = _Seq

import mirge3_amd  # noqa: E402,F401
from mirge3_amd.seqio import FlatSeqs, Library, index_basename, write_fasta  # noqa: E402

from mirge.libs.manifoldAlign import bwtAlign  # noqa: E402  (the reference)
from mirge.libs.bamFmt import bow2bam, sam_header  # noqa: E402  (the reference)

ORG, DB = "synthorg", "miRBase"  # an organism the reference has no built-in SAM header for
OUT = os.path.join(HERE, "sam_out")
PASS_COLS = ['exact miRNA', 'hairpin miRNA', 'mature tRNA', 'primary tRNA', 'snoRNA', 'rRNA', 'ncrna others', 'mRNA', 'isomiR miRNA',
             'spike-in']
COMP = str.maketrans("ACGT", "TGCA")


def rnd(rng, n):
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=n))


def sub(seq, pos, to=None):
    x = list(seq)
    x[pos] = to if to is not None else ("A" if x[pos] != "A" else "C")
    return "".join(x)


def make_libs(rng):
    mir = [rnd(rng, 22) for _ in range(6)]
    hp = [rnd(rng, 20) + m + rnd(rng, 38) for m in mir[:4]] + [rnd(rng, 90)]
    libs = {
        "mirna": Library([f"syn-miR-{i + 1}" for i in range(6)], FlatSeqs.from_list(mir),
                         [f"syn-miR-{i + 1} chr{1 + i % 2} segs:1-22 cds:{'-' if i == 2 else '+'}:{5000 + 100 * i}-{5021 + 100 * i}" for i in range(5)]
                         + ["syn-miR-6"]),                                            # the last miRNA carries no coordinates
        "hairpin": Library([f"syn-mir-{i + 1}" for i in range(5)], FlatSeqs.from_list(hp),
                           [f"syn-mir-{i + 1} chr{1 + i % 2} segs:1-{len(hp[i])} cds:{'-' if i == 1 else '+'}:{4980 + 100 * i}-{4979 + 100 * i + len(hp[i])}"
                            for i in range(5)]),
        "mature_trna": Library(["tRNA-A", "tRNA-B"], FlatSeqs.from_list([rnd(rng, 72), rnd(rng, 74)])),
        "pre_trna": Library(["pre-tRNA-A", "pre-tRNA-B"], FlatSeqs.from_list([rnd(rng, 90), rnd(rng, 95)])),
    }
    sno = [rnd(rng, 90) for _ in range(4)]
    libs["snorna"] = Library(["SNO1", "SNO2", "SNO3", "SNO4"], FlatSeqs.from_list(sno),
                             ["SNO1 chr3 segs:1-90 cds:+:20001-20090", "SNO2 chr4 segs:1-90 cds:-:30001-30090",
                              "SNO3", "SNO4 chrX segs:1-90"])                          # no coordinates / only part of them
    rr = [rnd(rng, 150) for _ in range(3)]
    libs["rrna"] = Library(["RR1", "RR2", "RR3"], FlatSeqs.from_list(rr),
                           ["RR1 chr5 segs:1-150 cds:+:700-849", "RR2 chrUn_PATCH segs:1-150 cds:+:900-1049",
                            "RR3 chr5 segs:1-150 cds:-:2000-2149"])
    nc = [rnd(rng, 120) for _ in range(3)]
    libs["ncrna_others"] = Library(["NC1", "NC2", "NC3"], FlatSeqs.from_list(nc),
                                   ["NC1 chr6 segs:1-120 cds:+:100-219", "NC2 chr6 segs:1-60,61-120 cds:-:5061-5120,4001-4060",
                                    "NC3 chr7 segs:1-120 cds:+:9000-9119"])
    mr = [rnd(rng, 300) for _ in range(4)]
    libs["mrna"] = Library(["ENST01.1", "ENST02.1", "ENST03.1", "ENST04.1"], FlatSeqs.from_list(mr),
                           ["ENST01.1 chr1 segs:1-100,101-300 cds:+:65565-65664,69037-69236",   # two segments
                            "ENST02.1 chr2 segs:1-100,121-300 cds:+:1000-1099,3000-3179",       # a gap in the segment list
                            "ENST03.1 chr2 segs:1-150,151-300 cds:-:8151-8300,7001-7150",       # minus strand, two segments
                            "ENST04.1 chr9 segs:1-300 cds:+:500-799"])
    return libs


def plan_reads(libs):
    """(read, count in S1, count in S2, tag) -- the tags name the cases the assertions below look for"""
    g = {k: v.seqs.to_list() for k, v in libs.items()}
    mir, hp, sno, rr, nc, mr = g["mirna"], g["hairpin"], g["snorna"], g["rrna"], g["ncrna_others"], g["mrna"]
    out = [
        (mir[0], 137, 1, "exact"),                                   # count >= 100 and count 1
        (mir[1], 10, 11, "exact10_11"),
        (mir[2], 3, 0, "exact_minus_one_sample"),                    # minus strand, present in S1 only
        (mir[5], 4, 4, "exact_no_coordinates"),
        ("A" + mir[3][:20] + "CC", 2, 12, "iso"),                    # pass 8: -5 1 -3 2
        ("C" + sub(mir[4][:20], 9) + "GT", 1, 0, "iso_mismatch"),
        (hp[0][3:31], 5, 2, "hairpin"),
        (hp[1][10:40], 0, 3, "hairpin_minus"),
        (sno[0][10:32], 1, 10, "sno"),
        (sub(sno[1][20:44], 15, "N"), 2, 1, "sno_minus_N"),          # minus-strand read with an N
        (sno[2][5:27], 6, 6, "sno_no_coordinates"),
        (sno[3][5:27], 2, 2, "sno_partial_header"),
        (sub(rr[0][5:30], 20), 11, 0, "rrna_one_mismatch"),
        (rr[1][40:62], 7, 7, "rrna_patch"),
        (rr[2][100:125], 1, 1, "rrna_minus"),
        (nc[0][30:52], 100, 9, "ncrna"),
        (nc[1][70:95], 1, 2, "ncrna_minus_second_segment"),
        (mr[0][150:172], 3, 1, "mrna_second_segment"),
        (mr[0][89:111], 2, 2, "mrna_past_segment_end"),              # POS 90 .. 111 runs past segment 1-100
        (mr[1][105:127], 1, 4, "mrna_outside_every_segment"),        # POS 106 lies in the gap 101-120
        (mr[2][160:185], 2, 0, "mrna_minus_second_segment"),
        (mr[3][0:30], 1, 1, "mrna_long"),
        (g["mature_trna"][0][5:27], 9, 9, "trna"),                   # annotated, writes nothing
        ("ACGTTGCAACGTTGCAAC", 5, 5, "unmapped"),
    ]
    return out


def build_frame(sample_dicts, base_names):
    """the frame ``baking`` hands to ``bwtAlign`` (schema of digest.py:237-261), as make_golden.py builds it"""
    complete_set = pd.DataFrame()
    for name, d in zip(base_names, sample_dicts):
        collapsed_df = pd.DataFrame(list(d.items()), columns=['Sequence', name])
        collapsed_df.set_index('Sequence', inplace=True)
        complete_set = collapsed_df if len(base_names) == 1 else complete_set.join(collapsed_df, how='outer')
        complete_set = complete_set.fillna(0).astype(int)
    complete_set = complete_set.assign(**dict.fromkeys(PASS_COLS, ''))
    complete_set = complete_set.assign(**dict.fromkeys(['annotFlag'], '0'))
    complete_set = complete_set.reindex(columns=['annotFlag'] + PASS_COLS + base_names)
    return complete_set.astype({"annotFlag": int})


def main():
    rng = np.random.Generator(np.random.PCG64(20240917))
    libs = make_libs(rng)
    plan = plan_reads(libs)
    shutil.rmtree(OUT, ignore_errors=True)
    tmp = tempfile.mkdtemp(prefix="mirge_golden_sam_")
    libdir = os.path.join(tmp, "Libs")
    idx = os.path.join(libdir, ORG, "index.Libs")
    os.makedirs(idx)
    os.makedirs(os.path.join(libdir, ORG, "annotation.Libs"))
    for key, lib in libs.items():
        write_fasta(os.path.join(idx, index_basename(ORG, key, DB) + ".fa"), lib)
    open(os.path.join(libdir, ORG, "annotation.Libs", f"{ORG}_merges_{DB}.csv"), "w").close()
    base_names = ["S1", "S2"]
    dicts = [{q: c[s] for q, *c, _ in plan if c[s] > 0} for s in range(2)]
    df = build_frame(dicts, base_names)
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    args = SimpleNamespace(threads=2, bowtie_path=os.path.join(HERE, "fake_bowtie"), bowtieVersion="True", quiet=True, bam_out=True,
                           tRNA_frag=False, spikeIn=False, organism_name=ORG, libraries_path=libdir, samtools_path=None)
    collapsed = df[base_names].copy()
    df = bwtAlign(args, df, work, DB)
    pdMapped = df[df.annotFlag.eq(1)].reset_index(level=['Sequence'])
    # ---- summary.py:841-880, without createBAM
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):  # (sam_header prints its note)
        header = sam_header(args)
    for nm in base_names:
        with open(os.path.join(work, nm + ".sam"), "w+") as fh:
            fh.write(header)
    for col, pref in (('snoRNA', 'snorna'), ('rRNA', 'rrna'), ('ncrna others', 'ncrna_others'), ('mRNA', 'mrna')):
        rows = pd.DataFrame(pdMapped[pdMapped[col].astype(bool)], columns=["Sequence", col] + base_names).values.tolist()
        rna_type = ORG + "_" + pref
        bow2bam(args, work, DB, rows, base_names, os.path.join(idx, rna_type), rna_type, pref)
    rows = pd.DataFrame(pdMapped[pdMapped['exact miRNA'].astype(bool)], columns=["Sequence", "exact miRNA"] + base_names).values.tolist()
    rows.extend(pd.DataFrame(pdMapped[pdMapped['isomiR miRNA'].astype(bool)], columns=["Sequence", "isomiR miRNA"] + base_names).values.tolist())
    rna_type = ORG + "_mirna_" + DB
    bow2bam(args, work, DB, rows, base_names, os.path.join(idx, rna_type), rna_type, "miRNA")
    rows = pd.DataFrame(pdMapped[pdMapped['hairpin miRNA'].astype(bool)], columns=["Sequence", "hairpin miRNA"] + base_names).values.tolist()
    rna_type = ORG + "_hairpin_" + DB
    bow2bam(args, work, DB, rows, base_names, os.path.join(idx, rna_type), rna_type, "hairpin_miRNA")

    # ---- the cases the fixture must hold
    sam = {}
    for nm in base_names:
        with open(os.path.join(work, nm + ".sam")) as fh:
            text = fh.read()
        assert text.startswith(header) and header == "@HD\tVN:1.0\tSO:unsorted\n"
        sam[nm] = [ln.split("\t") for ln in text[len(header):].split("\n") if ln]
    tag = {t: q for q, _, _, t in plan}
    cnt = {t: (a, b) for _, a, b, t in plan}
    col_of = {q: next((c for c in PASS_COLS if c in df.columns and df.at[q, c] != ''), None) for q in df.index}

    def lines(t, nm):
        return [f for f in sam[nm] if f[0].rsplit("_", 1)[0] == tag[t]]

    for t, col in (("exact", "exact miRNA"), ("iso", "isomiR miRNA"), ("hairpin", "hairpin miRNA"), ("sno", "snoRNA"),
                   ("rrna_one_mismatch", "rRNA"), ("ncrna", "ncrna others"), ("mrna_second_segment", "mRNA"), ("trna", "mature tRNA")):
        assert col_of[tag[t]] == col, (t, col_of[tag[t]])
    for t in tag:  # every row: as many lines as copies, numbered 0 .. c-1, or none at all
        absent = t in ("trna", "unmapped", "exact_no_coordinates", "sno_no_coordinates", "sno_partial_header", "rrna_patch")
        for s, nm in enumerate(base_names):
            got = lines(t, nm)
            assert len(got) == (0 if absent else cnt[t][s]), (t, nm, len(got))
            assert [f[0] for f in got] == [f"{tag[t]}_{k}" for k in range(len(got))]
    for t in ("exact_no_coordinates", "sno_no_coordinates", "sno_partial_header", "rrna_patch"):
        assert col_of[tag[t]] is not None  # annotated, yet without a line
    assert sorted({c for t in tag for c in cnt[t]} & {1, 10, 11}) == [1, 10, 11] and max(max(c) for c in cnt.values()) >= 100
    assert lines("exact_minus_one_sample", "S1") and not lines("exact_minus_one_sample", "S2")
    f = lines("sno_minus_N", "S1")[0]
    assert f[1] == "16" and "N" in f[9] and f[9] == tag["sno_minus_N"][::-1].translate(COMP) and f[2] == "chr4"
    assert f[3] == str(30090 - 20 - 24 + 1)
    f = lines("mrna_second_segment", "S1")[0]
    assert f[1] == "0" and f[2] == "chr1" and f[3] == str(69037 + (151 - 101)) and f[5] == "22M"
    f = lines("mrna_past_segment_end", "S1")[0]
    assert f[3] == str(65565 + 89) and f[5] == "22M"  # POS 90 + 22 - 1 = 111 > 100: still the plain CIGAR
    f = lines("mrna_outside_every_segment", "S1")[0]
    assert f[3] == "106" and f[2] == "chr2"
    f = lines("mrna_minus_second_segment", "S1")[0]
    assert f[1] == "16" and f[3] == str(7150 - (161 - 151) - 25 + 1)
    f = lines("ncrna_minus_second_segment", "S2")[0]
    assert f[1] == "16" and f[3] == str(4060 - (71 - 61) - 25 + 1)
    f = lines("iso", "S2")[0]
    assert len(f[9]) == len(tag["iso"]) - 3 and f[9] == tag["iso"][1:-2] and f[0].startswith(tag["iso"] + "_") and f[5] == "20M"
    f = lines("iso_mismatch", "S1")[0]
    assert f[-1] == "NM:i:1" and f[-2] != "MD:Z:20"
    # the order of the classes in a file
    order = [col_of[f[0].rsplit("_", 1)[0]] for f in sam["S1"]]
    seen = [c for k, c in enumerate(order) if k == 0 or order[k - 1] != c]
    assert seen == ['snoRNA', 'rRNA', 'ncrna others', 'mRNA', 'exact miRNA', 'isomiR miRNA', 'hairpin miRNA'], seen

    os.makedirs(OUT)
    shutil.copytree(os.path.join(libdir, ORG), os.path.join(OUT, "libs", ORG))
    collapsed.to_csv(os.path.join(OUT, "collapsed_input.csv"))
    for nm in base_names:
        shutil.copy(os.path.join(work, nm + ".sam"), os.path.join(OUT, nm + ".sam"))
    shutil.rmtree(tmp)
    print("sam_out:", {nm: len(v) for nm, v in sam.items()}, "lines ->", OUT)


if __name__ == "__main__":
    main()

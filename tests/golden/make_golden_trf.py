#!/usr/bin/env python3
"""Generate tests/golden/case8_trf/ by running the REFERENCE's own ``trfTypes`` (/root/reference/mirge/libs/summary.py:649) and
``trna_deliverables`` (mirge2_tRF_a2i.py:522) on a small tRNA library, its five annotation files and three samples made here.

Runs only where /root/reference exists (never on the GPU box, never from a test); what is committed is data: the library set, the
annotation files, the samples' FASTQ and the six files the reference wrote up to mirge2_tRF_a2i.py:744.  The reference goes on to
its clustering files (<sample>.aligned_tRFs.clusters.detail, <sample>.tRFs.report.tsv): it writes them into a temporary directory
and they are not committed (mirge3_amd/trf.py says why they are out of scope).  No reference source is copied.

Recipe, as in make_golden.py (stand-ins of tests/golden/stubs for Bio / cutadapt at import time), plus:
  * ``trfContentDic`` -- what summary.py:1182-1216 collects from bowtie's ``-a --best --strata`` SAM files -- is built HERE by a
    brute-force enumeration of every window, under the project's rules 1 and 2 (mirge3_amd/trf.py: lowest offset of a reference,
    references in library order), with the reference's own ``trfTypes`` and ``UID``;
  * ``random.choice`` and the ``set`` whose order the reference leaves to the hash seed (mirge2_tRF_a2i.py:563-567) are replaced in
    the imported module by rule 3: the candidates in library order, the first one chosen;
  * the dictionaries handed to ``trna_deliverables`` are built from the same structures the annotation files are written from, not
    by the project's parser, so that the golden files check that parser too.
The script asserts that the case holds everything it was made for before it writes.

usage: python tests/golden/make_golden_trf.py
"""
import os
import re
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

import mirge3_amd  # noqa: E402,F401
from mirge3_amd.seqio import FlatSeqs, Library, index_basename, write_fasta  # noqa: E402

import mirge.libs.mirge2_tRF_a2i as ref_trf  # noqa: E402  (the reference)
from mirge.libs.miRgeEssential import UID  # noqa: E402  (the reference)
from mirge.libs.summary import addDashNew, trfTypes  # noqa: E402  (the reference)

OUT = os.path.join(HERE, "case8_trf")
ORG, DB = "synthorg", "miRBase"
SAMPLES = ["S1", "S2", "S3"]  # S3 holds no tRNA read: the ZeroDivisionError branches
FILES = ("tRFs.aligned.report.tsv", "tRF.Counts.csv", "tRF.RP100K.csv", "discarded.reads.summary.assigningtRFs.csv")
AC = 33  # 0-based anticodon start of every synthetic tRNA


def rnd(rng, n):
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=n))


def sub(seq, pos):
    return seq[:pos] + "ACGT"[("ACGT".index(seq[pos]) + 1) % 4] + seq[pos + 1:]


def make_libraries(rng):
    aa = ["Ala-AGC", "Ala-AGC", "Gly-GCC", "Gly-GCC", "Leu-CAA", "Und-NNN", "Val-TAC", "Ser-GCT", "Lys-CTT", "Glu-CTC"]
    seqs = [rnd(rng, int(n)) for n in (72, 72, 76, 76, 88, 73, 74, 82, 75, 71)]
    seqs = [s[:-1] + "G" if s.endswith("TTT") or s[-1] == "T" else s for s in seqs]  # (a mature read must not end in a T run)
    seqs[1] = seqs[0]                          # identical sequence, another name
    seqs[3] = sub(seqs[2], 20)                 # one base apart
    rep = seqs[4][5:25]
    seqs[4] = seqs[4][:45] + rep + seqs[4][65:]  # a 20-mer twice
    names, k = [], {}
    for a in aa:
        k[a] = k.get(a, 0) + 1
        names.append(f"tRNA-{a}-{k[a]}-1")
    trailers = ["GCATCGATTTT", "CAGTCTTTTTT", "GGACTATTTT", "ACCGATTTT", "GTCAGCATTTTT", "CGTATTTT", "TGACGATTTT", "AGCCATTTT"]
    pre = [rnd(rng, 5 + i % 4) + seqs[i] + trailers[i] for i in range(8)]
    pre_names = ["pre_" + names[i] for i in range(8)]
    other = {
        "mirna": Library([f"syn-miR-{i + 1}" for i in range(4)], FlatSeqs.from_list([rnd(rng, 22) for _ in range(4)])),
        "hairpin": Library([f"syn-mir-{i + 1}" for i in range(3)], FlatSeqs.from_list([rnd(rng, 80) for _ in range(3)])),
        "snorna": Library(["SNO1", "SNO2"], FlatSeqs.from_list([rnd(rng, 120), rnd(rng, 90)])),
        "rrna": Library(["RR1"], FlatSeqs.from_list([rnd(rng, 200)])),
        "ncrna_others": Library(["NC1"], FlatSeqs.from_list([rnd(rng, 150)])),
        "mrna": Library(["ENST01.1"], FlatSeqs.from_list([rnd(rng, 300)])),
    }
    return names, seqs, pre_names, pre, aa, other


def make_infor(rng, names, seqs):
    """rows of _tRF_infor.csv: (cluster name, 'start-end', sequence, the column whose length is taken for the tRNA's)"""
    rows = []

    def put(r, s0, e0, tag, seq=None, total=None):  # 0-based inclusive bounds
        rows.append((f"{names[r]}_Cluster{tag}", f"{s0 + 1}-{e0 + 1}", seq if seq is not None else seqs[r][s0:e0 + 1],
                     (seqs[r] if total is None else seqs[r][:total])))

    put(6, 14, 35, 1)                 # read seqs[6][10:40]: |11 - 15| + |40 - 36| = 8 -> assigned
    put(6, 50, 70, 2)
    put(7, 14, 34, 1)                 # read seqs[7][10:40]: 4 + 5 = 9 -> Undef
    put(8, 8, 29, 9)                  # read seqs[8][10:30]: 2 and 2: 'Cluster10' sorts before 'Cluster9'
    put(8, 10, 31, 10)
    put(9, 0, 30, 1, total=50)        # a sequence column shorter than the tRNA
    put(9, 0, 30, 2, total=50)        # ... the same dashed string again: the later line's name stays
    put(9, 40, 70, 3, seq=sub(seqs[9][40:71], 7))
    for r in (0, 1, 2, 3, 4):         # (reference 5 has no row: 'Dele')
        for tag, (s0, e0) in enumerate(((0, AC - 1), (AC + 2, len(seqs[r]) - 1), (12, 40), (0, 18))):
            put(r, s0, e0, tag + 1)
    for i in range(3):
        put(i, 1 + i, 22 + i, 7, seq=None)
    rows.append((f"pre_{names[0]}_Cluster1", "70-85", "A" * 16, "A" * 88))
    return rows


def make_reads(rng, names, seqs, pre):
    """{read: (count in S1, count in S2)}"""
    reads = {}

    def put(s, c1=None, c2=None):
        if s not in reads:
            reads[s] = (int(rng.integers(1, 5)) if c1 is None else c1, int(rng.integers(0, 4)) if c2 is None else c2)

    for r in (0, 2, 4, 6):  # every trfTypes branch with the boundary values of each half test
        m, tl = seqs[r], len(seqs[r])
        put(m)                                                     # tRF-whole (more than 64 nt)
        for e in (AC - 3, AC - 2, AC + 1, AC + 2):
            put(m[:e + 1])                                         # 5'-tRF | 5'-half | 5'-half | 5'-tRF
        for s in (AC - 2, AC - 1, AC + 2, AC + 3):
            put(m[s:])                                             # 3'-tRF | 3'-half | 3'-half | 3'-tRF
        for e in (tl - 4, tl - 3, tl - 1):
            put(m[AC:e + 1]); put(m[5:e + 1])                      # i-tRF beyond the edge, 3' inside it
    put(seqs[2][10:36])                                            # exact in reference 2, one mismatch in reference 3
    put(sub(seqs[2][12:40], 20))                                   # one mismatch in 2 (at 32), two in 3: stratum 1
    put(sub(seqs[2][30:60], 4))                                    # one mismatch in both
    put(seqs[4][5:25]); put(seqs[4][3:25])                         # the 20-mer that is there twice
    put(seqs[5][8:30]); put(seqs[5][40:])                          # the reference without predefined tRFs
    put(seqs[6][10:40]); put(seqs[7][10:40]); put(seqs[8][10:30])  # distance 8, 9, and the tie
    put(seqs[9][:31]); put(seqs[9][40:71]); put(seqs[9][35:60])
    put(seqs[6][:12] + "N" + seqs[6][13:30]); put(seqs[8][40:50] + "N" + seqs[8][51:70], 3, 0)
    put(seqs[0][20:45], 5, 0); put(seqs[3][30:55], 0, 7)           # in one sample only
    for i in range(8):
        body = pre[i][:len(pre[i]) - len(re.search("T+$", pre[i]).group(0))]
        put(body[-18:] + "TTT")                                    # a T run of 3
        put(body[-24:] + "TTTT")
    put(pre[1][:-6][-20:] + "TTTTT", 4, 2)                         # a T run of 5 inside the trailer's six
    put(pre[3][:-4][-22:] + "TTTTTTT", 2, 1)                       # the run overhangs the trailer
    put(pre[4][:-5][10:40] + "TTT", 1, 1)                          # 'TTT' behind a window far from the trailer: overhang too
    for _ in range(30):
        r = int(rng.integers(0, len(seqs)))
        L = int(rng.integers(16, 50))
        o = int(rng.integers(0, len(seqs[r]) - L + 1))
        s = seqs[r][o:o + L]
        put(s if rng.integers(0, 3) else sub(s, int(rng.integers(0, L))))
    return reads


def windows(read, refs, max_mm):
    """[(ref, off, mismatches)] of every window of ACGT with at most max_mm mismatches; N in the read is a mismatch"""
    out = []
    for r, ref in enumerate(refs):
        for o in range(len(ref) - len(read) + 1):
            w = ref[o:o + len(read)]
            if set(w) - set("ACGT"):
                continue
            mm = sum(a != b for a, b in zip(read, w))
            if mm <= max_mm:
                out.append((r, o, mm))
    return out


def classify(read, seqs, pre):
    """-> ('mature' | 'primary' | None, [(ref, lowest offset)] in library order): rules 1 and 2"""
    w = windows(read, seqs, 1)
    if w:
        best = min(m for _, _, m in w)
        first = {}
        for r, o, m in w:
            if m == best:
                first.setdefault(r, o)
        return "mature", sorted(first.items()), len([1 for _, _, m in w if m == best]), best, len(w)
    t = re.search("T{3,}$", read)
    if t and t.start() > 0:
        w = windows(read[:t.start()], pre, 0)
        if w:
            first = {}
            for r, o, _ in w:
                first.setdefault(r, o)
            return "primary", sorted(first.items()), len(w), 0, len(w)
    return None, [], 0, 0, 0


def main():
    rng = np.random.default_rng(88)
    names, seqs, pre_names, pre, aa, other = make_libraries(rng)
    infor_rows = make_infor(rng, names, seqs)
    reads = make_reads(rng, names, seqs, pre)
    for lib in other.values():  # the tRNA reads belong to no class in front of theirs
        for s in lib.seqs.to_list():
            assert not any(rd in s for rd in reads)

    # ---- the dictionaries of summary.py:1067-1159, from the structures the files are written from
    stru = {nm: dict(seq=s, stru="." * AC + "XXX" + "." * (len(s) - AC - 3), anticodonStart=AC + 1, anticodonEnd=AC + 3) for nm, s in zip(names, seqs)}
    aa_dic = {}
    for nm, a in zip(names, aa):
        aa_dic[nm] = dict(aaType=a.split("-")[0], anticodon=a.split("-")[1])
        aa_dic["pre_" + nm] = dict(aaType=a.split("-")[0], anticodon=a.split("-")[1])
    # (a name whose stand-in is no hit of the read makes the reference raise KeyError, mirge2_tRF_a2i.py:583: not a golden case)
    dedup_lines = [(names[0], [names[0], names[1]]), (names[7], [names[7]])]
    dup = {item: uniq for uniq, items in dedup_lines for item in items}
    trf_dic = {}
    for cluster, span, seq, col in infor_rows:
        s, e = (int(x) for x in span.split("-"))
        trf_dic.setdefault(cluster.split("_Cluster")[0], {})[addDashNew(seq, len(col), s, e)] = cluster
    clusters = sorted({r[0] for r in infor_rows})
    merge_lines = [("m-" + c, [c]) for c in clusters[3:]] + [("m-joined", clusters[:3])]
    merged_list = [m for m, _ in merge_lines]
    merged_of = {c: m for m, cs in merge_lines for c in cs}
    pre_dic = dict(zip(pre_names, pre))
    lib_order = {nm: (0, i) for i, nm in enumerate(names)}
    lib_order.update({nm: (1, i) for i, nm in enumerate(pre_names)})

    # ---- trfContentDic (summary.py:1182-1216) by brute force, rows in mapped.csv's order: the sorted union of the samples' reads
    rows = {"mature": [], "primary": []}
    facts = dict(types=set(), multi_window=0, both_strata=0, n_read=0, whole64=0, truns=set(), overhang=0, one_sample=0, dedup_pair=0)
    for rd in sorted(reads):
        cls, hits, n_best, best, n_all = classify(rd, seqs, pre)
        assert cls is not None, rd
        rows[cls].append((rd, hits))
        facts["multi_window"] += n_best > len(hits)
        facts["both_strata"] += cls == "mature" and best == 0 and n_all > n_best
        facts["n_read"] += "N" in rd
        facts["one_sample"] += 0 in reads[rd]
        facts["dedup_pair"] += cls == "mature" and {0, 1} <= {r for r, _ in hits}
    content = {}
    sums = {"mature": [0, 0, 0], "primary": [0, 0, 0]}
    for cls in ("mature", "primary"):
        for rd, hits in rows[cls]:
            cnt = [reads[rd][0], reads[rd][1], 0]
            for i in range(3):
                sums[cls][i] += cnt[i]
            content[rd] = {"count": cnt, "uid": UID(rd, "tRF") if "N" not in rd else "."}
            for r, o in hits:
                nm = names[r] if cls == "mature" else pre_names[r]
                d = dict(start=o, cigar="undifined", tRFType=trfTypes(rd, nm, o, stru))
                d["end"] = o + len(rd) - 1
                if cls == "primary":
                    run = len(rd) - re.search("T{3,}$", rd).span(0)[0]
                    d["end"] -= run
                    facts["truns"].add(run)
                    facts["overhang"] += o + len(rd) > len(pre[r])
                else:
                    facts["whole64"] += d["tRFType"] == "tRF-whole" and len(rd) > 64
                content[rd][nm] = d
                facts["types"].add(d["tRFType"])

    # ---- the case holds what it is for
    assert facts["types"] == {"tRF-whole", "5'-half", "5'-tRF", "3'-half", "3'-tRF", "i-tRF", "tRF-1"}, facts["types"]
    for r in (0, 2, 4, 6):  # the boundary values, as the reference types them
        m, tl = seqs[r], len(seqs[r])
        assert [trfTypes(m[:e + 1], names[r], 0, stru) for e in (AC - 3, AC - 2, AC + 1, AC + 2)] == ["5'-tRF", "5'-half", "5'-half", "5'-tRF"]
        assert [trfTypes(m[s:], names[r], s, stru) for s in (AC - 2, AC - 1, AC + 2, AC + 3)] == ["3'-tRF", "3'-half", "3'-half", "3'-tRF"]
        assert [trfTypes(m[5:e + 1], names[r], 5, stru) for e in (tl - 4, tl - 3, tl - 1)] == ["i-tRF", "3'-tRF", "3'-tRF"]
    assert facts["multi_window"] and facts["both_strata"] and facts["n_read"] and facts["whole64"] and facts["one_sample"] and facts["dedup_pair"]
    assert {3, 5} <= facts["truns"] and facts["overhang"], facts
    assert seqs[0] == seqs[1] and sum(a != b for a, b in zip(seqs[2], seqs[3])) == 1 and seqs[4].count(seqs[4][5:25]) == 2
    assert all(p.endswith("TTTT") for p in pre) and names[5] not in trf_dic and sums["mature"][2] == 0 and sums["primary"][2] == 0
    dashed = lambda r, s0, L: addDashNew(seqs[r][s0:s0 + L], len(seqs[r]), s0 + 1, s0 + L)
    assert ref_trf.assign_cluster(dashed(6, 10, 30), names[6], trf_dic)[:2] == (names[6] + "_Cluster1", 8)
    assert ref_trf.assign_cluster(dashed(7, 10, 30), names[7], trf_dic)[:2] == ("Undef", 9)
    tie = sorted((ref_trf.getDistance2(dashed(8, 10, 20), s), c) for s, c in trf_dic[names[8]].items())
    assert tie[0][0] == tie[1][0] == 2 and tie[0][1].endswith("Cluster10")
    assert any(len(s) < len(seqs[9]) for s in trf_dic[names[9]])

    # ---- write the inputs
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    idx = os.path.join(OUT, "libs", ORG, "index.Libs")
    annd = os.path.join(OUT, "libs", ORG, "annotation.Libs")
    os.makedirs(idx)
    os.makedirs(annd)
    libs = dict(other, mature_trna=Library(names, FlatSeqs.from_list(seqs)), pre_trna=Library(pre_names, FlatSeqs.from_list(pre)))
    for key, lib in libs.items():
        write_fasta(os.path.join(idx, index_basename(ORG, key, DB) + ".fa"), lib)
    open(os.path.join(annd, f"{ORG}_merges_{DB}.csv"), "w").close()
    with open(os.path.join(annd, f"{ORG}_trna.str"), "w") as fh:
        fh.write("".join(f">{nm}\n{stru[nm]['seq']}\n{stru[nm]['stru']}\n" for nm in names))
    with open(os.path.join(annd, f"{ORG}_trna_aminoacid_anticodon.csv"), "w") as fh:
        fh.write("".join(f"{nm},{d['aaType']},{d['anticodon']}\n" for nm, d in aa_dic.items()))
    with open(os.path.join(annd, f"{ORG}_trna_deduplicated_list.csv"), "w") as fh:
        fh.write("unique tRNA,duplicated tRNAs\n" + "".join(f"{u},{'/'.join(items)}\n" for u, items in dedup_lines))
    with open(os.path.join(annd, f"{ORG}_tRF_infor.csv"), "w") as fh:
        fh.write("tRF cluster,type,anticodon,position,sequence,tRNA sequence\n")
        fh.write("".join(f"{c},tRF,NNN,{span},{seq},{col}\n" for c, span, seq, col in infor_rows))
    with open(os.path.join(annd, f"{ORG}_tRF_merges.csv"), "w") as fh:
        fh.write("".join(f"{m},{'/'.join(cs)}\n" for m, cs in merge_lines))
    mir = other["mirna"].seqs.to_list()
    per_sample = {s: [] for s in SAMPLES}
    for rd, (c1, c2) in reads.items():
        per_sample["S1"] += [rd] * c1
        per_sample["S2"] += [rd] * c2
    for i, s in enumerate(SAMPLES):
        per_sample[s] += [mir[i % len(mir)]] * (3 + i) + [rnd(rng, 30) for _ in range(4)]
        order = rng.permutation(len(per_sample[s]))
        with open(os.path.join(OUT, f"{s}.fastq"), "w") as fh:
            fh.write("".join(f"@{k}\n{per_sample[s][j]}\n+\n{'I' * len(per_sample[s][j])}\n" for k, j in enumerate(order)))

    # ---- the reference, with rule 3 in place of its random.choice and of its set's order
    in_lib_order = lambda xs: sorted(dict.fromkeys(xs), key=lambda nm: lib_order.get(nm, (2, nm)))
    ref_trf.random = SimpleNamespace(choice=lambda xs: in_lib_order(xs)[0])
    ref_trf.set = in_lib_order
    tmp = tempfile.mkdtemp(prefix="golden_trf_")
    try:
        ref_trf.trna_deliverables(SimpleNamespace(), tmp, pre_dic, content, sums["mature"], sums["primary"], aa_dic, SAMPLES, stru, dup,
                                  merged_list, trf_dic, merged_of)
    except Exception as e:  # the clustering behind line 744 is not this case's business
        print("the reference stopped behind its per-sample reports:", repr(e))
    for f in FILES:
        shutil.copy(os.path.join(tmp, f), os.path.join(OUT, f))
    os.makedirs(os.path.join(OUT, "tRFs.samples.tmp"))
    for s in SAMPLES:
        for suffix in (".aligned_tRFs.report", ".aligned_tRFs.summary.report"):
            shutil.copy(os.path.join(tmp, "tRFs.samples.tmp", s + suffix), os.path.join(OUT, "tRFs.samples.tmp", s + suffix))
    shutil.rmtree(tmp)
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(OUT) for f in fs)
    print(f"{len(reads)} reads ({len(rows['mature'])} mature, {len(rows['primary'])} primary), {size} bytes in {OUT}")
    assert size < 200 * 1024


if __name__ == "__main__":
    main()

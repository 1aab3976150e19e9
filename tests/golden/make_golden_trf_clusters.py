#!/usr/bin/env python3
"""Generate tests/golden/case9_trf_clusters/ by letting the REFERENCE's ``trna_deliverables`` (mirge2_tRF_a2i.py:522-947) run to its end:
the files of tests/golden/case8_trf's kind plus, per sample, ``<sample>.aligned_tRFs.clusters.detail`` and ``<sample>.tRFs.report.tsv``.

Runs only where /root/reference exists (never on the GPU box, never from a test); what is committed is data.  The library, annotation
and read builders are those of make_golden_trf.py, imported unchanged, and the same rule-3 patches are applied to the imported
reference module.  On top of them:
  * the primary tRNAs are named ``pre_<tRNA>_trailer``, the form the reference's name folding expects (mirge2_tRF_a2i.py:761-762, 941);
  * two more samples: S4 holds designed groups only (two clusters with a border and a far point, a one-cluster fallback, a centre with a
    mismatch, a tRNA selected as mature and as trailer), S5 one read 60 000 times (gzip keeps it small) so that a count of 1 is 1.7 RP100K;
  * counts are nudged until no group holds two equal float32 densities: the reference leaves their order to NumPy's sort.
Before it writes, the script asserts with the reference's own ``getDistance`` / ``local_density`` / ``min_distance`` on
``load_data_new``'s output that the case stays inside what the reference defines and holds what it is made for.

usage: python tests/golden/make_golden_trf_clusters.py
"""
import gzip
import os
import re
import shutil
import sys
import tempfile
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_trf as g8  # noqa: E402  (its imports put the stubs, the reference and the package on the path)

import numpy as np  # noqa: E402
from mirge3_amd.seqio import FlatSeqs, Library, index_basename, write_fasta  # noqa: E402

ref_trf = g8.ref_trf
OUT = os.path.join(HERE, "case9_trf_clusters")
ORG, DB, AC = g8.ORG, g8.DB, g8.AC
SAMPLES = ["S1", "S2", "S3", "S4", "S5"]
GZ = {"S1", "S2", "S4", "S5"}   # written as .fastq.gz
RUN = {"S5"}                     # one read over and over: written in order under one header, which is what gzip shrinks
FILES = g8.FILES
DEEP = 60000


def designed(seqs, pre):
    """{read: count} of S4 and of S5"""
    m6, m7, m2 = seqs[6], seqs[7], seqs[2]
    s4 = {m6[:31]: 100, m6[:39]: 60, m6[:26]: 50, m6[:21]: 45, m6[:34]: 2, m6[:37]: 1,   # centre P, centre Q, A, A2 (far), P1 | Q1 (border)
          m7[:30]: 9, m7[:33]: 5,                                                       # no point with delta >= 8: the fallback
          g8.sub(m2[12:40], 20): 20}                                                    # a centre with a mismatch
    body = pre[6][:len(pre[6]) - len(re.search("T+$", pre[6]).group(0))]
    s4[body[-18:] + "TTT"] = 12
    s4[body[-24:] + "TTTT"] = 7
    s5 = {seqs[8][10:30]: DEEP, seqs[9][:31]: 1, seqs[9][:33]: 1, seqs[9][:36]: 1, seqs[0][20:45]: 2}  # (distances 2, 3, 5: no two densities equal)
    return s4, s5


def clustering_facts(report_path):
    """what the reference's own functions say about every group of a sample's report"""
    out = []
    for info in ref_trf.load_data_new(report_path):
        dist, max_dis, _, max_id = ref_trf.getDistance(info)
        rho = ref_trf.local_density(dist, info, max_id, dc=3.0)
        out.append(dict(n=max_id, rho=rho[1:], tie=len(set(rho[1:].tolist())) < max_id, info=info, dist=dist, max_dis=max_dis))
    return out


def main():
    rng = np.random.default_rng(88)
    names, seqs, pre_names, pre, aa, other = g8.make_libraries(rng)
    infor_rows = g8.make_infor(rng, names, seqs)
    base = g8.make_reads(rng, names, seqs, pre)
    pre_names = [nm + "_trailer" for nm in pre_names]
    s4, s5 = designed(seqs, pre)
    reads = {rd: [c1, c2, 0, 0, 0] for rd, (c1, c2) in base.items()}
    for col, extra in ((3, s4), (4, s5)):
        for rd, c in extra.items():
            reads.setdefault(rd, [0, 0, 0, 0, 0])[col] = c
    for lib in other.values():
        for s in lib.seqs.to_list():
            assert not any(rd in s for rd in reads)

    stru = {nm: dict(seq=s, stru="." * AC + "XXX" + "." * (len(s) - AC - 3), anticodonStart=AC + 1, anticodonEnd=AC + 3) for nm, s in zip(names, seqs)}
    aa_dic = {}
    for i, (nm, a) in enumerate(zip(names, aa)):
        aa_dic[nm] = dict(aaType=a.split("-")[0], anticodon=a.split("-")[1])
        aa_dic["pre_" + nm + "_trailer"] = dict(aaType=a.split("-")[0], anticodon=a.split("-")[1])
    dedup_lines = [(names[0], [names[0], names[1]]), (names[7], [names[7]])]
    dup = {item: uniq for uniq, items in dedup_lines for item in items}
    trf_dic = {}
    for cluster, span, seq, col in infor_rows:
        s, e = (int(x) for x in span.split("-"))
        trf_dic.setdefault(cluster.split("_Cluster")[0], {})[g8.addDashNew(seq, len(col), s, e)] = cluster
    clusters = sorted({r[0] for r in infor_rows})
    merge_lines = [("m-" + c, [c]) for c in clusters[3:]] + [("m-joined", clusters[:3])]
    merged_list = [m for m, _ in merge_lines]
    merged_of = {c: m for m, cs in merge_lines for c in cs}
    pre_dic = dict(zip(pre_names, pre))
    lib_order = {nm: (0, i) for i, nm in enumerate(names)}
    lib_order.update({nm: (1, i) for i, nm in enumerate(pre_names)})
    in_lib_order = lambda xs: sorted(dict.fromkeys(xs), key=lambda nm: lib_order.get(nm, (2, nm)))
    ref_trf.random = SimpleNamespace(choice=lambda xs: in_lib_order(xs)[0])
    ref_trf.set = in_lib_order

    hits_of = {}
    for rd in sorted(reads):
        cls, hits, _, _, _ = g8.classify(rd, seqs, pre)
        assert cls is not None, rd
        hits_of[rd] = (cls, hits)

    def reference_run(tmp):
        content, sums = {}, {"mature": [0] * 5, "primary": [0] * 5}
        for cls in ("mature", "primary"):
            for rd in sorted(reads):
                if hits_of[rd][0] != cls:
                    continue
                for i in range(5):
                    sums[cls][i] += reads[rd][i]
                content[rd] = {"count": list(reads[rd]), "uid": g8.UID(rd, "tRF") if "N" not in rd else "."}
                for r, o in hits_of[rd][1]:
                    nm = names[r] if cls == "mature" else pre_names[r]
                    d = dict(start=o, cigar="undifined", tRFType=g8.trfTypes(rd, nm, o, stru), end=o + len(rd) - 1)
                    if cls == "primary":
                        d["end"] -= len(rd) - re.search("T{3,}$", rd).span(0)[0]
                    content[rd][nm] = d
        ref_trf.trna_deliverables(SimpleNamespace(), tmp, pre_dic, content, sums["mature"], sums["primary"], aa_dic, SAMPLES, stru, dup,
                                  merged_list, trf_dic, merged_of)
        return sums

    # ---- counts nudged until no group has two equal float32 densities
    for attempt in range(200):
        tmp = tempfile.mkdtemp(prefix="golden_trf_clusters_")
        sums = reference_run(tmp)
        facts = {s: clustering_facts(os.path.join(tmp, "tRFs.samples.tmp", s + ".aligned_tRFs.report")) for s in SAMPLES}
        tied = [(s, f) for s in SAMPLES for f in facts[s] if f["tie"]]
        empty = []  # (sample, tRNA) whose rows were all dropped: load_data_new skips the block and every later name is off by one
        for s in SAMPLES:
            with open(os.path.join(tmp, "tRFs.samples.tmp", s + ".aligned_tRFs.report")) as fh:
                lines = fh.readlines()
            empty += [(s, ln.split("\t")[0]) for ln, nxt in zip(lines, lines[1:]) if "RP100K sum:" in ln and "tRNA" in nxt.split("\t")[1]]
        if not tied and not empty:
            break
        shutil.rmtree(tmp)
        if empty:
            s, nm = empty[0]
            p = pre[pre_names.index(nm)]
            reads[p[:len(p) - len(re.search("T+$", p).group(0))][-18:] + "TTT"][SAMPLES.index(s)] += 1
            continue
        s, f = tied[0]
        rho = f["rho"].tolist()
        k = next(i for i in range(len(rho)) if rho.count(rho[i]) > 1) + 1
        rd = f["info"][k]["allignedSeq"].strip("-")
        assert s in ("S1", "S2"), (s, rd)  # (the designed samples hold no tie as designed)
        reads[rd][SAMPLES.index(s)] += 1 + attempt % 3
    else:
        raise AssertionError("ties remain")
    print("attempts:", attempt + 1)

    # ---- the case stays inside what the reference defines, and holds what it is made for
    tdir = os.path.join(tmp, "tRFs.samples.tmp")
    details = {s: open(os.path.join(tdir, s + ".aligned_tRFs.clusters.detail")).read() for s in SAMPLES}
    tsv = {s: open(os.path.join(tdir, s + ".tRFs.report.tsv")).read().splitlines()[1:] for s in SAMPLES}
    for s in SAMPLES:
        with open(os.path.join(tdir, s + ".aligned_tRFs.report")) as fh:
            n_names = sum("RP100K sum:" in ln for ln in fh)
        assert n_names == len(facts[s]), (s, "a tRNA whose rows were all dropped: the reference pairs names by position")
        assert all(f["n"] >= 1 for f in facts[s])
    assert any(f["n"] == 1 for s in SAMPLES for f in facts[s])
    halo_border = halo_far = False
    for f in facts["S4"]:
        if f["n"] < 6:
            continue
        delta, nneigh, _, order = ref_trf.min_distance(f["dist"], f["max_dis"], f["n"], np.concatenate([[-1], f["rho"]]).astype(np.float32))
        rho = np.concatenate([[-1], f["rho"]]).astype(np.float32)
        centres = [i for i in range(1, f["n"] + 1) if rho[i] >= 5.0 and delta[i] >= 8.0]
        assert len(centres) == 2, centres
        cl = {c: k + 1 for k, c in enumerate(centres)}
        for i in order[:f["n"]]:
            cl.setdefault(int(i), cl.get(int(nneigh[i])))
        bord = {1: 0.0, 2: 0.0}
        for i in range(1, f["n"]):
            for j in range(i + 1, f["n"] + 1):
                if cl[i] != cl[j] and f["dist"][(i, j)] <= 3.0:
                    bord[cl[i]] = max(bord[cl[i]], (rho[i] + rho[j]) / 2)
                    bord[cl[j]] = max(bord[cl[j]], (rho[i] + rho[j]) / 2)
        for i in range(1, f["n"] + 1):
            far = f["dist"][(i, centres[cl[i] - 1])] > 8.0
            halo_border |= rho[i] < bord[cl[i]] and not far
            halo_far |= far and not rho[i] < bord[cl[i]]
    assert halo_border and halo_far
    assert "Number of Clusters: 0\n" in details["S5"] and "Number of Clusters: 2\n" in details["S4"]
    m7 = [b for b in details["S4"].split("##################################\n") if b.startswith(names[7] + ":")]
    assert m7 and "Number of Clusters: 1\n" in m7[0] and "Elements: 2 " in m7[0]   # (delta 3 and 3: a centre only by the fallback)
    total5 = sums["mature"][4] + sums["primary"][4]
    assert 100000.0 / total5 < 5.0
    assert names[9] + ":" in details["S5"] and not any(ln.startswith(names[9] + "\t") for ln in tsv["S5"])      # under the cutoff of 10
    assert any(ln.split("\t")[4] == "tRF-1" and ln.startswith(names[6] + "\t") for ln in tsv["S4"])             # selected as trailer ...
    assert any(ln.split("\t")[4] != "tRF-1" and ln.startswith(names[6] + "\t") for ln in tsv["S4"])             # ... and as mature
    assert any(ln.split("\t")[3].startswith("Y:") for s in SAMPLES for ln in tsv[s])
    assert any("N" in ln.split("\t")[0].strip("-") for s in SAMPLES for ln in open(os.path.join(tdir, s + ".aligned_tRFs.report")) if "\t" in ln and "sum:" not in ln)
    assert any(len(rd) > 64 and max(c) > 0 for rd, c in reads.items())

    # ---- write the inputs and the reference's files
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
    for i, s in enumerate(SAMPLES):
        seq_list = [rd for rd, c in reads.items() for _ in range(c[i])]
        seq_list += [mir[i % len(mir)]] * (3 + i) + [g8.rnd(rng, 30) for _ in range(4)]
        order = rng.permutation(len(seq_list)) if s not in RUN else np.arange(len(seq_list))
        text = "".join(f"@{'r' if s in RUN else k}\n{seq_list[j]}\n+\n{'I' * len(seq_list[j])}\n" for k, j in enumerate(order))
        if s in GZ:
            with open(os.path.join(OUT, f"{s}.fastq.gz"), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as fh:
                fh.write(text.encode())
        else:
            with open(os.path.join(OUT, f"{s}.fastq"), "w") as fh:
                fh.write(text)
    for f in FILES:
        shutil.copy(os.path.join(tmp, f), os.path.join(OUT, f))
    os.makedirs(os.path.join(OUT, "tRFs.samples.tmp"))
    for s in SAMPLES:
        for suffix in (".aligned_tRFs.report", ".aligned_tRFs.summary.report", ".aligned_tRFs.clusters.detail", ".tRFs.report.tsv"):
            shutil.copy(os.path.join(tdir, s + suffix), os.path.join(OUT, "tRFs.samples.tmp", s + suffix))
    shutil.rmtree(tmp)
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(OUT) for f in fs)
    print(f"{len(reads)} reads, groups per sample {[len(facts[s]) for s in SAMPLES]}, {size} bytes in {OUT}")
    assert size < 200 * 1024


if __name__ == "__main__":
    main()

"""tRNA fragment reports (``--trf-report``): the reference's ``-trf`` up to its per-sample reports -- summary.py:1060-1220 and
``trna_deliverables`` (mirge2_tRF_a2i.py:522-744) -- and, with ``--trf-clusters``, the density-peak clustering behind them (:745-947).

Written into the run's directory: ``tRFs.aligned.report.tsv``, ``tRF.Counts.csv``, ``tRF.RP100K.csv``,
``discarded.reads.summary.assigningtRFs.csv`` and, per sample, ``tRFs.samples.tmp/<sample>.aligned_tRFs.report`` and
``.aligned_tRFs.summary.report``; with ``--trf-clusters`` also ``<sample>.aligned_tRFs.clusters.detail`` and
``<sample>.tRFs.report.tsv``.  NOT written: the intermediate ``miRge3_tRNA.sam`` / ``miRge3_pre_tRNA.sam``.

The sequence work runs on the device (csrc/kernels_trf.hpp): every best-stratum alignment of every tRNA read
(``_ffi.trf_hits``: bowtie's ``-a --best --strata`` of passes 2 and 3, where the cascade keeps one alignment per read) and the
comparison of every report row with all predefined tRFs of its tRNA (``_ffi.trf_assign``: ``assign_cluster`` / ``getDistance2``).
The sums, the sorts and the text are host work in Python floats, so that ``'%.3f' % round(x, 3)`` rounds as the reference does.
The clustering's pair work -- all distances between the reads stacked on one tRNA, their densities, nearest denser points and border
densities -- runs on the device too (``_ffi.trf_cluster``); a point is a row of ``<sample>.aligned_tRFs.report`` with the RP100K the
report prints (``report_value``), taken from memory.  The float32 densities are the reference's bit for bit: the Gaussian comes from
a table of Python's ``math.exp`` and the double sum runs in the reference's order with product and sum rounded separately.  The
per-cluster sums, the ``repr`` of the float lists and the text of the two files are host work (``cluster_block``, ``write_clusters``).

Where the reference leaves the outcome to chance, this is the project's rule:

1. Several windows of one read on one reference: the reference's dict keeps whichever line bowtie printed last; here the lowest
   offset is kept.
2. Order of a read's references: bowtie's ``-a`` order in the reference; here library order.
3. ``random.choice(candidatetRNAUniquelist)`` (mirge2_tRF_a2i.py:563-567), and the order of that list itself (a ``set`` of
   strings): here the candidates -- the hit names mapped through ``_trna_deduplicated_list.csv``, made unique -- stand in library
   order (mature before ``pre_``, then the reference index) and the first one is chosen.

4. Points with equal float32 densities: ``np.argsort(-rho)`` leaves their order to NumPy's version and to the CPU; here they stand in
   index order (the sort made stable).
5. The reference pairs ``readInforList`` with ``tRNANameList`` by position although ``load_data_new`` skips a tRNA whose rows were all
   dropped, so every later block carries the name before its own; here such a tRNA writes no block and the names stay with their
   blocks.

A candidate that is not itself a hit of the read raises ``KeyError`` in the reference (:583); here the row is written from the
candidates that are hits, and ``run.log`` names the first such read.  A hit's type (``trfTypes``, summary.py:649-674) is decided by
the hit's class where the reference tests the name for ``'pre_'``; the two agree on the shipped libraries, whose primary
references, and only they, carry that prefix.  Everything else follows the reference as written, its substring tests (``'pre' not in
name``) and the ``len(filledSeq) == len(templateSeq)`` filter, which drops primary reads whose T run overhangs the trailer,
included."""
from __future__ import annotations

import os
import re
import time
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

TYPES = ("tRF-whole", "5'-half", "5'-tRF", "3'-half", "3'-tRF", "i-tRF", "tRF-1")  # csrc/kernels_trf.hpp: MIRGE_TRF_*
MATURE_PASS, PRIMARY_PASS = 2, 3
TRF_CLUSTER_MAXCOL = 256  # csrc/kernels_trf.hpp: MIRGE_TRF_CL_MAXCOL
FILES = ("_trna.str", "_trna_aminoacid_anticodon.csv", "_trna_deduplicated_list.csv", "_tRF_infor.csv", "_tRF_merges.csv")
_UID_ALPHABET = "BD0EF1HI2JK3LM4NO5PQ6RS7UV8WX9YZ"
_UID_OFFSET = (0, 0, 4, 20, 84)


def uid(seq: str, prefix: str = "tRF") -> str:
    """miRgeEssential.UID (:364-370): two symbols of a 32-letter alphabet per 5-mer, a shorter last chunk numbered after all
    shorter k-mers (the rule of csrc/native_host.hpp: uid_append)"""
    out = [prefix + "-" + str(len(seq)) + "-"]
    for at in range(0, len(seq), 5):
        chunk = seq[at:at + 5]
        v = 0
        for ch in chunk:
            v = v * 4 + "ACGT".index(ch)
        if len(chunk) < 5:
            v += _UID_OFFSET[len(chunk)]
        out.append(_UID_ALPHABET[v] if len(chunk) < 5 and v < 32 else _UID_ALPHABET[v // 32] + _UID_ALPHABET[v % 32])
    return "".join(out)


def add_dash(seq: str, total: int, start: int, end: int) -> str:
    return "-" * (start - 1) + seq + "-" * (total - end)


def coordinate(dashed: str) -> Tuple[int, int]:
    return len(dashed) - len(dashed.lstrip("-")) + 1, len(dashed.rstrip("-"))


class Annotation:
    """the five files of ``annotation.Libs`` as summary.py:1067-1159 reads them"""

    def __init__(self):
        self.stru: Dict[str, dict] = {}            # name -> seq, anticodonStart (1-based)
        self.aa: Dict[str, Tuple[str, str]] = {}   # name -> (amino acid, anticodon)
        self.dedup: Dict[str, str] = {}            # duplicate name -> the name that stands for it
        self.infor: Dict[str, Dict[str, str]] = {}  # tRNA -> {dashed string: cluster name}
        self.merged_list: List[str] = []
        self.merged_of: Dict[str, str] = {}


def load_annotation(libraries_path, organism: str, say: Callable[[str], None]) -> Optional[Annotation]:
    """-> the annotation, or None when one of the five files cannot be read: ``say`` then got the reference's line for each"""
    base = Path(libraries_path) / organism / "annotation.Libs"
    a = Annotation()
    ok = True

    def lines_of(suffix):
        nonlocal ok
        path = base / (organism + suffix)
        try:
            with open(path, "r") as fh:
                return fh.readlines()
        except IOError:
            ok = False
            say(f"File {path} does not exist!!\nProceeding the annotation with out -trf\n")
            return None

    lines = lines_of(FILES[0])
    if lines is not None:
        state, name, seq = 0, None, None
        for ln in lines:
            ln = ln.strip()
            if ln.startswith(">"):
                name = ln.replace(">", "")
                state += 1
            elif state == 1:
                state, seq = 2, ln
            elif state == 2:
                state = 0
                a.stru[name] = dict(seq=seq, stru=ln, anticodonStart=ln.index("XXX") + 1)
    lines = lines_of(FILES[1])
    for ln in lines or ():
        c = ln.strip().split(",")
        a.aa[c[0]] = (c[1], c[2])
    lines = lines_of(FILES[2])
    for ln in (lines or ())[1:]:
        c = ln.strip().split(",")
        for item in c[1].split("/"):
            a.dedup[item.strip()] = c[0].strip()
    lines = lines_of(FILES[3])
    for ln in (lines or ())[1:]:
        c = ln.strip().split(",")
        s, e = int(c[3].split("-")[0]), int(c[3].split("-")[1])
        a.infor.setdefault(c[0].split("_Cluster")[0], {})[add_dash(c[4], len(c[5]), s, e)] = c[0]  # (the same string again: the later line)
    lines = lines_of(FILES[4])
    for ln in lines or ():
        c = ln.strip().split(",")
        a.merged_list.append(c[0])
        for item in c[1].split("/"):
            a.merged_of[item] = c[0]
    return a if ok else None


class InforTables:
    """the predefined tRFs as the CSR ``_ffi.trf_assign`` takes: tRNAs in the order of ``infor``, a tRF's rank = the rank of its
    cluster name in Python's string order"""

    def __init__(self, infor: Dict[str, Dict[str, str]]):
        self.index = {name: k for k, name in enumerate(infor)}
        self.strings: List[bytes] = []
        self.names: List[str] = []
        ptr = [0]
        for name in infor:
            for s, cluster in infor[name].items():
                self.strings.append(s.encode())
                self.names.append(cluster)
            ptr.append(len(self.strings))
        self.ref_ptr = np.asarray(ptr, dtype=np.int64)
        rank_of = {nm: i for i, nm in enumerate(sorted(set(self.names)))}
        self.rank = np.asarray([rank_of[nm] for nm in self.names], dtype=np.int32)
        co = [coordinate(s.decode()) for s in self.strings]
        self.c_start = np.asarray([c[0] for c in co], dtype=np.int32)
        self.c_end = np.asarray([c[1] for c in co], dtype=np.int32)


def hits_by_row(reads: Sequence[str], rec: dict, mature_names: Sequence[str], primary_names: Sequence[str]) -> List[List[tuple]]:
    """the device's records (sorted by (row, ref, off)) -> per row [(name, start, end, type)] in library order, the lowest offset of
    a reference kept (rules 1 and 2); start / end 0-based, end without the T run for a primary hit (summary.py:1196-1216)"""
    out: List[List[tuple]] = [[] for _ in reads]
    last = (-1, -1)
    for row, ref, off, cls, ty in zip(rec["row"].tolist(), rec["ref"].tolist(), rec["off"].tolist(), rec["cls"].tolist(), rec["type"].tolist()):
        if (row, ref) == last:
            continue
        last = (row, ref)
        rd = reads[row]
        end = off + len(rd) - 1
        if cls:
            end -= len(rd) - re.search("T{3,}$", rd).span(0)[0]
        out[row].append(((primary_names if cls else mature_names)[ref], off, end, TYPES[ty]))
    return out


def write_reports(workDir, base_names: Sequence[str], reads: Sequence[str], counts, hits: List[List[tuple]], mature_sums, primary_sums,
                  ann: Annotation, pre_seqs: Dict[str, str], lib_order: Dict[str, tuple], assign: Callable, say: Callable[[str], None],
                  cluster: Optional[Callable] = None, tm: Optional[dict] = None) -> dict:
    """``trna_deliverables`` up to mirge2_tRF_a2i.py:744.  ``reads`` / ``counts`` / ``hits``: the report's rows in order (mature-tRNA
    rows of mapped.csv, then the primary-tRNA rows); ``lib_order``: name -> sort key of rule 3; ``assign(rows)`` with rows =
    [(row index, tRNA name, 1-based start)] -> (distances, tRF indices into ``InforTables(ann.infor)`` or -1).  ``cluster``
    (``--trf-clusters``): see ``write_clusters``; None: the clustering files are not written."""
    workDir = Path(workDir)
    S = len(base_names)
    counts = [[int(x) for x in row] for row in counts]
    rpm = []
    for row in counts:
        r = []
        for i in range(S):
            try:
                r.append((100000.0 * row[i]) / (int(mature_sums[i]) + int(primary_sums[i])))
            except ZeroDivisionError:
                r.append(0.0)
        rpm.append(r)
    info = lambda name, h: ":".join([name, h[3], str(h[1] + 1), str(h[2] + 1)])
    pre = lambda name, aa: "pre:" + aa if "pre_" in name else aa
    selected: List[Optional[tuple]] = [None] * len(reads)   # the one hit a row keeps
    printed: List[tuple] = []                                # (row, name, start, end, counts, RP100K as printed)
    not_a_hit = None
    with open(workDir / "tRFs.aligned.report.tsv", "w") as outf:
        outf.write('read sequence\tuid\tread count(%s)\tRP100K (%s)\tamino acid all hits\tamino acid-anticodon all hits\ttRF information all hits\t'
                   'amino acid all deduplicated hits\tamino acid-anticodon all deduplicated hits\ttRF information all deduplicated hits\t'
                   'amino acid one hit\tamino acid-anticodon one hit\ttRF information one hit\n' % (';'.join(base_names), ';'.join(base_names)))
        for k, seq in enumerate(reads):
            by_name = {h[0]: h for h in hits[k]}
            infos, aa_anticodons, aa_types = [], [], []
            for name, h in by_name.items():
                infos.append(info(name, h))
                aa = pre(name, ann.aa[name][0])
                if aa not in ("Und", "pre:Und"):
                    if aa + "-" + ann.aa[name][1] not in aa_anticodons:
                        aa_anticodons.append(aa + "-" + ann.aa[name][1])
                    if aa not in aa_types:
                        aa_types.append(aa)
            cand = sorted({ann.dedup.get(name, name) for name in by_name}, key=lambda nm: lib_order.get(nm, (2, nm)))
            if any(nm not in by_name for nm in cand):
                if not_a_hit is None:
                    not_a_hit = seq
                cand = [nm for nm in cand if nm in by_name]
            if not cand:
                continue
            one = cand[0]
            rp = ['%.3f' % (round(s, 3)) for s in rpm[k]]
            outf.write('\t'.join([seq, uid(seq) if "N" not in seq else ".", ';'.join(str(s) for s in counts[k]), ';'.join(rp)]))
            outf.write('\t' + '\t'.join([','.join(aa_types), ','.join(aa_anticodons), ','.join(infos)]) + '\t')
            d_types = [pre(nm, ann.aa[one][0]) for nm in cand]  # (the reference takes the amino acid of the ONE hit here, :577)
            outf.write('\t'.join([','.join(d_types), ','.join(t + '-' + ann.aa[nm][1] for t, nm in zip(d_types, cand)),
                                  ','.join(info(nm, by_name[nm]) for nm in cand)]) + '\t')
            aa_one = pre(one, ann.aa[one][0])
            outf.write('\t'.join([aa_one, aa_one + '-' + ann.aa[one][1]]) + '\t' + info(one, by_name[one]) + '\n')
            selected[k] = by_name[one]
            printed.append((k, one, by_name[one][1] + 1, by_name[one][2] + 1, counts[k], [float(x) for x in rp]))
    if not_a_hit is not None:
        say(f"tRF report: a deduplicated tRNA name is no alignment of read {not_a_hit} (the reference raises KeyError there): such names are left out\n")

    # ---- every printed row against the predefined tRFs of its tRNA (:603-657)
    tabs = InforTables(ann.infor)
    dist, idx = assign([(k, name, start) for k, name, start, _, _, _ in printed]) if printed else ((), ())
    entity = {s: {m: [0, 0.0] for m in ann.merged_list} for s in base_names}
    summary = {s: [0, 0] for s in base_names}
    for (k, name, start, end, cnt, rp), d, t in zip(printed, dist, idx):
        assigned = "Dele" if name not in ann.infor else (tabs.names[int(t)] if int(d) <= 8 else "Undef")
        for i, s in enumerate(base_names):
            summary[s][1] += cnt[i]
            if assigned not in ("Undef", "Dele"):
                m = ann.merged_of[assigned]
                entity[s][m][0] += cnt[i]
                entity[s][m][1] += rp[i]
            else:
                summary[s][0] += cnt[i]
    with open(workDir / "discarded.reads.summary.assigningtRFs.csv", "w") as outf:
        outf.write('sample name,percentage of discarded reads,details\n')
        for s in base_names:
            try:
                outf.write(s + ',%.2f%%,%d\\%d\n' % (round((float(summary[s][0]) / summary[s][1]) * 100.0, 2), summary[s][0], summary[s][1]))
            except ZeroDivisionError:
                outf.write(s + ',0.00%%,%d\\%d\n' % (summary[s][0], summary[s][1]))
    with open(workDir / "tRF.Counts.csv", "w") as o1, open(workDir / "tRF.RP100K.csv", "w") as o2:
        o1.write('entry name,' + ','.join(base_names) + '\n')
        o2.write('entry name,' + ','.join(base_names) + '\n')
        for m in ann.merged_list:
            o1.write(m + ',' + ','.join(str(entity[s][m][0]) for s in base_names) + '\n')
            o2.write(m + ',' + ','.join('%.2f' % (round(entity[s][m][1], 2)) for s in base_names) + '\n')

    # ---- per sample: the reads stacked on their tRNA, and the sums per amino acid (:659-744)
    tdir = workDir / "tRFs.samples.tmp"
    os.makedirs(tdir, exist_ok=True)
    template_of = lambda name: ann.stru[name]["seq"] if "pre" not in name else pre_seqs[name]
    per_sample: Dict[str, Dict[str, list]] = {s: {} for s in base_names}
    for k, seq in enumerate(reads):
        h = selected[k]
        if h is None:
            continue
        for i, s in enumerate(base_names):
            if counts[k][i] > 0:
                filled = h[1] * '-' + seq + (len(template_of(h[0])) - h[1] - len(seq)) * '-'
                per_sample[s].setdefault(h[0], []).append((counts[k][i], h[1], seq, filled, h[3], rpm[k][i], k))  # (k: behind what the sort looks at)
    blocks: Dict[str, list] = {s: [] for s in base_names}   # per sample, in the report's order: (tRNA, template, its printed rows)
    for s in base_names:
        aa_list, aa_sum = [], {}
        with open(tdir / (s + '.aligned_tRFs.report'), "w") as outf:
            sums = [(sum(t[0] for t in sets), name, sum(t[5] for t in sets)) for name, sets in per_sample[s].items()]
            sums.sort(reverse=True)
            for read_sum, name, rpm_sum in sums:
                aa = pre(name, ann.aa[name][0])
                for key in ([aa + ' tRF-1'] if 'pre:' in aa else [aa + " 5'", aa + " 3'", aa + " other"]):
                    if key not in aa_list:
                        aa_list.append(key)
                        aa_sum[key] = [0, 0, 0]
                per_sample[s][name].sort(reverse=True)
                outf.write(name + '\t' + 'read count sum:' + str(read_sum) + '\tRP100K sum:' + '%.3f' % (round(rpm_sum, 3)) + '\n')
                template = template_of(name)
                blocks[s].append((name, template, [t for t in per_sample[s][name] if len(t[3]) == len(template)]))
                for t in per_sample[s][name]:
                    if len(t[3]) == len(template):
                        outf.write(t[3] + '\t' + t[4] + '\t' + str(t[0]) + '\t' + '%.3f' % (round(t[5], 3)) + '\n')
                        if 'pre:' in aa:
                            key = aa + ' tRF-1'
                        else:
                            left, right = len(t[3]) - len(t[3].lstrip('-')), len(t[3]) - len(t[3].rstrip('-'))
                            key = aa + (" 5'" if left <= 2 else (" 3'" if right <= 2 else " other"))
                        aa_sum[key][0] = aa_sum[key][0] + t[0]
                        aa_sum[key][1] = aa_sum[key][1] + t[5]
                        aa_sum[key][2] = aa_sum[key][2] + 1
                outf.write(template + '\t' + ('mature tRNA' if 'pre' not in name else 'primary tRNA trailer') + '\t' + str(read_sum) + '\t' +
                           '%.3f' % (round(rpm_sum, 3)) + '\n')
        with open(tdir / (s + '.aligned_tRFs.summary.report'), "w") as outf:
            outf.write('amino acid\tCounts\tRP100K\tUnique reads\n')
            for key in aa_list:
                outf.write('\t'.join([key, str(aa_sum[key][0]), '%.3f' % (round(aa_sum[key][1], 3)), str(aa_sum[key][2])]) + '\n')
    out = dict(rows=len(reads), printed=len(printed), discarded={s: tuple(summary[s]) for s in base_names})
    if cluster is not None:
        out["clusters"] = write_clusters(tdir, base_names, blocks, cluster, ann, pre_seqs, tm)
    return out


class TemplateTooLong(ValueError):
    """``--trf-clusters``: a tRNA (or a primary tRNA with its leader and trailer) has more columns than the clustering kernels take"""


def report_value(x: float) -> float:
    """an RP100K as ``load_data_new`` reads it back from <sample>.aligned_tRFs.report"""
    return float('%.3f' % round(x, 3))


def detect_mismatch(target: str, template: str, position: str) -> Tuple[str, str]:
    """detectMismach (mirge2_tRF_a2i.py:215-228)"""
    start, end = int(position.split(':')[0]) - 1, int(position.split(':')[1]) - 1
    tmp = template[start:end + 1]
    pos = [str(start + 1 + i) for i in range(min(len(target), len(tmp))) if target[i] != tmp[i]]
    return ('Y' if pos else 'N'), ','.join(pos)


def cluster_block(name: str, pts: Sequence[tuple], cl: Sequence[int], halo: Sequence[int], nclust: int, centre: Sequence[int]):
    """one tRNA's block of <sample>.aligned_tRFs.clusters.detail (mirge2_tRF_a2i.py:840-924).  ``pts``: (dashed string, type, count,
    RP100K) per point; ``cl`` / ``halo``: per point, 0-based lists of the 1-based cluster numbers; ``centre``: the 1-based index of
    every cluster's centre -> (text, [(sequence, type, 'start:end', count, RP100K)] per written cluster, the block's RP100K)"""
    n = len(pts)
    text = [name + ':\n']
    sum_count, sum_rp = 0, 0.0
    core_c, halo_c, core_r, halo_r, content = [], [], [], [], []
    number = 1
    if nclust >= 1:
        for i in range(1, nclust + 1):
            c = centre[i - 1] - 1
            nc, select, t_halo_c, t_halo_r = 0, [], 0, 0.0
            for j in range(n):
                if cl[j] == i:
                    nc += 1
                if halo[j] == i:
                    select.append(j)
                if cl[j] == i and halo[j] != i:
                    t_halo_c = t_halo_c + pts[j][2]
                    t_halo_r = t_halo_r + pts[j][3]
            nh = len(select)
            t_core_c, t_core_r = 0, 0.0
            for j in select:
                t_core_c = t_core_c + pts[j][2]
                t_core_r = t_core_r + pts[j][3]
            if t_core_c > 0:
                # (the reference sorts (count, the CENTRE's string, the CENTRE's type) tuples: whichever count is largest, the
                # sequence, the type and the coordinates are the centre's)
                seq = pts[c][0]
                head, tail = len(seq) - len(seq.lstrip('-')), len(seq) - len(seq.rstrip('-'))
                text.append('Cluster: %d Total Read Count in Core: %d Total Read Count in Halo: %d Total RP100K in Core: %.2f Total RP100K in Halo: '
                            '%.2f Center Index: %d Elements: %d Core: %d Halo: %d\n' % (number, t_core_c, t_halo_c, t_core_r, t_halo_r, c + 1, nc, nh, nc - nh))
                text.append('Center:\n')
                text.append('%s\t%s\t%d\t%.2f\n' % pts[c][:4])
                a_count, a_rp = 0 + pts[c][2], 0.0 + pts[c][3]
                for j in select:
                    if j != c:
                        text.append('%s\t%s\t%d\t%.2f\n' % pts[j][:4])
                        a_count = a_count + pts[j][2]
                        a_rp = a_rp + pts[j][3]
                text.append('**********************************\n')
                content.append((seq[head:len(seq) - tail], pts[c][1], ':'.join([str(head + 1), str(len(seq) - tail)]), a_count, a_rp))
                number += 1
            sum_count = sum_count + t_halo_c + t_core_c
            sum_rp = sum_rp + t_halo_r
            sum_rp = sum_rp + t_core_r
            core_c.append(t_core_c); halo_c.append(t_halo_c); core_r.append(t_core_r); halo_r.append(t_halo_r)
    else:
        for j in range(n):
            sum_count = sum_count + pts[j][2]
            sum_rp = sum_rp + pts[j][3]
    text.append('Summary:\nNumber of Clusters: %d\n' % (number - 1))
    text.append('total Read Count : %d\n' % sum_count)
    text.append('total RP100K: %.2f\n' % sum_rp)
    text.append('total Cluster Core Read Count: %s=%d\n' % ('+'.join(str(x) for x in core_c), sum(core_c)))
    text.append('total Cluster Core RP100K: %s=%.3f\n' % ('+'.join(str(x) for x in core_r), sum(core_r)))
    text.append('total Cluster Halo Read Count: %s=%d\n' % ('+'.join(str(x) for x in halo_c), sum(halo_c)))
    text.append('total Cluster Halo RP100K: %s=%.3f\n' % ('+'.join(str(x) for x in halo_r), sum(halo_r)))
    text.append('##################################\n')
    return ''.join(text), content, sum_rp


def write_clusters(tdir, base_names: Sequence[str], blocks: Dict[str, list], cluster: Callable, ann: Annotation, pre_seqs: Dict[str, str],
                   tm: Optional[dict] = None) -> dict:
    """the rest of ``trna_deliverables`` (mirge2_tRF_a2i.py:745-947): <sample>.aligned_tRFs.clusters.detail and <sample>.tRFs.report.tsv.
    ``blocks``: per sample (tRNA, template, rows of ``write_reports``); ``cluster(groups)`` with groups = [dict(tlen, rows, off, rp,
    dashed)] -> the arrays of ``_ffi.trf_cluster`` over the groups' points in order."""
    tm = tm if tm is not None else {}
    groups, owner = [], []
    for s in base_names:
        for name, template, rows in blocks[s]:
            if not rows:
                continue  # (rule 5: a tRNA whose rows were all dropped writes no block (the reference shifts every later name by one))
            if len(template) > TRF_CLUSTER_MAXCOL:
                raise TemplateTooLong(f"--trf-clusters: {name} has {len(template)} columns, the clustering takes at most {TRF_CLUSTER_MAXCOL}")
            groups.append(dict(tlen=len(template), rows=[t[6] for t in rows], off=[t[1] for t in rows], rp=[report_value(t[5]) for t in rows],
                               dashed=[t[3] for t in rows]))
            owner.append((s, name, [(t[3], t[4], t[0], rp) for t, rp in zip(rows, groups[-1]["rp"])]))
    t0 = time.perf_counter()
    res = cluster(groups) if groups else None
    tm["trf_cluster_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ptr = np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum([len(g["rows"]) for g in groups], out=ptr[1:])
    at = 0
    n_clusters = {}
    for s in base_names:
        selected, unified, content_of = [], [], {}
        with open(Path(tdir) / (s + '.aligned_tRFs.clusters.detail'), "w") as o1:
            while at < len(owner) and owner[at][0] == s:
                _, name, pts = owner[at]
                lo, hi = int(ptr[at]), int(ptr[at + 1])
                nclust = int(res["nclust"][at])
                text, content, sum_rp = cluster_block(name, pts, res["cl"][lo:hi].tolist(), res["halo"][lo:hi].tolist(), nclust,
                                                      res["centre"][lo:lo + nclust].tolist())
                o1.write(text)
                content_of[name] = content
                n_clusters[(s, name)] = len(content)
                if sum_rp >= 10.0:
                    selected.append(name)
                    u = '_'.join(name.split('_')[1:-1]) if 'pre' in name else name
                    if u not in unified:
                        unified.append(u)
                at += 1
        with open(Path(tdir) / (s + '.tRFs.report.tsv'), "w") as o2:
            o2.write('tRNA name\ttRNA sequence\ttRF sequence\ttRF mismatch\ttRF type\ttRF coordinate\tRead count\tRP100K\n')
            for u in unified:
                if u in selected:
                    seq = ann.stru[u]['seq']
                    for c in content_of[u]:
                        o2.write(u + '\t' + seq + '\t' + c[0] + '\t' + ':'.join(detect_mismatch(c[0], seq, c[2])) + '\t' + c[1] + '\t' + c[2] + '\t' +
                                 str(c[3]) + '\t' + '%.2f' % (round(c[4], 2)) + '\n')
                pname = 'pre_' + u + '_trailer'
                if pname in selected:
                    seq = pre_seqs[pname]
                    for c in content_of[pname]:
                        pos = ':'.join([c[2].split(':')[0], str(int(c[2].split(':')[1]) - 3)])
                        o2.write(u + '\t' + seq + '\t' + c[0] + '\t' + ':'.join(detect_mismatch(c[0][:-3], seq, pos)) + '\t' + c[1] + '\t' + c[2] + '\t' +
                                 str(c[3]) + '\t' + '%.2f' % (round(c[4], 2)) + '\n')
    tm["trf_cluster_text_s"] = time.perf_counter() - t0
    return dict(groups=len(groups), points=int(ptr[-1]), clusters=n_clusters)


def library_order(mature_names: Sequence[str], primary_names: Sequence[str]) -> Dict[str, tuple]:
    """rule 3's sort key: mature before ``pre_``, then the reference index"""
    order = {nm: (1, i) for i, nm in enumerate(primary_names)}
    order.update({nm: (0, i) for i, nm in enumerate(mature_names)})
    return order


def run(args, workDir, base_names, casc, uniq, res, order, class_sums, tm=None) -> Optional[dict]:
    """``--trf-report`` of a single-process run, called from ``fastpath.reports`` behind the per-read CSVs.  ``order``: the row
    order of mapped.csv (handle indices), ``class_sums`` [n_pass, S]: the RP100K denominators (mirge2_tRF_a2i.py:530)."""
    from . import _ffi
    tm = tm if tm is not None else {}
    t0 = time.perf_counter()
    workDir = Path(workDir)
    with open(workDir / "run.log", "a+") as log:
        def say(msg):
            if not getattr(args, "quiet", False):
                print(msg)
            log.write(msg + "\n")
        ann = load_annotation(args.libraries_path, args.organism_name, say)
        if ann is None:
            return None
        mlib, plib = casc.libs["mature_trna"], casc.libs["pre_trna"]
        ctx = casc.ctx
        ps, _, _, _ = res.fetch()
        order = np.asarray(order, dtype=np.int64)
        rows = np.concatenate([order[ps[order] == MATURE_PASS], order[ps[order] == PRIMARY_PASS]])  # summary.py:1061-1066,1181
        missing = [nm for nm in mlib.names if nm not in ann.stru]
        if missing:
            raise KeyError(f"--trf-report: {missing[0]} of the mature tRNA library has no entry in {args.organism_name}{FILES[0]}")
        anticodon = np.asarray([ann.stru[nm]["anticodonStart"] - 1 for nm in mlib.names], dtype=np.int32)
        t = time.perf_counter()
        rec = _ffi.trf_hits(ctx, uniq, res, MATURE_PASS, casc.dev_libs[MATURE_PASS], casc.policies[MATURE_PASS], PRIMARY_PASS,
                            casc.dev_libs[PRIMARY_PASS], casc.policies[PRIMARY_PASS], rows, anticodon)
        tm["trf_hits_s"] = time.perf_counter() - t
        reads = uniq.unpack().take(rows).to_list() if rows.size else []
        counts = _ffi.trf_row_counts(ctx, uniq, rows)  # (the tRNA rows alone, not the whole matrix)
        hits = hits_by_row(reads, rec, mlib.names, plib.names)
        tabs = InforTables(ann.infor)

        def assign(arows):
            t1 = time.perf_counter()
            out = _ffi.trf_assign(ctx, uniq, res, [rows[k] for k, _, _ in arows], [tabs.index.get(nm, -1) for _, nm, _ in arows],
                                  [st for _, _, st in arows], tabs.ref_ptr, tabs.strings, tabs.c_start, tabs.c_end, tabs.rank)
            tm["trf_assign_s"] = time.perf_counter() - t1
            return out

        def cluster(groups):
            ptr = np.zeros(len(groups) + 1, dtype=np.int64)
            np.cumsum([len(g["rows"]) for g in groups], out=ptr[1:])
            return _ffi.trf_cluster(ctx, uniq, ptr, [rows[k] for g in groups for k in g["rows"]], [o for g in groups for o in g["off"]],
                                    [x for g in groups for x in g["rp"]], [g["tlen"] for g in groups])

        pre_seqs = dict(zip(plib.names, plib.seqs.to_list()))
        too_long = [nm for nm, sq in list(zip(mlib.names, mlib.seqs.to_list())) + list(pre_seqs.items()) if len(sq) > TRF_CLUSTER_MAXCOL] \
            if getattr(args, "trf_clusters", False) else []
        if too_long:  # (before anything is written)
            raise TemplateTooLong(f"--trf-clusters: {too_long[0]} has more than {TRF_CLUSTER_MAXCOL} columns")
        out = write_reports(workDir, list(base_names), reads, counts, hits, class_sums[MATURE_PASS], class_sums[PRIMARY_PASS], ann, pre_seqs,
                            library_order(mlib.names, plib.names), assign, say, cluster if getattr(args, "trf_clusters", False) else None, tm)
    tm["trf_report_s"] = time.perf_counter() - t0
    return out

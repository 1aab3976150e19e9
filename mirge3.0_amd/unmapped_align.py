"""``--unmapped-align``: the unmapped reads of a sample against the sequences of its own clusters -- the last stretch of the
reference's ``-nmir`` that is alignment work (mirge/libs/novel_mir.py:152-210,362-421, mirge/libs/processSam.py), without
bowtie-build, bowtie or sort:

    <sample>_clusters.tsv --preTrimClusteredSeq--> <sample>clusters_trimmed.tsv, <sample>_clusters_trimmed_orig.fa
    the kept clusters --bowtie-build-->                                                   (mirge_genome_create, one reference each)
    unmapped_mirna_<sample>.fa --bowtie -n 0 --best -a --norc -m <mloc> -l <sl>--> <sample>_tmp1.sam     (mirge_genome_align_loci)
                 --split_fasta_from_sam--> <sample>_imperfectMath2Cluster.fa
                 --bowtie -n 1 -l 15 -5 1 -3 3 --best --strata -a --norc--> <sample>_tmp2.sam     (mirge_genome_align_loci_strata)
    combineSam, decorateSam (twice), parse_refine_sam, sort -k6,6 -k1,1 (twice)

The alignments come from the device; the text around them is made here.  ``sort`` is restated in byte order (``LC_ALL=C``):
field 6, then field 1, then the whole line.
"""
import os
import pickle
import re
import time
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np

from .unmapped import MAXTOTAL, revcomp, settings as cluster_settings

CLC = 30  # -clc, mirge/libs/parse.py:136
RUN2 = dict(n_mm=1, seedlen=15, trim5=1, trim3=3)  # novel_mir.py:403
_POLY_A_END, _POLY_T_START = re.compile("A{6,}$"), re.compile("^T{6,}")


def settings(args) -> dict:
    """the six values of ``--unmapped-clusters`` and -clc"""
    out = cluster_settings(args)
    v = getattr(args, "ignored_clc", None)
    out["clc"] = int(v) if v is not None else CLC
    return out


def load_repeats(path) -> dict:
    """``<org>_genome_repeats.pckl``: {chromosome: [[k-d tree over (start, 0)], [(start, end, name), ...]]}; a missing file means
    no repeats (novel_mir.py:261-265).  The trees are scipy's, so scipy is needed exactly when the file exists."""
    if not os.path.exists(path):
        return {}
    try:
        import scipy.spatial  # noqa: F401  (the pickle names scipy.spatial's k-d tree)
    except ImportError as e:
        raise RuntimeError(f"{path} holds scipy k-d trees: --unmapped-align needs scipy to read it") from e
    with open(path, "rb") as fh:
        return pickle.load(fh)


def read_fasta(path) -> Tuple[List[str], List[str]]:
    names, seqs = [], []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if line.startswith(">"):
                names.append(line[1:].split()[0] if line[1:].split() else "")
                seqs.append("")
            elif names:
                seqs[-1] += line
    return names, seqs


def _overlaps(el, start: int, end: int) -> bool:
    return max(int(el[0]), start) <= min(int(el[1]), end)


def pretrim_clusters(repeats: dict, cluster_file, clc: int, out_tsv, out_fa) -> Tuple[List[str], List[str]]:
    """``preTrimClusteredSeq`` (novel_mir.py:152-210): every cluster with its original-strand sequence, a keep flag and the
    repeat element's name -> ``out_tsv``; the kept ones -> ``out_fa``.  Kept: at most ``clc`` long, no A{6,} at the end and no
    T{6,} at the start of the original-strand sequence, and no overlap with the two repeat elements whose starts are nearest
    to the cluster's start (one element when the chromosome has one; the name is the nearest's when that overlaps, else the
    second's).  -> names and sequences of the kept clusters"""
    names, seqs, rows, fa = [], [], [], []
    with open(cluster_file) as fh:
        head = fh.readline()
        rows.append("\t".join(["miRClusterID\tOriginalSeq\tFlag\trepetitiveElementName"] + head.split("\t")[1:]))
        for line in fh:
            c = line.strip().split("\t")
            flag, rep = "0", "*"
            orig = revcomp(c[5]) if c[2] == "-" else c[5]
            if int(c[6]) <= clc:
                chrom, start, end = c[1], int(c[3]), int(c[4])
                if _POLY_A_END.search(orig) is None and _POLY_T_START.search(orig) is None:
                    if chrom in repeats:
                        tree, elements = repeats[chrom][0][0], repeats[chrom][1]
                        dist, idx = tree.query([(start, 0)], 2)
                        first = elements[idx[0][0]]
                        if np.isfinite(dist[0][0]) and np.isfinite(dist[0][1]):
                            second = elements[idx[0][1]]
                            if _overlaps(first, start, end):
                                rep = first[2]
                            elif _overlaps(second, start, end):
                                rep = second[2]
                            else:
                                flag = "1"
                        elif _overlaps(first, start, end):
                            rep = first[2]
                        else:
                            flag = "1"
                    else:
                        flag = "1"
            rows.append("\t".join([c[0], orig, flag, rep] + c[1:]) + "\n")
            if flag == "1":
                nm = f"{c[0]}:{chrom}:{start}_{end}{c[2]}"
                names.append(nm)
                seqs.append(orig)
                fa.append(f">{nm}\n{orig}\n")
    with open(out_tsv, "w") as fh:
        fh.write("".join(rows))
    with open(out_fa, "w") as fh:
        fh.write("".join(fa))
    return names, seqs


def cluster_sam_text(names: Sequence[str], seqs: Sequence[str], loci: dict, ref_names: Sequence[str], ref_lens, command: str = "",
                     trim5: int = 0, trim3: int = 0) -> str:
    """one cluster run as SAM, the fields of ``unmapped.sam_text``: the reads in FASTA order, a read's alignments by (reference,
    offset), every one with flag 0 (--norc), a read without a reported alignment as its flag-4 line in place (XM:i:1: more
    than -m alignments).  The sequence is the read as it was aligned: ``trim5`` / ``trim3`` bases cut"""
    out = ["@HD\tVN:1.0\tSO:unsorted"]
    out += [f"@SQ\tSN:{n}\tLN:{int(ln)}" for n, ln in zip(ref_names, ref_lens)]
    out.append(f"@PG\tID:mirge3.0_amd\tPN:mirge_genome_align_loci\tCL:\"{command}\"")
    q = loci["query"].astype(np.int64)
    order = np.lexsort((loci["off"].astype(np.int64), loci["ref"].astype(np.int64), q))
    q, r, o, mm = q[order].tolist(), loci["ref"][order].tolist(), loci["off"][order].tolist(), loci["mm"][order].tolist()
    k, n_rec = 0, len(q)
    for i, name in enumerate(names):
        s = seqs[i][trim5:len(seqs[i]) - trim3]
        if k < n_rec and q[k] == i:
            while k < n_rec and q[k] == i:
                out.append(f"{name}\t0\t{ref_names[r[k]]}\t{o[k] + 1}\t255\t{len(s)}M\t*\t0\t0\t{s}\t{'I' * len(s)}\tNM:i:{mm[k]}")
                k += 1
        else:
            out.append(f"{name}\t4\t*\t0\t0\t*\t*\t0\t0\t{s or '*'}\t{'I' * len(s) or '*'}\tXM:i:{1 if loci['capped'][i] else 0}")
    return "\n".join(out) + "\n"


def split_fasta_from_sam(sam_path, names: Sequence[str], seqs: Sequence[str], out_fa) -> Tuple[List[str], List[str]]:
    """``split_fasta_from_sam``: the reads without a flag-0 / 16 line, in FASTA order.  A read over -m has none either and goes
    along, as in the reference"""
    aligned = set()
    with open(sam_path) as fh:
        for line in fh:
            if line[0] != "@":
                f = line.split("\t", 2)
                if f[1] in ("0", "16"):
                    aligned.add(f[0])
    keep = [i for i, n in enumerate(names) if n not in aligned]
    with open(out_fa, "w") as fh:
        fh.write("".join(f">{names[i]}\n{seqs[i]}\n" for i in keep))
    return [names[i] for i in keep], [seqs[i] for i in keep]


def combine_sam(tmp1, tmp2, out_path):
    """``combineSam``: the first file's header and aligned lines, then every line of the second but its header"""
    with open(out_path, "w") as out:
        with open(tmp1) as fh:
            for line in fh:
                if line[0] == "@" or line.strip().split("\t")[1] in ("0", "16"):
                    out.write(line)
        with open(tmp2) as fh:
            for line in fh:
                if line[0] != "@":
                    out.write(line)


def decorate_sam(sam_path, read_seqs: Dict[str, str], out_path, cluster_seqs: Dict[str, str] = None):
    """``decorateSam``: name, count (the name's last ``_`` field), read sequence[, cluster sequence or ``*``] in front of the
    line's fields from the second on; header lines as they are"""
    with open(sam_path) as fh, open(out_path, "w") as out:
        for line in fh:
            if line[0] == "@":
                out.write(line)
                continue
            f = line.strip().split("\t")
            head = [f[0], f[0].split("_")[-1], read_seqs[f[0]]]
            if cluster_seqs is not None:
                head.append(cluster_seqs.get(f[2], "*"))
            out.write("\t".join(head + f[1:]) + "\n")


def parse_refine_sam(modified_sam, selected, reverse_kept):
    """``parse_refine_sam``: flag 0 / 256 lines to both files, 16 / 272 to the second"""
    with open(modified_sam) as fh, open(selected, "w") as o1, open(reverse_kept, "w") as o2:
        for line in fh:
            if line[0] == "@":
                continue
            flag = line.strip().split("\t")[4]
            if flag in ("0", "256"):
                o1.write(line)
                o2.write(line)
            elif flag in ("16", "272"):
                o2.write(line)


def sort_tsv(src, dst):
    """``sort -k6,6 -k1,1`` in byte order (LC_ALL=C): field 6, then field 1, then the whole line"""
    with open(src, "rb") as fh:
        lines = fh.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()

    def key(ln):
        f = ln.split(b"\t")
        return (f[5] if len(f) > 5 else b"", f[0], ln)
    lines.sort(key=key)
    with open(dst, "wb") as fh:
        fh.write(b"".join(ln + b"\n" for ln in lines))


def align_sample(ctx, sample: str, out_dir, names: Sequence[str], seqs: Sequence[str], repeats: dict, p: dict, log: list = None) -> dict:
    """one sample after ``<sample>_clusters.tsv`` exists; ``names`` / ``seqs`` = ``unmapped_mirna_<sample>.fa``"""
    from . import _ffi
    from .a2i import GpuGenome
    from .seqio import FlatSeqs
    out_dir = Path(out_dir)
    t0 = time.perf_counter()
    fa = out_dir / f"{sample}_clusters_trimmed_orig.fa"
    c_names, c_seqs = pretrim_clusters(repeats, out_dir / f"{sample}_clusters.tsv", p["clc"], out_dir / f"{sample}clusters_trimmed.tsv", fa)
    t_trim = time.perf_counter() - t0
    res = dict(kept=len(c_names), reads=len(names), aligned1=0, capped=0, imperfect=0, aligned2=0)
    if not c_names:
        if log is not None:
            log.append(f"No cluster sequences are generated and prediction is aborted for {sample}.\n")
        return res
    t = time.perf_counter()
    dev = _ffi.DeviceGenome(ctx, seqs=FlatSeqs.from_list(list(c_seqs)))
    try:
        g = GpuGenome(ctx, dev)
        t_build = time.perf_counter() - t
        c_lens = [len(s) for s in c_seqs]
        t = time.perf_counter()
        l1 = g.loci(seqs, n_mm=0, seedlen=p["sl"], maxtotal=MAXTOTAL, max_loci=p["mloc"], norc=True)
        t_run1 = time.perf_counter() - t
        l1["capped"] = (l1["totals"] > p["mloc"]) if p["mloc"] else np.zeros(len(names), dtype=bool)
        tmp1, tmp2 = out_dir / f"{sample}_tmp1.sam", out_dir / f"{sample}_tmp2.sam"
        with open(tmp1, "w") as fh:
            fh.write(cluster_sam_text(names, seqs, l1, c_names, c_lens, f"-f -n 0 --best -a --norc -m {p['mloc']} -l {p['sl']} -S"))
        i_names, i_seqs = split_fasta_from_sam(tmp1, names, seqs, out_dir / f"{sample}_imperfectMath2Cluster.fa")
        t = time.perf_counter()
        l2 = g.loci(i_seqs, maxtotal=MAXTOTAL, norc=True, strata=True, **RUN2)
        t_run2 = time.perf_counter() - t
        l2["capped"] = np.zeros(len(i_names), dtype=bool)
    finally:
        dev.close()
    t = time.perf_counter()
    with open(tmp2, "w") as fh:
        fh.write(cluster_sam_text(i_names, i_seqs, l2, c_names, c_lens, "-f -n 1 -l 15 -5 1 -3 3 --best --strata -a --norc -S",
                                  RUN2["trim5"], RUN2["trim3"]))
    combined, modified = out_dir / f"{sample}.sam", out_dir / f"{sample}_modified.sam"
    combine_sam(tmp1, tmp2, combined)
    read_seqs = dict(zip(names, seqs))
    decorate_sam(combined, read_seqs, modified, dict(zip(c_names, c_seqs)))
    decorate_sam(out_dir / f"unmapped_mirna_{sample}_vs_genome_sorted.sam", read_seqs, out_dir / f"{sample}_RepSeq_modified.sam")
    sel, rev = out_dir / f"{sample}_selected.tsv", out_dir / f"{sample}_selected_reverseKept.tsv"
    parse_refine_sam(modified, sel, rev)
    sort_tsv(sel, out_dir / f"{sample}_modified_selected_sorted.tsv")
    sort_tsv(rev, out_dir / f"{sample}_modified_selected_reverseKept_sorted.tsv")
    t_text = time.perf_counter() - t
    res.update(aligned1=int(np.unique(l1["query"]).shape[0]), capped=int(l1["capped"].sum()), imperfect=len(i_names),
               aligned2=int(np.unique(l2["query"]).shape[0]), alignments1=int(l1["query"].shape[0]), alignments2=int(l2["query"].shape[0]))
    if log is not None:
        log.append(f"unmapped align, {sample}: {res['kept']} clusters kept, {res['reads']} reads: {res['aligned1']} exact "
                   f"({res['capped']} over -m {p['mloc']}), {res['imperfect']} to the second run, {res['aligned2']} aligned there; "
                   f"filter {t_trim:.3f} s, cluster genome {t_build:.3f} s, run 1 {t_run1:.3f} s, run 2 {t_run2:.3f} s, text {t_text:.3f} s\n")
    return res


def repeats_path(args) -> Path:
    return Path(args.libraries_path) / args.organism_name / "annotation.Libs" / (str(args.organism_name) + "_genome_repeats.pckl")


def run(args, ctx, workDir, base_names: Sequence[str], tm: dict = None) -> dict:
    """The whole step after ``unmapped.run`` wrote ``unmapped_tmp/``: every sample's FASTA and cluster file are read back from there."""
    t0 = time.perf_counter()
    workDir = Path(workDir)
    out_dir = workDir / "unmapped_tmp"
    p = settings(args)
    repeats = load_repeats(repeats_path(args))
    log, result = [], {}
    for sample in base_names:
        names, seqs = read_fasta(out_dir / f"unmapped_mirna_{sample}.fa")
        result[sample] = align_sample(ctx, sample, out_dir, names, seqs, repeats, p, log)
    seconds = time.perf_counter() - t0
    with open(workDir / "run.log", "a+") as fh:
        fh.write("".join(log) + f"unmapped align: {seconds:.3f} s\n")
    if tm is not None:
        tm["unmapped_align_s"] = seconds
    return result

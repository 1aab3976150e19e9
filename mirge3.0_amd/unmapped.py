"""``--unmapped-clusters``: where the reads the cascade could not annotate pile up on the genome -- the front half of the
reference's ``-nmir`` (mirge/libs/novel_mir.py:41-150,340-362) without bowtie or samtools:

    unmapped.csv --convert2Fasta--> unmapped_tmp/unmapped_mirna[_raw|_<sample>].fa
                 --bowtie <org>_genome -f -n 0 --best -a -m <mloc> -l <sl> -S, samtools sort-->   (mirge_genome_align_loci)
                 unmapped_mirna_<sample>_vs_genome_sorted.sam
                 --cluster_basedon_location--> <sample>_clusters.tsv                               (mirge_loci_cluster)

The alignments and the cluster boundaries come from the device; the text around them (FASTA names, SAM lines, the clusters'
sequences, which are built from the members' read sequences, :109-114) is made here.  ``cluster_scan`` is the kernel's
formulation in numpy: tests compare both with a sequential restatement, nothing in a run calls it in the kernel's place.
"""
import os
import time
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np

DEFAULTS = dict(minl=16, maxl=25, c=2, mloc=3, sl=25, olc=14)  # mirge/libs/parse.py:130-135
MAXTOTAL = 2  # bowtie's -e 70 over FASTA's Q40 calls: two mismatches past the seed
_RC = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def revcomp(s: str) -> str:
    return s.translate(_RC)[::-1]


def read_unmapped_csv(path, base_names: Sequence[str]) -> Tuple[List[str], np.ndarray]:
    """rows of ``unmapped.csv`` in file order: sequences and their counts per sample"""
    seqs: List[str] = []
    rows: List[List[int]] = []
    with open(path) as fh:
        head = fh.readline().rstrip("\n").split(",")
        cols = [head.index(b) for b in base_names]
        for line in fh:
            f = line.rstrip("\n").split(",")
            if f == [""]:
                continue
            seqs.append(f[0])
            rows.append([int(float(f[c])) for c in cols])
    return seqs, np.array(rows, dtype=np.int64).reshape(len(seqs), len(base_names))


def convert2fasta(seqs: Sequence[str], counts: np.ndarray, base_names: Sequence[str], minl: int, maxl: int, cutoff: int, outdir):
    """``convert2Fasta`` (novel_mir.py:41-79): ``unmapped_mirna_raw.fa`` (every row, ``mir<row>_<sum>``, rows numbered from 1),
    ``unmapped_mirna.fa`` (length in [minl, maxl] and sum >= cutoff) and per sample ``unmapped_mirna_<sample>.fa``: the rows of
    the filtered frame whose count IN THAT SAMPLE is >= cutoff too, named ``mir<row>_<count in the sample>``.
    -> {sample: (names, sequences)}, raw counts, filtered counts"""
    outdir = Path(outdir)
    total = counts.sum(axis=1)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    keep = (lens >= minl) & (lens <= maxl) & (total >= cutoff)
    with open(outdir / "unmapped_mirna_raw.fa", "w") as fh:
        fh.write("".join(f">mir{i + 1}_{int(total[i])}\n{s}\n" for i, s in enumerate(seqs)))
    with open(outdir / "unmapped_mirna.fa", "w") as fh:
        fh.write("".join(f">mir{i + 1}_{int(total[i])}\n{seqs[i]}\n" for i in np.nonzero(keep)[0]))
    per, raw_n, filt_n = {}, {}, {}
    for s, name in enumerate(base_names):
        raw_n[name] = int((counts[:, s] >= 1).sum())
        idx = np.nonzero(keep & (counts[:, s] >= cutoff))[0]
        filt_n[name] = int(idx.size)
        names = [f"mir{i + 1}_{int(counts[i, s])}" for i in idx]
        sq = [seqs[i] for i in idx]
        with open(outdir / f"unmapped_mirna_{name}.fa", "w") as fh:
            fh.write("".join(f">{n}\n{q}\n" for n, q in zip(names, sq)))
        per[name] = (names, sq)
    return per, raw_n, filt_n


def sam_text(names: Sequence[str], seqs: Sequence[str], loci: dict, ref_names: Sequence[str], ref_lens=None, command: str = "") -> str:
    """the coordinate-sorted SAM of one sample: the records in the order the device hands them out, (reference, offset, query,
    '+' before '-'), then the reads without a reported alignment (XM:i:1: more than -m alignments)"""
    out = ["@HD\tVN:1.0\tSO:coordinate"]
    if ref_lens is not None:
        out += [f"@SQ\tSN:{n}\tLN:{int(ln)}" for n, ln in zip(ref_names, ref_lens)]
    out.append(f"@PG\tID:mirge3.0_amd\tPN:mirge_genome_align_loci\tCL:\"{command}\"")
    rc = {}
    for q, r, o, st, mm in zip(loci["query"].tolist(), loci["ref"].tolist(), loci["off"].tolist(), loci["strand"].tolist(),
                               loci["mm"].tolist()):
        s = seqs[q]
        if st:
            s = rc.get(q) or rc.setdefault(q, revcomp(s))
        out.append(f"{names[q]}\t{16 if st else 0}\t{ref_names[r]}\t{o + 1}\t255\t{len(s)}M\t*\t0\t0\t{s}\t{'I' * len(s)}\tNM:i:{mm}")
    reported = np.zeros(len(names), dtype=bool)
    reported[loci["query"]] = True
    for q in np.nonzero(~reported)[0].tolist():
        s = seqs[q]
        out.append(f"{names[q]}\t4\t*\t0\t0\t*\t*\t0\t0\t{s}\t{'I' * len(s)}\tXM:i:{1 if loci['totals'][q] else 0}")
    return "\n".join(out) + "\n"


def read_sam(path):
    """the aligned lines of a sorted SAM -> names, sequences (as printed), flags, reference names, 0-based offsets"""
    names, seqs, flags, chrs, offs = [], [], [], [], []
    with open(path) as fh:
        for line in fh:
            if line[0] == "@":
                continue
            f = line.rstrip("\n").split("\t")
            if f[1] not in ("0", "16"):
                continue
            names.append(f[0]); flags.append(int(f[1])); chrs.append(f[2]); offs.append(int(f[3]) - 1); seqs.append(f[9])
    return names, seqs, flags, chrs, offs


def cluster_scan(ref, off, strand, length, ref_skip, threshold: int, minus_first_only: bool = True) -> np.ndarray:
    """``mirge_loci_cluster``'s formulation on the host, for the tests: records sorted by (ref, off) -> cluster id per record
    (-1: dropped), ids rising over (ref, strand, start).  Inside one (ref, strand) a record joins iff
    ``off + max(threshold, 1) <= max(off + length)`` over the records before it: a running maximum over the whole segment, which
    decides as the maximum over the current cluster does (a record that opened a cluster lay past every earlier end, and so
    does everything after it)."""
    ref, off, strand, length = (np.asarray(a, dtype=np.int64) for a in (ref, off, strand, length))
    n = ref.shape[0]
    cluster = np.full(n, -1, dtype=np.int64)
    if n == 0:
        return cluster
    order = np.argsort(ref * 2 + strand, kind="stable")
    key = (ref * 2 + strand)[order]
    bounds = np.concatenate(([0], np.nonzero(np.diff(key))[0] + 1, [n]))
    need = max(int(threshold), 1)
    next_id = 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        idx = order[a:b]
        if ref_skip[ref[idx[0]]]:
            continue
        end = off[idx] + length[idx]
        before = np.concatenate(([np.iinfo(np.int64).min], np.maximum.accumulate(end)[:-1]))
        opens = off[idx] + need > before
        ordinal = np.cumsum(opens) - 1
        if strand[idx[0]] == 1 and minus_first_only:
            kept = ordinal == 0
            cluster[idx[kept]] = next_id
            next_id += 1
        else:
            cluster[idx] = next_id + ordinal
            next_id += int(ordinal[-1]) + 1
    return cluster


def clusters_tsv(sample: str, names, seqs, flags, chrs, offs, cluster: np.ndarray, table: dict = None) -> str:
    """``<sample>_clusters.tsv`` (novel_mir.py:133-149) from the records in SAM order and their cluster ids.  A cluster's sequence
    grows by the reference's append rule (:109-114): a member that reaches past the cluster's end adds its bases past that end --
    read bases, not genome text.  ``table`` (the device's): its start / end / reads / members are written; without it they are
    derived from the members."""
    members: Dict[int, List[int]] = {}
    for i, c in enumerate(np.asarray(cluster).tolist()):
        if c >= 0:
            members.setdefault(c, []).append(i)
    out = ["miRClusterID\tChr\tStrand\tStart\tEnd\tSequence\tSequenceLenght\tCoutOfReads\tCountOfMembers\tMembers\n"]
    for c in sorted(members):
        m = members[c]
        first = m[0]
        start, end, seq = offs[first] + 1, offs[first] + len(seqs[first]), seqs[first]
        for i in m[1:]:
            e = offs[i] + len(seqs[i])
            if e > end:
                seq += seqs[i][end - offs[i]:]
                end = e
        reads = sum(int(names[i].split("_")[1]) for i in m)
        n_mem = len(m)
        if table is not None:
            start, end, reads, n_mem = int(table["start"][c]) + 1, int(table["end"][c]), int(table["reads"][c]), int(table["members"][c])
        out.append("\t".join([f"{sample}:miRCluster_{c + 1}_{len(seq)}", chrs[first], "-" if flags[first] == 16 else "+", str(start),
                              str(end), seq, str(len(seq)), str(reads), str(n_mem), ",".join(names[i] for i in m)]) + "\n")
    return "".join(out)


def clusters_from_sam(sam_path, sample: str, threshold: int, out_path, cluster_fn=None) -> int:
    """the host half on its own: a sorted SAM -> ``<sample>_clusters.tsv``.  ``cluster_fn(ref, off, strand, length, ref_skip,
    threshold)`` -> ids; default ``cluster_scan``.  -> number of clusters"""
    names, seqs, flags, chrs, offs = read_sam(sam_path)
    ref_names = list(dict.fromkeys(chrs))
    rid = {n: k for k, n in enumerate(ref_names)}
    ref = np.array([rid[c] for c in chrs], dtype=np.int64)
    skip = np.array(["chr" not in n for n in ref_names], dtype=np.uint8)
    cl = (cluster_fn or cluster_scan)(ref, np.array(offs, dtype=np.int64), np.array([f == 16 for f in flags], dtype=np.int64),
                                      np.array([len(s) for s in seqs], dtype=np.int64), skip, threshold)
    with open(out_path, "w") as fh:
        fh.write(clusters_tsv(sample, names, seqs, flags, chrs, offs, cl))
    return int(cl.max()) + 1 if len(cl) else 0


def settings(args) -> dict:
    """-minl -maxl -c -mloc -sl -olc with the reference's defaults"""
    out = {}
    for k, d in DEFAULTS.items():
        v = getattr(args, "ignored_" + k, None)
        out[k] = int(v) if v is not None else d
    return out


def run(args, ctx, workDir, base_names: Sequence[str], genome, tm: dict = None) -> dict:
    """The whole step after ``unmapped.csv`` exists.  ``genome`` = ``a2i.GpuGenome`` (the genome -ai loaded, when both run)."""
    from . import _ffi
    t0 = time.perf_counter()
    workDir = Path(workDir)
    out_dir = workDir / "unmapped_tmp"
    os.makedirs(out_dir, exist_ok=True)
    p = settings(args)
    seqs, counts = read_unmapped_csv(workDir / "unmapped.csv", base_names)
    per, raw_n, filt_n = convert2fasta(seqs, counts, base_names, p["minl"], p["maxl"], p["c"], out_dir)
    ref_names = getattr(genome.genome, "ref_names", None)
    if ref_names is None:
        raise RuntimeError("--unmapped-clusters: the genome carries no reference names (load it with a2i.load_genome)")
    skip = np.array(["chr" not in n for n in ref_names], dtype=np.uint8)
    log, result = [], {}
    for sample in base_names:
        names, sq = per[sample]
        t = time.perf_counter()
        loci = genome.loci(sq, n_mm=0, seedlen=p["sl"], maxtotal=MAXTOTAL, max_loci=p["mloc"])
        t_loci = time.perf_counter() - t
        with open(out_dir / f"unmapped_mirna_{sample}_vs_genome_sorted.sam", "w") as fh:
            fh.write(sam_text(names, sq, loci, ref_names, getattr(genome.genome, "ref_lens", None),
                              f"-f -n 0 --best -a -m {p['mloc']} -l {p['sl']} -S"))
        t = time.perf_counter()
        qlen = np.array([len(s) for s in sq], dtype=np.int32)
        qcount = np.array([int(n.split("_")[1]) for n in names], dtype=np.int64)
        tab = _ffi.loci_cluster(ctx, loci["ref"], loci["off"], loci["strand"], loci["query"], qlen, qcount, skip, p["olc"], True)
        q, st = loci["query"].tolist(), loci["strand"].tolist()
        rseq = [revcomp(sq[a]) if b else sq[a] for a, b in zip(q, st)]
        text = clusters_tsv(sample, [names[a] for a in q], rseq, [16 if b else 0 for b in st], [ref_names[r] for r in loci["ref"].tolist()],
                            loci["off"].astype(np.int64).tolist(), tab["cluster"], tab)
        with open(out_dir / f"{sample}_clusters.tsv", "w") as fh:
            fh.write(text)
        t_cl = time.perf_counter() - t
        n_cap = int((loci["totals"] > p["mloc"]).sum()) if p["mloc"] else 0
        result[sample] = dict(reads=len(sq), alignments=int(loci["query"].shape[0]), capped=n_cap, clusters=int(tab["ref"].shape[0]))
        log.append(f"unmapped clusters, {sample}: {raw_n[sample]} collapsed reads, {filt_n[sample]} after filtering, "
                   f"{result[sample]['alignments']} alignments ({n_cap} reads over -m {p['mloc']}), {result[sample]['clusters']} clusters; "
                   f"loci {t_loci:.3f} s, clustering {t_cl:.3f} s\n")
    seconds = time.perf_counter() - t0
    with open(workDir / "run.log", "a+") as fh:
        fh.write("".join(log) + f"unmapped clusters: {seconds:.3f} s\n")
    if tm is not None:
        tm["unmapped_loci_s"] = seconds
    return result

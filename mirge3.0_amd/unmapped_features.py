"""``--unmapped-features``: which clusters of unmapped reads look like miRNAs -- ``generate_featureFiles`` and ``get_precursors``
(mirge/libs/generate_featureFiles.py, mirge/classes/readCluster.py; novel_mir.py:424-428), the last stretch of the reference's
``-nmir`` that is sequence work:

    <sample>_modified_selected_sorted.tsv --locateStartPosition / calculateFeature--> <sample>_cluster.txt, <sample>_features.tsv
    <sample>_features.tsv --get_precursors--> <sample>_precursor.fa                  (the input of RNAfold, which is out of scope)

The reference aligns every (cluster, read) row with ``pairwise2.align.localms(cluster, read, 2, -1, -20, -20)``, twice, and stacks
the padded strings.  Here the device reports each row's best ungapped diagonal (``mirge_cluster_diagonals``), the clusters'
paddings and count-weighted column tallies (``mirge_cluster_pileup``) and the genome windows (``mirge_genome_fetch``); the text
around those integers and bytes is made here, every ratio as a Python float division printed with ``str()``.  A row whose
ungapped score does not rule a gap out (``best <= 2 * min(L, C) - 20``) sends its cluster through ``string_pile``: the
reference's own string route over ``localms``, a Smith-Waterman twin of the stand-in tests/golden/stubs/Bio/pairwise2.py.
"""
import time
from pathlib import Path
from typing import Callable, Dict, List, Sequence, Tuple

import numpy as np

THRESHOLD, HEAD_SHIFT, TAIL_SHIFT = 0.8, 3, 6  # readCluster.py:20-22
READ_COUNT_LIMIT, SEQ_COUNT_LIMIT, STABLE_LEN_LIMIT = 10, 3, 16 - 6 - 3  # generate_featureFiles.py:60-62
CLOSEST, FARTHEST, TERMINAL = 9, 44, 20  # :63-66
MATCH, MISMATCH, GAP = 2, -1, -20
HEADER = ("realMicRNA\trealMicRNAName\tchr\tstartPos\tendPos\tclusterName\tclusterSeq\tmajoritySeq\tstableClusterSeq\talignedClusterSeq\t"
          "adjustedClusterSeq\tclusterSecondSeq\ttemplateSeq\tseqCount\treadCountSum\texactMatchRatio\theadUnstableLength\t"
          "tailUnstableLength\t")
_NUC = ("templateNucleotide", "TemplateNucleotide_percentage", "nonTemplateNucleotide_percentage", "A_percentage", "T_percentage",
        "C_percentage", "G_percentage")
POSITION_LABELS = [("head_minus%d_" % (HEAD_SHIFT - i) if i <= HEAD_SHIFT - 1 else "tail_plus%d_" % (i + 1 - HEAD_SHIFT)) + n
                   for i in range(HEAD_SHIFT + TAIL_SHIFT) for n in _NUC]


# ------------------------------------------------------------------------------------------------ the Smith-Waterman twin
def localms_first(a: str, b: str):
    """``pairwise2.align.localms(a, b, 2, -1, -20, -20)[0][:2]`` as the stand-in makes it: the best-scoring local alignment
    whose end cell comes first in ``a``, then in ``b``, traced back diagonal before gap, both FULL sequences written along it
    and padded with '-' to one length.  -> (padded a, padded b, score), None when nothing scores (the reference's IndexError)"""
    n, m = len(a), len(b)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    best, end = 0, None
    for i in range(1, n + 1):
        ai, Hi, Hp = a[i - 1], H[i], H[i - 1]
        for j in range(1, m + 1):
            v = max(0, Hp[j - 1] + (MATCH if ai == b[j - 1] else MISMATCH), Hp[j] + GAP, Hi[j - 1] + GAP)
            Hi[j] = v
            if v > best:  # row-major and strict: the first cell that reaches the best
                best, end = v, (i, j)
    if end is None:
        return None
    i, j = end
    ra, rb = [], []
    while i > 0 and j > 0 and H[i][j] > 0:
        if H[i][j] == H[i - 1][j - 1] + (MATCH if a[i - 1] == b[j - 1] else MISMATCH):
            ra.append(a[i - 1]); rb.append(b[j - 1]); i -= 1; j -= 1
        elif H[i][j] == H[i - 1][j] + GAP:
            ra.append(a[i - 1]); rb.append("-"); i -= 1
        else:
            ra.append("-"); rb.append(b[j - 1]); j -= 1
    ha, hb, ta, tb = a[:i], b[:j], a[end[0]:], b[end[1]:]
    hl, tl = max(len(ha), len(hb)), max(len(ta), len(tb))
    return ("-" * (hl - len(ha)) + ha + "".join(reversed(ra)) + ta + "-" * (tl - len(ta)),
            "-" * (hl - len(hb)) + hb + "".join(reversed(rb)) + tb + "-" * (tl - len(tb)), best)


def calculate_identity(sa: str, sb: str) -> int:
    return sum(1 for i in range(len(sa)) if sa[i] == sb[i] and sa[i] != "-" and sb[i] != "-")


# ------------------------------------------------------------------------------------------------ a cluster's pile-up
class Pile:
    """``rows``: the reference's alignSeqList (the padded cluster, then every read's padded row), ``exact``: the summed counts of
    the reads that lie in the cluster without a mismatch, ``tally``: per column the summed counts of A, T, C, G"""
    __slots__ = ("rows", "exact", "tally")

    def __init__(self, rows, exact, tally):
        self.rows, self.exact, self.tally = rows, exact, tally


def string_pile(cluster_seq: str, read_seqs: Sequence[str], counts: Sequence[int]) -> Pile:
    """``align2Standard`` and the tallies of ``locateStartPosition`` as the reference makes them, from strings (the host route)"""
    rows, exact = [], 0
    for i, seq in enumerate(read_seqs):
        al = localms_first(cluster_seq, seq)
        if al is None:
            raise ValueError(f"read {seq} has no local alignment with its cluster {cluster_seq} (the reference stops here too)")
        new, row = al[0], al[1]
        if calculate_identity(new, row) == len(seq):
            exact += counts[i]
        if not rows:
            rows += [new, row]
        elif new == rows[0]:
            rows.append(row)
        else:
            h1 = new.index(cluster_seq)
            t1 = len(new) - h1 - len(cluster_seq)
            h2 = rows[0].index(cluster_seq)
            t2 = len(rows[0]) - h2 - len(cluster_seq)
            if h1 >= h2 and t1 >= t2:
                rows = [(h1 - h2) * "-" + r + (t1 - t2) * "-" for r in rows] + [row]
            elif h1 >= h2:
                rows = [(h1 - h2) * "-" + r for r in rows] + [row + (t2 - t1) * "-"]
            elif t1 >= t2:
                rows = [r + (t1 - t2) * "-" for r in rows] + [(h2 - h1) * "-" + row]
            else:
                rows.append((h2 - h1) * "-" + row + (t2 - t1) * "-")
    tally = []
    for i in range(len(rows[0])):
        n = dict(A=0, T=0, C=0, G=0)
        for j in range(1, len(rows)):
            if rows[j][i] in n:
                n[rows[j][i]] += counts[j - 1]
        tally.append((n["A"], n["T"], n["C"], n["G"]))
    return Pile(rows, exact, tally)


def diagonal_pile(cluster_seq: str, read_seqs: Sequence[str], counts: Sequence[int], diag, identity, head: int, tail: int, tally) -> Pile:
    """the same from the device's integers: every row lies on its diagonal, the cluster starts at column ``head``"""
    width = head + len(cluster_seq) + tail
    rows = ["-" * head + cluster_seq + "-" * tail]
    exact = 0
    for s, n, d, same in zip(read_seqs, counts, diag, identity):
        rows.append("-" * (head + d) + s + "-" * (width - head - d - len(s)))
        if same == len(s):
            exact += n
    return Pile(rows, exact, [tuple(t[:4]) for t in tally])


def device_eligible(cluster_seq: str, read_seqs: Sequence[str]) -> bool:
    """what the kernels take: a cluster of A/C/G/T up to 128 nt, reads of 1 to 64 nt (plain ASCII).  Anything else is the host's"""
    from ._ffi import PILEUP_MAXCLUSTER, PILEUP_MAXREAD
    return (0 < len(cluster_seq) <= PILEUP_MAXCLUSTER and not cluster_seq.strip("ACGT") and cluster_seq.isascii()
            and all(0 < len(s) <= PILEUP_MAXREAD and s.isascii() for s in read_seqs))


def device_arrays(ctx, clusters: Sequence[Tuple[str, Sequence[str], Sequence[int]]], tm: dict = None) -> dict:
    """the two pile-up calls over ``clusters`` = [(cluster sequence, read sequences, counts)], all of them ``device_eligible``"""
    from . import _ffi
    from .seqio import FlatSeqs
    tm = tm if tm is not None else {}
    n_rows = [len(c[1]) for c in clusters]
    row_start = np.zeros(len(clusters) + 1, dtype=np.int64)
    np.cumsum(n_rows, out=row_start[1:])
    reads = FlatSeqs.from_list([s for c in clusters for s in c[1]])
    count = np.array([n for c in clusters for n in c[2]], dtype=np.int64)
    t = time.perf_counter()
    out = _ffi.cluster_diagonals(ctx, reads, FlatSeqs.from_list([c[0] for c in clusters]), np.repeat(np.arange(len(clusters)), n_rows))
    tm["diagonals_s"] = tm.get("diagonals_s", 0.0) + time.perf_counter() - t
    t = time.perf_counter()
    out.update(_ffi.cluster_pileup(ctx, reads, [len(c[0]) for c in clusters], row_start, out["diag"], count))
    tm["pileup_s"] = tm.get("pileup_s", 0.0) + time.perf_counter() - t
    out["row_start"] = row_start
    return out


def piles_from_arrays(clusters, arrays: dict) -> Tuple[List[Pile], int, int]:
    """-> the clusters' piles, the number of rows the device flagged and the rows of the clusters that therefore took the string
    route (a cluster with a flagged row takes it whole)"""
    piles, flagged, fallback = [], 0, 0
    rs, co = arrays["row_start"].tolist(), arrays["col_off"].tolist()
    for k, (cseq, rseqs, counts) in enumerate(clusters):
        a, b = rs[k], rs[k + 1]
        bad = int(np.count_nonzero(arrays["flag"][a:b]))
        flagged += bad
        if bad:
            fallback += b - a
            piles.append(string_pile(cseq, rseqs, counts))
        else:
            piles.append(diagonal_pile(cseq, rseqs, counts, arrays["diag"][a:b].tolist(), arrays["identity"][a:b].tolist(),
                                       int(arrays["head"][k]), int(arrays["tail"][k]), arrays["tally"][co[k]:co[k + 1]].tolist()))
    return piles, flagged, fallback


# ------------------------------------------------------------------------------------------------ the reference's text
def read_clusters(path):
    """the grouping of generate_featureFiles.py:77-102: a row joins the LAST entry of its chromosome when the names agree, else
    opens one; chromosomes sorted as strings, a chromosome's entries as the lists [start, end, name, sequence, names, reads,
    counts] -> (chromosomes, {chromosome: entries})"""
    content: Dict[str, list] = {}
    with open(path) as fh:
        for line in fh:
            f = line.strip().split("\t")
            name, count, seq, cseq, cname = f[0], int(f[1]), f[2], f[3], f[5]
            chrom = cname.split(":")[2].strip()
            span = cname.split(":")[-1][:-1].split("_")
            start, end = int(span[0].strip()), int(span[1].strip())
            if chrom not in content:
                content[chrom] = [[start, end, cname, cseq, [name], [seq], [count]]]
            elif cname == content[chrom][-1][2]:
                e = content[chrom][-1]
                e[4].append(name); e[5].append(seq); e[6].append(count)
            else:
                content[chrom].append([start, end, cname, cseq, [name], [seq], [count]])
    chroms = sorted(content)
    for c in chroms:
        content[c].sort()
    return chroms, content


def enough_reads(entry) -> bool:
    """:118: the counts sum to at least 10 over at least 3 distinct reads"""
    return sum(entry[6]) >= READ_COUNT_LIMIT and len(entry[5]) >= SEQ_COUNT_LIMIT


def inside_margins(entry, chrom_len: int) -> bool:
    """:119: not within 20 nt of either end of the chromosome (asked only of a cluster with enough reads: the reference looks the
    chromosome's length up only then)"""
    return entry[0] > TERMINAL and entry[1] < chrom_len - TERMINAL


def locate(pile: Pile, counts: Sequence[int]):
    """``locateStartPosition`` after the alignment: per column the cluster base's and the majority base's share of all counts
    (the majority by ``sort(reverse=True)`` on [count, letter]: T > G > C > A on equal counts), and the first / last column
    whose majority share reaches 0.8 (the last as a negative index) -> (cluster ratios, majority sequence, majority ratios,
    head, tail).  The threshold is the reference's float comparison on the same quotient."""
    total = sum(counts)
    c_ratio, m_ratio, major = [], [], ""
    for ch, (a, t, c, g) in zip(pile.rows[0], pile.tally):
        own = {"A": a, "T": t, "C": c, "G": g}
        c_ratio.append(float(own[ch]) / total if ch in own else 0)  # the reference's integer 0 prints as '0'
        top = sorted([[a, "A"], [t, "T"], [c, "C"], [g, "G"]], reverse=True)[0]
        m_ratio.append(float(top[0]) / total)
        major += top[1]
    head = next((i for i in range(len(m_ratio)) if m_ratio[i] >= THRESHOLD), None)
    tail = next((i for i in range(-1, -len(m_ratio) - 1, -1) if m_ratio[i] >= THRESHOLD), None)
    return c_ratio, major, m_ratio, head, tail


def head_dashes(s: str) -> int:
    return len(s) - len(s.lstrip("-"))


def tail_dashes(s: str) -> int:
    return len(s) - len(s.rstrip("-"))


def adjust(pile: Pile, head: int, tail: int) -> dict:
    """readCluster.py:164-203: the pile padded to 3 columns in front of the stable head and 6 behind the stable tail, and the
    genome window of its template as a Python slice (a, b) of the chromosome"""
    head_add, tail_add = head, -tail - 1
    ph = HEAD_SHIFT - head_add if head_add < HEAD_SHIFT else 0
    pt = TAIL_SHIFT - tail_add if tail_add < TAIL_SHIFT else 0
    adjusted = "-" * ph + pile.rows[0] + "-" * pt
    return dict(head_unstable=head_add, tail_unstable=tail_add, pad_head=ph, head=HEAD_SHIFT if ph else head, tail=-TAIL_SHIFT if pt else tail,
                adjusted=adjusted, second="-" * ph + pile.rows[1] + "-" * pt, head_dash=head_dashes(adjusted), tail_dash=tail_dashes(adjusted))


def template_window(adj: dict, strand: str, start: int, end: int) -> Tuple[int, int]:
    if strand == "+":
        return start - adj["head_dash"] - 1, end + adj["tail_dash"]
    return start - adj["tail_dash"] - 1, end + adj["head_dash"]


def slice_bounds(a, b, length: int) -> Tuple[int, int]:
    """chromosome[a:b] as (0-based start, length), Python's slice semantics: ``None`` / past-the-end clamp, a negative bound
    counts from the end (what the reference gets for a window that would start before base 1)"""
    lo, hi, _ = slice(a, b).indices(length)
    return lo, max(0, hi - lo)


def nucleotide_profile(pile: Pile, adj: dict, template: str, name: str) -> list:
    """readCluster.py:208-320: the nine columns (3 in front of the stable head, 6 from the stable tail on) against the template.
    A template base that is not A/C/G/T over a column with reads leaves the four letter shares as the column before set them
    (the reference's ``else: pass``)"""
    width = len(adj["adjusted"])
    cols = list(range(adj["head"] - HEAD_SHIFT, adj["head"])) + list(range(adj["tail"], adj["tail"] + TAIL_SHIFT))
    out = []
    unset = object()
    pa = pt = pc = pg = unset
    for col in cols:
        try:
            nt = template[col]
        except IndexError:
            raise RuntimeError(f"{name}: its template window leaves the chromosome (template {template!r}, column {col}); the "
                               "reference exits here as well") from None
        k = (col if col >= 0 else col + width) - adj["pad_head"]
        a, t, c, g = pile.tally[k] if 0 <= k < len(pile.tally) else (0, 0, 0, 0)
        own = {"A": a, "T": t, "C": c, "G": g}
        n_t, n_non = (own[nt], a + t + c + g - own[nt]) if nt in own else (0, 0)
        if a + t + c + g != 0:
            p_t, p_non = float(n_t) / (a + t + c + g), float(n_non) / (a + t + c + g)
            if nt in own:
                pa, pt, pc, pg = [(float(v) / n_non if n_non != 0 else 0) if x != nt else 0 for x, v in own.items()]
        else:
            p_t = p_non = pa = pt = pc = pg = 0
        if pa is unset:
            raise RuntimeError(f"{name}: template base {nt!r} in the first profile column (the reference fails here as well)")
        out += [nt, p_t, p_non, pa, pt, pc, pg]
    return out


def stable_span(start: int, end: int, padded_cluster: str, head: int, tail: int) -> Tuple[int, int]:
    return start + head - head_dashes(padded_cluster), end + 1 + tail + tail_dashes(padded_cluster)


def neighbour_state(detailed: list, t: int):
    """generate_featureFiles.py:144-212: from the stable regions' distance d = s2 - e1 - 1 to the clusters before and behind on
    the chromosome: Good (9..44 on the same strand), Null (past 44; a lone cluster), else Bad"""
    if len(detailed) < 2:
        return "Null", None, None
    me = detailed[t]

    def gap(first, second):
        return second["span"][0] - first["span"][1] - 1

    def good(d, other):
        return CLOSEST <= d <= FARTHEST and other["strand"] == me["strand"]
    up = gap(detailed[t - 1], me) if t > 0 else None
    down = gap(me, detailed[t + 1]) if t < len(detailed) - 1 else None
    sides = [(d, o) for d, o in ((up, detailed[t - 1]), (down, detailed[(t + 1) % len(detailed)])) if d is not None]
    if any(good(d, o) for d, o in sides):
        state = "Good"
    elif all(d > FARTHEST for d, _ in sides):
        state = "Null"
    else:
        state = "Bad"
    return state, up, down


def remove_dashes(s: str) -> str:
    return s.replace("-", "")


def cluster_text(d: dict, t: int) -> str:
    """one entry of ``<sample>_cluster.txt``"""
    e, pile = d["entry"], d["pile"]
    out = [f"Cluster Name: {e[2]}\n", "%s (%d - %d%s) cluster %d:\n" % (d["chrom"], e[0], e[1], e[2][-1], t),
           f"{pile.rows[0]}: " + "\t".join(map(str, d["c_ratio"])) + "\n", f"{d['major']}: " + "\t".join(map(str, d["m_ratio"])) + "\n",
           pile.rows[0] + "\n"]
    out += ["%s\t%d\n" % (row, n) for row, n in zip(pile.rows[1:], e[6])]
    return "".join(out)


def feature_row(d: dict, adj: dict, template: str, profile: list, state, up, down) -> str:
    e, pile, head, tail = d["entry"], d["pile"], d["head"], d["tail"]
    counts = e[6]
    majority = remove_dashes(sorted([[counts[i], pile.rows[i + 1]] for i in range(len(pile.rows) - 1)], reverse=True)[0][1])
    stable = remove_dashes(pile.rows[0][head:] if tail == -1 else pile.rows[0][head:tail + 1])
    total = sum(counts)
    f = ["Null", "Null", d["chrom"], str(e[0]), str(e[1]), e[2], e[3], majority, stable, pile.rows[0], adj["adjusted"], adj["second"], template,
         str(len(e[5])), str(total), str(float(pile.exact) / total), str(adj["head_unstable"]), str(adj["tail_unstable"])]
    return "\t".join(f) + "\t" + "".join(str(v) + "\t" for v in profile) + state + "\t" + str(up) + "\t" + str(down) + "\n"


def precursor_windows(features_path) -> list:
    """``get_precursors``: per cluster name (once) of ``<sample>_features.tsv`` the two windows around its stable region, 70 nt
    upstream / 20 downstream and 20 / 70, as Python slices of the chromosome -> [(header, chromosome, a, b, strand)]"""
    out, seen = [], []
    with open(features_path) as fh:
        head = fh.readline().strip().split("\t")
        k_head, k_tail, k_aligned = head.index("headUnstableLength"), head.index("tailUnstableLength"), head.index("alignedClusterSeq")
        for line in fh:
            f = line.strip().split("\t")
            name = f[5]
            if name in seen:
                continue
            seen.append(name)
            hd, td = head_dashes(f[k_aligned]), tail_dashes(f[k_aligned])
            span = name.split(":")[3][:-1].split("_")
            start, end, strand = int(span[0].strip()), int(span[1].strip()), name[-1]
            if strand == "+":
                start, end = start - hd + int(f[k_head]), end + td - int(f[k_tail])
            else:
                start, end = start - td + int(f[k_tail]), end + hd - int(f[k_head])
            for k, (up, down) in enumerate(((70, 20), (20, 70))):
                out.append((f"{name}:precusor_{k + 1}", name.split(":")[2], start - 1 - up if start - 1 - up >= 0 else None, end + down, strand))
    return out


def write_features(sample: str, out_dir, chrom_lens: Dict[str, int], pile_fn: Callable, fetch: Callable) -> dict:
    """The host text of the step.  ``pile_fn([(cluster sequence, reads, counts)]) -> ([Pile], flagged rows, fallback rows)``;
    ``fetch([(chromosome, 0-based start, length, minus, rna)]) -> [text]``.  -> counts for the log"""
    out_dir = Path(out_dir)
    chroms, content = read_clusters(out_dir / f"{sample}_modified_selected_sorted.tsv")
    picked = []
    for chrom in chroms:
        for e in content[chrom]:
            if enough_reads(e):
                if chrom not in chrom_lens:
                    raise RuntimeError(f"{e[2]}: chromosome {chrom} is not in the genome")
                if inside_margins(e, chrom_lens[chrom]):
                    picked.append((chrom, e))
    t0 = time.perf_counter()
    piles, flagged, fallback = pile_fn([(e[3], e[5], e[6]) for _, e in picked])
    t_pile = time.perf_counter() - t0
    t0 = time.perf_counter()
    detailed: Dict[str, list] = {c: [] for c in chroms}
    for (chrom, e), pile in zip(picked, piles):
        c_ratio, major, m_ratio, head, tail = locate(pile, e[6])
        if head is None or tail is None:
            continue
        detailed[chrom].append(dict(chrom=chrom, entry=e, pile=pile, c_ratio=c_ratio, major=major, m_ratio=m_ratio, head=head, tail=tail,
                                    strand=e[2][-1], span=stable_span(e[0], e[1], pile.rows[0], head, tail)))
    every = [d for c in chroms for d in detailed[c]]
    for d in every:
        d["adj"] = adjust(d["pile"], d["head"], d["tail"])
        a, b = template_window(d["adj"], d["strand"], d["entry"][0], d["entry"][1])
        d["window"] = slice_bounds(a, b, chrom_lens[d["chrom"]])
    t_text = time.perf_counter() - t0
    t0 = time.perf_counter()
    templates = fetch([(d["chrom"],) + d["window"] + (d["strand"] == "-", False) for d in every])
    t_fetch = time.perf_counter() - t0
    t0 = time.perf_counter()
    rows = 0
    cluster_txt, feat = [], [HEADER]
    for chrom in chroms:
        for t, d in enumerate(detailed[chrom]):
            state, up, down = neighbour_state(detailed[chrom], t)
            cluster_txt.append(cluster_text(d, t))
            template = templates[len(cluster_txt) - 1]
            profile = nucleotide_profile(d["pile"], d["adj"], template, d["entry"][2])
            if len(cluster_txt) == 1:
                feat.append("\t".join(POSITION_LABELS) + "\tneighborState\tupstreamDistance\tdownstreamDistance\n")
            if len(d["adj"]["adjusted"]) - d["adj"]["head_unstable"] - d["adj"]["tail_unstable"] >= STABLE_LEN_LIMIT:
                feat.append(feature_row(d, d["adj"], template, profile, state, up, down))
                rows += 1
    with open(out_dir / f"{sample}_cluster.txt", "w") as fh:
        fh.write("".join(cluster_txt))
    with open(out_dir / f"{sample}_features.tsv", "w") as fh:
        fh.write("".join(feat))
    wins = precursor_windows(out_dir / f"{sample}_features.tsv")
    t_text += time.perf_counter() - t0
    t0 = time.perf_counter()
    for w in wins:
        if w[1] not in chrom_lens:
            raise RuntimeError(f"{w[0]}: chromosome {w[1]} is not in the genome")
    seqs = fetch([(w[1],) + slice_bounds(w[2], w[3], chrom_lens[w[1]]) + (w[4] == "-", True) for w in wins])
    t_fetch += time.perf_counter() - t0
    with open(out_dir / f"{sample}_precursor.fa", "w") as fh:
        fh.write("".join(f">{w[0]}\n{s}\n" for w, s in zip(wins, seqs)))
    return dict(clusters=sum(len(content[c]) for c in chroms), passed=len(picked), detailed=len(every), rows=rows, precursors=len(wins),
                flagged=flagged, fallback=fallback, pile_s=t_pile, fetch_s=t_fetch, text_s=t_text)


def features_sample(ctx, sample: str, out_dir, genome, log: list = None, arrays_fn: Callable = None) -> dict:
    """one sample from the files ``--unmapped-align`` left in ``out_dir``; ``genome`` = the resident ``_ffi.DeviceGenome`` with
    its ``ref_names`` / ``ref_lens``.  ``arrays_fn(ctx, clusters, tm)`` stands in for ``device_arrays`` (tests, timing)."""
    ref_id = {n: k for k, n in enumerate(genome.ref_names)}
    chrom_lens = {n: int(ln) for n, ln in zip(genome.ref_names, genome.ref_lens)}
    tm: dict = {}

    def pile_fn(clusters):
        on_dev = [device_eligible(c[0], c[1]) for c in clusters]
        sub = [c for c, ok in zip(clusters, on_dev) if ok]
        piles, flagged, fallback = piles_from_arrays(sub, (arrays_fn or device_arrays)(ctx, sub, tm)) if sub else ([], 0, 0)
        it = iter(piles)
        out = [next(it) if ok else string_pile(*c) for c, ok in zip(clusters, on_dev)]
        return out, flagged, fallback + sum(len(c[1]) for c, ok in zip(clusters, on_dev) if not ok)

    def fetch(windows):
        if not windows:
            return []
        return genome.fetch([ref_id[w[0]] for w in windows], [w[1] for w in windows], [w[2] for w in windows], [w[3] for w in windows],
                            [w[4] for w in windows])
    res = write_features(sample, out_dir, chrom_lens, pile_fn, fetch)
    res.update(diagonals_s=tm.get("diagonals_s", 0.0), pileup_s=tm.get("pileup_s", 0.0))
    if log is not None:
        log.append(f"unmapped features, {sample}: {res['clusters']} clusters read, {res['passed']} passed the count / terminal filter, "
                   f"{res['detailed']} with a stable head and tail, {res['rows']} rows written, {res['precursors']} precursors; "
                   f"{res['flagged']} rows flagged, {res['fallback']} rows aligned on the host; diagonals {res['diagonals_s']:.3f} s, "
                   f"pile-up {res['pileup_s']:.3f} s, genome windows {res['fetch_s']:.3f} s, text {res['text_s']:.3f} s\n")
    return res


def run(args, ctx, workDir, base_names: Sequence[str], tm: dict = None) -> dict:
    """The whole step after ``unmapped_align.run``: every sample that reached ``<sample>_modified_selected_sorted.tsv``."""
    from .a2i import genome_base, load_genome
    t0 = time.perf_counter()
    workDir = Path(workDir)
    out_dir = workDir / "unmapped_tmp"
    genome = load_genome(ctx, str(genome_base(args)))  # the genome --unmapped-clusters aligned to: resident, not loaded again
    log, result = [], {}
    for sample in base_names:
        if (out_dir / f"{sample}_modified_selected_sorted.tsv").exists():  # else: no cluster was kept, prediction was aborted
            result[sample] = features_sample(ctx, sample, out_dir, genome, log)
    seconds = time.perf_counter() - t0
    with open(workDir / "run.log", "a+") as fh:
        fh.write("".join(log) + f"unmapped features: {seconds:.3f} s\n")
    if tm is not None:
        tm["unmapped_features_s"] = seconds
    return result

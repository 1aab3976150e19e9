"""``--trf-clusters`` on the host (mirge3_amd/trf.py): the text of ``<sample>.aligned_tRFs.clusters.detail`` and
``<sample>.tRFs.report.tsv`` against the files the reference wrote (tests/golden/case9_trf_clusters, made by
tests/golden/make_golden_trf_clusters.py), byte for byte.  The clustering arrays that the device delivers in a real run come here from
``restate``: getDistance / local_density / min_distance and the centre / halo loop restated in NumPy from mirge2_tRF_a2i.py:122-207,
776-839 with a stable argsort.  The device's arrays are held against the same restatement in tests/test_trf_clusters_hostsim.py (CPU)
and tests/test_trf_clusters_gpu.py, which share the helpers below."""
import gzip
import math
import os
import re
from collections import Counter

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import trf
from mirge3_amd.cli import parse_args
from mirge3_amd.seqio import load_library_dir

from test_trf_hostsim import MATURE_PASS, PRIMARY_PASS, TYPES, Text, classify, trf_type
from test_trf import restated_assign

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "case9_trf_clusters")
ORG, DB = "synthorg", "miRBase"
SAMPLES = ["S1", "S2", "S3", "S4", "S5"]
SAMPLE_FILES = ["S1.fastq.gz", "S2.fastq.gz", "S3.fastq", "S4.fastq.gz", "S5.fastq.gz"]
TOP = ["tRFs.aligned.report.tsv", "tRF.Counts.csv", "tRF.RP100K.csv", "discarded.reads.summary.assigningtRFs.csv"]
OLD = [os.path.join("tRFs.samples.tmp", s + suffix) for s in SAMPLES for suffix in (".aligned_tRFs.report", ".aligned_tRFs.summary.report")]
NEW = [os.path.join("tRFs.samples.tmp", s + suffix) for s in SAMPLES for suffix in (".aligned_tRFs.clusters.detail", ".tRFs.report.tsv")]


# ---- the reference's clustering, restated
def restate(dashed, rp):
    """one group: ``dashed`` strings of one length, ``rp`` their RP100K -> the arrays of ``mirge_trf_cluster`` for the group (1-based
    indices; ``order`` = the 0-based position in sort_rho_idx; ``centre`` padded with 0 to the group's size)"""
    n = len(dashed)
    A = np.frombuffer("".join(dashed).encode(), dtype=np.uint8).reshape(n, -1)
    letter = A != ord("-")
    start = letter.argmax(axis=1) + 1                        # coordinate()
    end = A.shape[1] - letter[:, ::-1].argmax(axis=1)
    D = np.zeros((n + 1, n + 1))                             # getDistance: 1-based, floats
    for i in range(n):
        D[i + 1, 1:] = np.abs(start[i] - start) + np.abs(end[i] - end) + ((A[i] != A) & letter[i] & letter).sum(axis=1)
    max_dis = float(D.max()) if n > 1 else 0.0
    rpf = np.asarray(rp, dtype=np.float64)
    G = np.asarray([math.exp(-(d / 3.0) ** 2) for d in range(int(D.max()) + 1)])
    rho = [-1.0] + [0.0] * n                                  # local_density: rho[k]'s terms arrive in ascending j, then + RPM
    for k in range(1, n + 1):
        terms = np.delete(G[D[k, 1:].astype(np.int64)] * rpf, k - 1)
        acc = float(np.cumsum(terms)[-1]) if terms.size else 0   # (cumsum adds one after the other, as the loop does)
        rho[k] = acc + float(rpf[k - 1])
    rho = np.array(rho, np.float32)
    idx = np.argsort(-rho, kind="stable")                    # min_distance; rule 4: equal densities in index order
    delta, nneigh = [0.0] + [max_dis] * n, [0] * (n + 1)
    delta[idx[0]] = -1.0
    for i in range(1, n):
        oi, ahead = idx[i], idx[:i]
        ds = D[oi, ahead]
        last = np.nonzero(ds == ds.min())[0][-1]              # `<=`: of equal distances the last one wins
        delta[oi], nneigh[oi] = float(ds[last]), int(ahead[last])
    delta[idx[0]] = max(delta)
    delta = np.array(delta, np.float32)
    nclust, cl, ccenter = 0, np.zeros(n + 1) - 1, {}
    for i in range(1, n + 1):
        if rho[i] >= 5.0 and delta[i] >= 8.0:
            nclust += 1
            cl[i] = nclust
            ccenter[nclust] = i
    if nclust == 0:
        if max([-1.0] + delta[1:].tolist()) <= 8.0 and max([-1.0] + rho[1:].tolist()) >= 5.0:
            nclust = 1
            i = ([-1.0] + rho[1:].tolist()).index(max([-1.0] + rho[1:].tolist()))
            cl[i] = 1
            ccenter[1] = i
    for i in range(n):
        if cl[idx[i]] == -1:
            cl[idx[i]] = cl[nneigh[idx[i]]]
    cl = cl.astype(np.int32)
    halo = np.zeros(n + 1)
    halo[:] = cl
    if nclust > 1:
        bord = np.zeros(nclust + 1)
        for i in range(1, n):
            for j in range(i + 1, n + 1):
                if cl[i] != cl[j] and D[i, j] <= 3.0:
                    aver = (rho[i] + rho[j]) / 2
                    bord[cl[i]] = max(bord[cl[i]], aver)
                    bord[cl[j]] = max(bord[cl[j]], aver)
        for i in range(1, n + 1):
            if rho[i] < bord[cl[i]]:
                halo[i] = 0
            if cl[i] in ccenter and D[i, ccenter[cl[i]]] > 8.0:
                halo[i] = 0
    elif nclust == 1:
        for i in range(1, n + 1):
            if cl[i] in ccenter and D[i, ccenter[cl[i]]] > 8.0:
                halo[i] = 0
    else:
        halo[:] = 0
    order = np.zeros(n + 1, np.int32)
    order[idx[:n]] = np.arange(n)
    centre = np.zeros(n, np.int32)
    centre[:nclust] = [ccenter[k] for k in range(1, nclust + 1)]
    return dict(rho=rho[1:], delta=delta[1:], nneigh=np.asarray(nneigh[1:], np.int32), order=order[1:], cl=cl[1:], halo=halo[1:].astype(np.int32),
                centre=centre, nclust=np.asarray([nclust], np.int32))


def restated_cluster(groups):
    """``cluster(groups)`` of ``trf.write_clusters`` from the restatement"""
    parts = [restate(g["dashed"], g["rp"]) for g in groups]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


# ---- case 9 by brute force (as tests/test_trf.py does for case 8)
def golden_samples():
    per = []
    for f in SAMPLE_FILES:
        with (gzip.open if f.endswith(".gz") else open)(os.path.join(GOLDEN, f), "rt") as fh:
            per.append(Counter(ln.strip() for k, ln in enumerate(fh) if k % 4 == 1))
    reads = sorted(set().union(*per))
    return reads, np.asarray([[c[r] for c in per] for r in reads], dtype=np.int64)


@pytest.fixture(scope="module")
def inputs():
    libs = load_library_dir(os.path.join(GOLDEN, "libs"), ORG, DB)
    mature, primary = libs["mature_trna"], libs["pre_trna"]
    ann = trf.load_annotation(os.path.join(GOLDEN, "libs"), ORG, lambda msg: pytest.fail(msg))
    reads, counts = golden_samples()
    tm, tp = Text(mature.seqs.to_list()), Text(primary.seqs.to_list())
    ps, mm, _ = classify(reads, tm, tp)
    rows = [i for i in range(len(reads)) if ps[i] == MATURE_PASS] + [i for i in range(len(reads)) if ps[i] == PRIMARY_PASS]
    rec = dict(row=[], ref=[], off=[], cls=[], type=[])
    for k, i in enumerate(rows):
        pre, rd = ps[i] == PRIMARY_PASS, reads[i]
        w = tp.windows(rd[:re.search("T{3,}$", rd).start()], 0) if pre else [x for x in tm.windows(rd, 1) if x[1] == mm[i]]
        for ref, off in sorted((tp if pre else tm).where(g) for g, _ in w):
            ty = trf_type(len(rd), pre, off, 0 if pre else len(tm.refs[ref]), 0 if pre else ann.stru[mature.names[ref]]["anticodonStart"] - 1)
            for key, v in zip(("row", "ref", "off", "cls", "type"), (k, ref, off, int(pre), TYPES.index(ty))):
                rec[key].append(v)
    sums = np.zeros((4, len(SAMPLES)), dtype=np.int64)
    for i in rows:
        sums[ps[i]] += counts[i]
    return dict(libs=libs, ann=ann, reads=[reads[i] for i in rows], counts=counts[rows], rec={k: np.asarray(v) for k, v in rec.items()}, sums=sums)


def write(inputs, out_dir, cluster):
    mature, primary = inputs["libs"]["mature_trna"], inputs["libs"]["pre_trna"]
    hits = trf.hits_by_row(inputs["reads"], inputs["rec"], mature.names, primary.names)
    tm = {}
    out = trf.write_reports(out_dir, SAMPLES, inputs["reads"], inputs["counts"], hits, inputs["sums"][MATURE_PASS], inputs["sums"][PRIMARY_PASS],
                            inputs["ann"], dict(zip(primary.names, primary.seqs.to_list())), trf.library_order(mature.names, primary.names),
                            restated_assign(inputs), lambda msg: pytest.fail(msg), cluster, tm)
    return out, tm


def test_cluster_files_equal_the_reference_files(inputs, tmp_path):
    seen = []

    def cluster(groups):
        seen.extend(groups)
        return restated_cluster(groups)
    out, tm = write(inputs, tmp_path, cluster)
    for f in TOP + OLD + NEW:
        with open(os.path.join(GOLDEN, f), "rb") as fh:
            assert (tmp_path / f).read_bytes() == fh.read(), f
    assert out["clusters"]["groups"] == len(seen) and out["clusters"]["points"] == sum(len(g["rows"]) for g in seen)
    assert {"trf_cluster_s", "trf_cluster_text_s"} <= set(tm)
    # the case holds what the restatement has to get right
    sizes = [len(g["rows"]) for g in seen]
    assert 1 in sizes and max(sizes) >= 10
    assert any(len(d.strip("-")) > 64 for g in seen for d in g["dashed"]) and any("N" in d for g in seen for d in g["dashed"])
    res = [restate(g["dashed"], g["rp"]) for g in seen]
    assert {0, 1, 2} <= {int(r["nclust"][0]) for r in res}
    assert any(r["nclust"][0] >= 2 and ((r["halo"] == 0) & (r["cl"] > 0)).sum() >= 2 for r in res)
    assert all(len(set(r["rho"].tolist())) == len(r["rho"]) for r in res)  # (no ties: the reference is defined on the whole case)
    assert all(g["rp"] == [float("%.3f" % x) for x in g["rp"]] for g in seen)


def test_without_the_switch_no_cluster_file_is_written(inputs, tmp_path):
    write(inputs, tmp_path, None)
    assert sorted(os.listdir(tmp_path / "tRFs.samples.tmp")) == sorted(os.path.basename(f) for f in OLD)


def test_equal_densities_stand_in_index_order():
    """rule 4: two points with equal float32 densities -- the restatement's stable argsort and ``cluster_block`` agree on which one is
    the centre, whichever way NumPy's default sort would leave them"""
    t = "ACGTTGCAAGGCTTACGGATCCATGACCTGAAGTCCATTGCAGTCAAGGT"
    dashed = [trf.add_dash(t[0:20], len(t), 1, 20), trf.add_dash(t[2:22], len(t), 3, 22), trf.add_dash(t[30:50], len(t), 31, 50)]
    r = restate(dashed, [7.0, 7.0, 7.0])
    assert r["rho"][0] == r["rho"][1] and r["order"].tolist() == [0, 1, 2]
    assert r["nneigh"].tolist() == [0, 1, 2] and r["delta"].tolist() == [56.0, 4.0, 56.0]
    assert r["nclust"][0] == 2 and r["centre"].tolist() == [1, 3, 0] and r["cl"].tolist() == [1, 1, 2]
    text, content, total = trf.cluster_block("tRNA-X", [(d, "i-tRF", 3, 7.0) for d in dashed], r["cl"].tolist(), r["halo"].tolist(), 2, [1, 3])
    assert "Center Index: 1 Elements: 2 Core: 2 Halo: 0\n" in text and "Center Index: 3 Elements: 1 Core: 1 Halo: 0\n" in text
    assert content[0][:4] == (t[0:20], "i-tRF", "1:20", 6) and total == 21.0
    assert "total Cluster Core RP100K: 14.0+7.0=21.000\n" in text


def test_a_trna_whose_rows_all_overhang_writes_no_block(tmp_path):
    """rule 5: the reference's ``load_data_new`` skips such a tRNA and then pairs every later block with the name before it"""
    ann = trf.Annotation()
    ann.stru = {"tRNA-A": dict(seq="ACGTACGTACGTACGTACGTAGGCT"), "tRNA-B": dict(seq="TTGCAAGGCTTACGGATCCATGACC")}
    pre_seqs = {"pre_tRNA-A_trailer": "GGACGTACGTACGTACGTACGTAGGCTCATTTT"}
    over = (5, 20, "GTAGGCTCATTTTTTT", "-" * 20 + "GTAGGCTCATTTTTTT", "tRF-1", 900.0, 0)   # longer than its template: dropped from the report
    rows_b = [(4, 0, "TTGCAAGGCTTACGGATC", "TTGCAAGGCTTACGGATC-------", "5'-tRF", 700.0, 1)]
    blocks = {"S": [("pre_tRNA-A_trailer", pre_seqs["pre_tRNA-A_trailer"], [t for t in [over] if len(t[3]) == 33]),
                    ("tRNA-B", ann.stru["tRNA-B"]["seq"], rows_b)]}
    os.makedirs(tmp_path / "t")
    out = trf.write_clusters(tmp_path / "t", ["S"], blocks, restated_cluster, ann, pre_seqs)
    assert out["groups"] == 1 and out["points"] == 1
    detail = (tmp_path / "t" / "S.aligned_tRFs.clusters.detail").read_text()
    assert detail.startswith("tRNA-B:\n") and "pre_tRNA-A_trailer" not in detail and detail.count("Summary:") == 1
    tsv = (tmp_path / "t" / "S.tRFs.report.tsv").read_text().splitlines()
    assert len(tsv) == 2 and tsv[1].split("\t")[:4] == ["tRNA-B", ann.stru["tRNA-B"]["seq"], "TTGCAAGGCTTACGGATC", "N:"]


def test_a_template_beyond_the_cap_is_refused_by_name(tmp_path):
    ann = trf.Annotation()
    long_t = "ACGT" * 70
    rows = [(1, 0, long_t[:20], long_t[:20] + "-" * 260, "5'-tRF", 50.0, 0)]
    with pytest.raises(trf.TemplateTooLong, match="tRNA-L has 280 columns"):
        trf.write_clusters(tmp_path, ["S"], {"S": [("tRNA-L", long_t, rows)]}, restated_cluster, ann, {})
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("extra", [["-spl"], ["-rr"], ["--backend", "bowtie"]])
def test_switch_implies_the_report_and_carries_its_refusals(extra, capsys):
    base = ["-s", "x.fastq", "-lib", "L", "-on", "human"]
    args = parse_args(base + ["--trf-clusters"])
    assert args.trf_clusters and args.trf_report
    assert not parse_args(base + ["--trf-report"]).trf_clusters
    with pytest.raises(SystemExit):
        parse_args(base + ["--trf-clusters"] + extra)
    assert "--trf-clusters run on the device-resident route" in capsys.readouterr().err

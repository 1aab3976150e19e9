"""``--trf-report`` on the host (mirge3_amd/trf.py): the six files produced from brute-force hit records and the restated
``assign_cluster`` against the golden files the reference wrote (tests/golden/case8_trf, made by tests/golden/make_golden_trf.py),
byte for byte; the annotation parser; the switch's refusals.  The device calls that deliver the records and the assignment in a real
run are held against the same brute force in tests/test_trf_hostsim.py (CPU) and tests/test_trf_gpu.py."""
import os
from collections import Counter

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import trf
from mirge3_amd.cli import parse_args
from mirge3_amd.seqio import load_library_dir

from test_trf_hostsim import MATURE_PASS, PRIMARY_PASS, TYPES, Text, assign_cluster, classify, trf_type

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "case8_trf")
ORG, DB = "synthorg", "miRBase"
SAMPLES = ["S1", "S2", "S3"]
SIX = ["tRFs.aligned.report.tsv", "tRF.Counts.csv", "tRF.RP100K.csv", "discarded.reads.summary.assigningtRFs.csv"] + \
      [os.path.join("tRFs.samples.tmp", s + suffix) for s in SAMPLES for suffix in (".aligned_tRFs.report", ".aligned_tRFs.summary.report")]


def golden_samples():
    """-> (reads in mapped.csv's order: the sorted union, counts [reads, samples])"""
    per = []
    for s in SAMPLES:
        with open(os.path.join(GOLDEN, s + ".fastq")) as fh:
            per.append(Counter(ln.strip() for k, ln in enumerate(fh) if k % 4 == 1))
    reads = sorted(set().union(*per))
    return reads, np.asarray([[c[r] for c in per] for r in reads], dtype=np.int64)


def brute_force_inputs():
    """what ``trf.run`` collects from the device, by brute force: the report's rows, their counts, EVERY window of every row as
    records sorted by (row, ref, off), and the class sums"""
    libs = load_library_dir(os.path.join(GOLDEN, "libs"), ORG, DB)
    mature, primary = libs["mature_trna"], libs["pre_trna"]
    ann = trf.load_annotation(os.path.join(GOLDEN, "libs"), ORG, lambda msg: pytest.fail(msg))
    reads, counts = golden_samples()
    tm, tp = Text(mature.seqs.to_list()), Text(primary.seqs.to_list())
    ps, mm, _ = classify(reads, tm, tp)
    rows = [i for i in range(len(reads)) if ps[i] == MATURE_PASS] + [i for i in range(len(reads)) if ps[i] == PRIMARY_PASS]
    rec = dict(row=[], ref=[], off=[], cls=[], type=[])
    for k, i in enumerate(rows):
        pre = ps[i] == PRIMARY_PASS
        rd = reads[i]
        if pre:
            import re
            w = tp.windows(rd[:re.search("T{3,}$", rd).start()], 0)
        else:
            w = [x for x in tm.windows(rd, 1) if x[1] == mm[i]]
        for ref, off in sorted((tp if pre else tm).where(g) for g, _ in w):
            ty = trf_type(len(rd), pre, off, 0 if pre else len(tm.refs[ref]), 0 if pre else ann.stru[mature.names[ref]]["anticodonStart"] - 1)
            for key, v in zip(("row", "ref", "off", "cls", "type"), (k, ref, off, int(pre), TYPES.index(ty))):
                rec[key].append(v)
    rec = {k: np.asarray(v) for k, v in rec.items()}
    sums = np.zeros((4, len(SAMPLES)), dtype=np.int64)
    for i in rows:
        sums[ps[i]] += counts[i]
    return dict(libs=libs, ann=ann, reads=[reads[i] for i in rows], counts=counts[rows], rec=rec, sums=sums)


@pytest.fixture(scope="module")
def inputs():
    return brute_force_inputs()


def restated_assign(inp):
    """``assign(rows)`` of ``trf.write_reports`` from ``assign_cluster`` restated (tests/test_trf_hostsim.py)"""
    ann, mature, primary = inp["ann"], inp["libs"]["mature_trna"], inp["libs"]["pre_trna"]
    tabs = trf.InforTables(ann.infor)
    length = {nm: len(s) for lib in (mature, primary) for nm, s in zip(lib.names, lib.seqs.to_list())}

    def assign(rows):
        dist, idx = [], []
        for k, name, start in rows:
            rd = inp["reads"][k]
            d, cluster = assign_cluster(trf.add_dash(rd, length[name], start, start + len(rd) - 1), ann.infor.get(name))
            dist.append(d)
            if cluster is None:
                idx.append(-1)
                continue
            lo, hi = tabs.ref_ptr[tabs.index[name]], tabs.ref_ptr[tabs.index[name] + 1]
            idx.append(next(t for t in range(lo, hi) if tabs.names[t] == cluster))
        return dist, idx
    return assign


def test_reports_equal_the_reference_files(inputs, tmp_path):
    mature, primary = inputs["libs"]["mature_trna"], inputs["libs"]["pre_trna"]
    hits = trf.hits_by_row(inputs["reads"], inputs["rec"], mature.names, primary.names)
    assert any(len(h) > 1 for h in hits) and len(inputs["rec"]["row"]) > sum(len(h) for h in hits)  # (rule 1 had something to drop)
    said = []
    out = trf.write_reports(tmp_path, SAMPLES, inputs["reads"], inputs["counts"], hits, inputs["sums"][MATURE_PASS], inputs["sums"][PRIMARY_PASS],
                            inputs["ann"], dict(zip(primary.names, primary.seqs.to_list())), trf.library_order(mature.names, primary.names),
                            restated_assign(inputs), said.append)
    assert not said and out["printed"] == out["rows"] == len(inputs["reads"])
    for f in SIX:
        with open(os.path.join(GOLDEN, f), "rb") as fh:
            assert (tmp_path / f).read_bytes() == fh.read(), f
    assert sorted(os.listdir(tmp_path / "tRFs.samples.tmp")) == sorted(os.path.basename(f) for f in SIX[4:])  # no clustering files


def test_uid_is_the_reference_uid(inputs):
    with open(os.path.join(GOLDEN, SIX[0])) as fh:
        rows = [ln.split("\t")[:2] for ln in fh.readlines()[1:]]
    assert len(rows) > 100 and {len(s) % 5 for s, _ in rows} == {0, 1, 2, 3, 4}
    for seq, u in rows:
        assert u == ("." if "N" in seq else trf.uid(seq))


def test_a_stand_in_that_is_no_hit_is_left_out_and_logged(inputs, tmp_path):
    """the reference raises KeyError there (mirge2_tRF_a2i.py:583)"""
    import copy
    mature, primary = inputs["libs"]["mature_trna"], inputs["libs"]["pre_trna"]
    ann = copy.deepcopy(inputs["ann"])
    ann.dedup[mature.names[6]] = mature.names[9]  # reference 9 is no hit of the reads of reference 6
    hits = trf.hits_by_row(inputs["reads"], inputs["rec"], mature.names, primary.names)
    said = []
    out = trf.write_reports(tmp_path, SAMPLES, inputs["reads"], inputs["counts"], hits, inputs["sums"][MATURE_PASS], inputs["sums"][PRIMARY_PASS],
                            ann, dict(zip(primary.names, primary.seqs.to_list())), trf.library_order(mature.names, primary.names),
                            restated_assign(inputs), said.append)
    only_6 = [k for k, h in enumerate(hits) if [x[0] for x in h] == [mature.names[6]]]
    assert only_6 and out["printed"] == out["rows"] - len(only_6)
    assert len(said) == 1 and inputs["reads"][only_6[0]] in said[0]


def test_missing_annotation_file_says_the_reference_line(tmp_path):
    import shutil
    shutil.copytree(os.path.join(GOLDEN, "libs"), tmp_path / "libs")
    os.remove(tmp_path / "libs" / ORG / "annotation.Libs" / f"{ORG}_tRF_infor.csv")
    said = []
    assert trf.load_annotation(tmp_path / "libs", ORG, said.append) is None
    path = tmp_path / "libs" / ORG / "annotation.Libs" / f"{ORG}_tRF_infor.csv"
    assert said == [f"File {path} does not exist!!\nProceeding the annotation with out -trf\n"]


def test_annotation_tables(inputs):
    ann = inputs["ann"]
    names = inputs["libs"]["mature_trna"].names
    assert ann.dedup[names[1]] == names[0] and names[5] not in ann.infor and all(ann.stru[nm]["anticodonStart"] == 34 for nm in names)
    assert len(ann.infor[names[9]]) == 2  # two lines with one dashed string: one entry, the later line's name
    assert sorted(ann.infor[names[9]].values())[0].endswith("_Cluster2")
    tabs = trf.InforTables(ann.infor)
    assert tabs.ref_ptr[-1] == len(tabs.strings) == sum(len(v) for v in ann.infor.values())
    k9, k10 = (tabs.names.index(names[8] + "_Cluster" + t) for t in ("9", "10"))
    assert tabs.rank[k10] < tabs.rank[k9]  # Python's string order


@pytest.mark.parametrize("extra", [["-spl"], ["-rr"], ["--backend", "bowtie"]])
def test_switch_refused_off_the_device_route(extra, capsys):
    base = ["-s", "x.fastq", "-lib", "L", "-on", "human"]
    assert parse_args(base + ["--trf-report"]).trf_report
    with pytest.raises(SystemExit):
        parse_args(base + ["--trf-report"] + extra)
    assert "--trf-report runs on the device-resident route" in capsys.readouterr().err


def test_trf_itself_stays_refused():
    with pytest.raises(SystemExit):
        parse_args(["-s", "x.fastq", "-lib", "L", "-on", "human", "-trf"])

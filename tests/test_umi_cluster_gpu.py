"""``--umi-cluster directional`` on the MI355X: ``mirge_umi_cluster`` (csrc/native_umi.hpp, csrc/kernels_umi.hpp) through the C ABI on
the cases of tests/umi_cases.py -- inputs built with ``DeviceReads.pack`` + ``collapse(weights=counts)`` so that counts are free to choose --
then the route through ``mirge_reads_parse_umi`` / ``parse_sample`` on FASTQ text and the command line.  Everything is compared exactly
with the restatement (tests/umi_restate.py), which runs UMI-tools' sequential search with ties both ways on every input used here."""
import os

import numpy as np
import pytest

import umi_cases
import umi_restate
from helpers import GoldenCase, ORG
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi
from mirge3_amd.collapse import ILLUMINA_3P, parse_sample
from mirge3_amd.seqio import FlatSeqs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def cluster(ctx, reads, counts, f, b):
    """-> founder flags in the order of `reads` (mirge_umi_cluster answers in handle order), and the call's statistics"""
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(list(reads)))
    tagged = raw.collapse(weights=np.asarray(counts, dtype=np.uint32))
    try:
        assert len(tagged) == len(reads)
        got = tagged.umi_cluster(f, b)
        stats = _ffi.umi_cluster_stats()
        if not len(reads):
            return got, stats
        cnt, first = tagged.counts()
        assert np.array_equal(np.sort(first), np.arange(len(reads)))  # a read's first index is its position in `reads`
        assert np.array_equal(cnt[np.argsort(first), 0], np.asarray(counts, dtype=np.uint32))
        out = np.zeros(len(reads), np.uint8)
        out[first] = got
        return out, stats
    finally:
        tagged.close(); raw.close()


@pytest.mark.parametrize("name", sorted(umi_cases.all_cases()))
def test_flags_equal_the_restatement(ctx, name):
    _, reads, counts, f, b = umi_cases.all_cases()[name]
    want = umi_cases.expected(name)
    got, stats = cluster(ctx, reads, counts, f, b)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, bad[:5], [reads[i] for i in bad[:5]])
    assert stats["tagged"] == len(reads) and stats["eligible"] == sum(umi_restate.eligible(r, f, b) for r in reads)
    if name == "chain_alone":
        assert stats["linked"] == 600 and stats["rounds"] >= 2


def test_collisions_change_nothing(ctx, monkeypatch):
    _, reads, counts, f, b = umi_cases.all_cases()["collisions"]
    plain, _ = cluster(ctx, reads, counts, f, b)
    monkeypatch.setenv("MIRGE_TEST_UMI_HASH_BITS", "6")
    hooked, _ = cluster(ctx, reads, counts, f, b)
    monkeypatch.delenv("MIRGE_TEST_UMI_HASH_BITS")
    assert np.array_equal(hooked, plain) and np.array_equal(plain, umi_cases.expected("collisions"))


def test_bad_layouts_and_handles_are_refused(ctx):
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(["ACGTACGTACGTACGTACGTAC", "ACGTACGTACGTACGTACGTAA"]))
    tagged = raw.collapse()
    for f, b in ((-1, 4), (4, -1), (0, 0), (20, 20), (33, 0)):
        with pytest.raises(RuntimeError, match="f \\+ b"):
            tagged.umi_cluster(f, b)
    with pytest.raises(RuntimeError, match="collapse result"):
        raw.umi_cluster(4, 4)
    assert tagged.umi_cluster(16, 16).tolist() == [1, 1]  # len < f + b
    tagged.close(); raw.close()


# ---- the route: FASTQ text -> mirge_reads_parse_umi -> inserts of the founders

def _fastq(reads):
    return "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(reads)).encode()


def _library(seed, f, b, adapter, qiagen, n=1500):
    """reads of a UMI library: a few inserts (one of them heavy, one too short), UMIs with PCR copies and one-letter errors"""
    rng = np.random.default_rng(seed)
    inserts = [umi_cases.rand_seq(rng, int(rng.integers(17, 30))) for _ in range(12)] + ["ACGTACGTACGT"]
    reads = []
    while len(reads) < n:
        ins = inserts[min(int(rng.pareto(0.7)), len(inserts) - 1)]
        u = umi_cases.rand_seq(np.random.default_rng(int(rng.integers(0, 60))), f + b)  # 60 UMIs: molecules repeat
        for _ in range(int(rng.geometric(0.4))):
            v = u
            if rng.random() < 0.3:
                v = umi_cases.mutate(u, int(rng.integers(0, f + b)), int(rng.integers(1, 4)))
            reads.append((ins + adapter + v + "AGATCGGAAGAGC") if qiagen else (v[:f] + ins + v[f:] + adapter + "AGATC"))
    return reads


def _dictionary(raw):
    uniq = raw.collapse()
    cnt, first = uniq.counts()
    seqs = uniq.unpack().to_list()
    order = np.argsort(first, kind="stable")
    uniq.close()
    return [(seqs[i], int(cnt[i, 0])) for i in order]


ROUTES = [("4N", 4, 4, ILLUMINA_3P, False, 16), ("qiagen", 0, 12, "AACTGTAGGCACCATCAAT", True, 16), ("4N_min0", 4, 4, ILLUMINA_3P, False, 0)]


@pytest.mark.parametrize("tag,f,b,adapter,qiagen,min_len", ROUTES)
def test_parse_route(ctx, tmp_path, tag, f, b, adapter, qiagen, min_len):
    text = _fastq(_library(len(tag), f, b, adapter, qiagen))
    trim = _ffi.MirgeTrim.make(adapter=adapter, quality_back=10, count_per_modifier=False)
    out = {}
    for mode in (None, "directional"):
        wd = tmp_path / str(mode)
        wd.mkdir()
        umi = _ffi.MirgeUmi.make(f, b, qiagen=qiagen, dedup=True, cluster=mode)
        assert umi.dedup == (2 if mode else 1)
        raw, n_rec = parse_sample(ctx, text, min_len, trim, umi, wd, "S")
        out[mode] = dict(n=len(raw), d=_dictionary(raw), csv=(wd / "S_umiCounts.csv").read_bytes(), wd=wd)
        raw.close()
    # the tagged reads as -udd sees them: the rows of _umiCounts.csv hold those whose insert passes the length test; the others (an
    # insert below min_len) are nodes too, so the graph is restated from the device's own tagged reads
    raw, n_rec, tagged = _ffi.DeviceReads.parse_umi(ctx, text, 0, min_len, trim, _ffi.MirgeUmi.make(f, b, qiagen=qiagen, dedup=True))
    order = tagged.first_appearance_order()
    treads = [tagged.unpack().to_list()[i] for i in order]
    tcounts = tagged.counts()[0][order, 0].tolist()
    raw.close(); tagged.close()
    flags = umi_restate.founders(treads, tcounts, list(range(len(treads))), f, b)
    want = umi_restate.insert_counts(treads, flags, f, b, min_len)
    udd, dire = out[None], out["directional"]
    assert 0 < sum(flags) < len(flags)
    got = dict(dire["d"])
    assert got == {k: v for k, v in want.items() if v} and set(got) == set(want)  # every insert keeps a founder
    assert set(got) == set(dict(udd["d"])) and all(got[k] <= v for k, v in udd["d"])
    assert dire["n"] == sum(want.values()) and dire["n"] < udd["n"]
    # rows stand where their earliest founder appeared
    seen = []
    for t, fl in zip(treads, flags):
        ins = umi_restate.split(t, f, b)[1]
        if fl and len(ins) >= min_len and ins not in seen:
            seen.append(ins)
    assert [k for k, _ in dire["d"]] == seen
    assert dire["csv"] == udd["csv"] and not (udd["wd"] / "S_umiClusters.csv").exists()
    lines = ["UMISeq,transcriptSeq,UMICounts,Founder"]
    for t, c, fl in zip(treads, tcounts, flags):
        u, ins = umi_restate.split(t, f, b)
        if len(ins) >= min_len:
            lines.append(f"{u},{ins},{c},{fl}")
    assert (dire["wd"] / "S_umiClusters.csv").read_text() == "\n".join(lines) + "\n"
    elig = sum(umi_restate.eligible(t, f, b) for t in treads)
    assert (dire["wd"] / "run.log").read_text().strip().endswith(
        f"{len(treads)} distinct UMI-tagged reads, {elig} eligible, {sum(flags)} founders")


def test_command_line(tmp_path):
    from test_gpu_parity import _run_cli
    case = GoldenCase("case1_single")
    reads = _library(9, 4, 4, ILLUMINA_3P, False, n=400)
    p = tmp_path / "s.fastq"
    p.write_bytes(_fastq(reads))
    common = ["-s", str(p), "-lib", case.libdir, "-on", ORG, "-db", "miRBase", "-o", str(tmp_path), "-shh", "-a", "illumina", "-umi", "4,4",
              "-udd", "--trim-count", "once"]
    _run_cli(common + ["-dn", "udd"])
    _run_cli(common + ["-dn", "dir", "--umi-cluster", "directional"])
    rows = {}
    for d in ("udd", "dir"):
        rows[d] = {}
        for name in ("mapped.csv", "unmapped.csv"):
            for line in (tmp_path / d / name).read_text().splitlines()[1:]:
                rows[d][line.split(",")[0]] = int(line.rsplit(",", 1)[1])
    csv = (tmp_path / "dir" / "s_umiClusters.csv").read_text().splitlines()[1:]
    treads, tcounts = [], []
    for line in csv:
        u, ins, c, _ = line.split(",")
        treads.append(u[:4] + ins + u[4:]); tcounts.append(int(c))
    # (tagged reads whose insert is below -m 16 are not in the file: they have inserts of their own, so they are nobody's neighbours here)
    flags = umi_restate.founders(treads, tcounts, list(range(len(treads))), 4, 4)
    assert [int(line.rsplit(",", 1)[1]) for line in csv] == flags and 0 < sum(flags) < len(flags)
    want = umi_restate.insert_counts(treads, flags, 4, 4, 16)
    assert rows["dir"] == want and set(rows["dir"]) == set(rows["udd"]) and sum(rows["dir"].values()) < sum(rows["udd"].values())
    assert (tmp_path / "dir" / "s_umiCounts.csv").read_bytes() == (tmp_path / "udd" / "s_umiCounts.csv").read_bytes()
    assert not (tmp_path / "udd" / "s_umiClusters.csv").exists()

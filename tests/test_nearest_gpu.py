"""``--unmapped-nearest`` on the MI355X.  ``mirge_nearest_scan`` through the C ABI equals the restatement (tests/near_restate.py) exactly on
every named case (tests/near_cases.py) and on the random set, with chunks of 64 bases and of the default size, and with every query in the
64-bit instance.  ``mirge_nearest_unmapped`` on a dictionary of about 2 000 reads made from the hairpins of tests/golden/case4_gff_a2i by
substring plus edits, with reads the cascade annotates mixed in: the fetched rows are exactly the restatement's rows of the unannotated
reads, the stats the counted numbers.  The CLI on that FASTQ: both files equal what ``nearest.py``'s writers make of the restatement's rows,
``unmapped.nearest.csv`` is a subsequence of ``unmapped.csv``, and a run without the switch writes the same tables."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import near_cases
import near_restate
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, nearest, seqio
from mirge3_amd.cascade import Cascade
from mirge3_amd.seqio import FlatSeqs
from mirge3_amd.unmapped import read_unmapped_csv

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
LIBS4 = os.path.join(HERE, "golden", "case4_gff_a2i", "libs")
FIELDS = ("dist", "hairpin", "start", "end")
CHUNK = "MIRGE_NEAR_CHUNK_BASES"


@pytest.fixture(scope="module")
def gctx():
    ctx = _ffi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture
def clean_env(monkeypatch):
    monkeypatch.delenv(CHUNK, raising=False)
    monkeypatch.delenv("MIRGE_NEAR_FORCE64", raising=False)
    return monkeypatch


def scan_sets():
    return [(c["name"], c["hairpins"], c["queries"]) for c in near_cases.CASES] + \
        [(f"random{k}", h, q) for k, (h, q) in enumerate(near_cases.random_sets())]


@pytest.fixture(scope="module")
def scan_want():
    """the restatement of every set, computed once"""
    return {name: near_restate.nearest_all(q, h) for name, h, q in scan_sets()}


@pytest.mark.parametrize("chunk,force64", [("64", None), (None, None), ("64", "1")], ids=["chunk64", "default", "chunk64-all-in-64-bit"])
def test_scan_equals_the_restatement(gctx, clean_env, scan_want, chunk, force64):
    if chunk:
        clean_env.setenv(CHUNK, chunk)
    if force64:
        clean_env.setenv("MIRGE_NEAR_FORCE64", force64)
    for name, hairpins, queries in scan_sets():
        got = _ffi.nearest_scan(gctx, queries, hairpins)
        for k in FIELDS:
            assert np.array_equal(got[k].astype(np.int64), scan_want[name][k]), (name, k, np.flatnonzero(got[k] != scan_want[name][k])[:5])


def test_scan_refuses_a_wrong_chunk_size(gctx, clean_env):
    for bad in ("0", "4097", "x"):
        clean_env.setenv(CHUNK, bad)
        with pytest.raises(RuntimeError, match="MIRGE_NEAR_CHUNK_BASES"):
            _ffi.nearest_scan(gctx, ["ACGTACGTACGT"], ["ACGTACGTACGTAA"])
    clean_env.delenv(CHUNK)
    assert _ffi.nearest_scan(gctx, [], ["ACGT"])["dist"].shape == (0,)


# ------------------------------------------------------------------------------------------------------------------ the dictionary
def make_reads():
    """-> (libs of case 4, the reads of two samples): near misses of the hairpins, reads the cascade annotates, random reads, lengths from
    8 to 90"""
    libs = seqio.load_library_dir(LIBS4, "human", "miRBase")
    hp = libs["hairpin"].seqs.to_list()
    mir = libs["mirna"].seqs.to_list()
    rng = random.Random(404)
    reads = []
    for _ in range(1400):
        h = rng.choice(hp)
        n = rng.randint(14, min(64, len(h))) if rng.random() < 0.8 else rng.randint(8, 13)
        at = rng.randrange(len(h) - n + 1)
        reads.append(near_cases.edit(rng, h[at:at + n], rng.choice([0, 1, 1, 1, 2, 2, 3, 4, 5])))
    reads += [rng.choice(mir) for _ in range(300)]                                  # exact miRNAs: annotated
    reads += [near_cases.rnd_seq(rng, rng.randint(8, 90)) for _ in range(200)]       # nothing known, some too short, some too long
    reads += [near_cases.rnd_seq(rng, rng.randint(8, 11), "ACGTNNNN") for _ in range(80)]  # too short, and too many N for any pass
    reads += [rng.choice(hp)[:rng.randint(65, 68)] for _ in range(20)]               # too long for the scan, known to the hairpin pass
    reads += [rng.choice(reads[:1400]) for _ in range(200)]                           # counts above one
    rng.shuffle(reads)
    cut = len(reads) * 3 // 5
    return libs, [reads[:cut], reads[cut - 300:]]


@pytest.fixture(scope="module")
def made():
    libs, samples = make_reads()
    every = sorted(set(samples[0]) | set(samples[1]))
    hp = libs["hairpin"].seqs.to_list()
    want = near_restate.nearest_many(every, hp)  # once, for the dictionary and for the command line
    return libs, samples, {q: tuple(int(want[k][i]) for k in FIELDS) for i, q in enumerate(every)}


@pytest.mark.parametrize("K,chunk", [(3, None), (1, "64"), (8, "64")])
def test_unmapped_route_fetches_the_restatements_rows(gctx, clean_env, made, K, chunk):
    libs, samples, want = made
    if chunk:
        clean_env.setenv(CHUNK, chunk)
    casc = Cascade(gctx, libs)
    raw = _ffi.DeviceReads.pack(gctx, FlatSeqs.from_list(samples[0] + samples[1]))
    uniq = raw.collapse()
    raw.close()
    res = casc.run(uniq)
    try:
        ps = res.fetch()[0]
        useq = uniq.unpack().to_list()
        assert 1500 <= len(useq) <= 2200
        unm = [i for i in range(len(useq)) if ps[i] < 0]
        assert 300 <= len(useq) - len(unm)  # reads the cascade annotates are mixed in
        got, stats = _ffi.nearest_unmapped(gctx, uniq, res, libs["hairpin"].seqs, K)
        rows = [i for i in unm if near_restate.reported(useq[i], want[useq[i]][0], K)]
        assert got["row"].tolist() == rows and len(rows) >= 200
        assert [tuple(int(got[k][j]) for k in FIELDS) for j in range(len(rows))] == [want[useq[i]] for i in rows]
        lens = [len(useq[i]) for i in unm]
        assert stats == dict(unmapped=len(unm), short=sum(n < 12 for n in lens), long=sum(n > 64 for n in lens),
                             considered=sum(12 <= n <= 64 for n in lens), reported=len(rows))
        assert stats["short"] >= 20 and stats["long"] >= 20
        # some kept row sits on each side of the instances' bound, and at every distance up to min(K, 3)
        assert {len(useq[i]) <= 32 for i in rows} == {True, False}
        assert set(range(min(K, 3) + 1)) <= set(got["dist"].tolist())
        # K outside 1 .. 8 is refused; a library without a base keeps nothing and counts all the same
        for bad in (0, 9):
            with pytest.raises(RuntimeError, match="K is 1 .. 8"):
                _ffi.nearest_unmapped(gctx, uniq, res, libs["hairpin"].seqs, bad)
        none, st0 = _ffi.nearest_unmapped(gctx, uniq, res, ["", ""], K)
        assert none["row"].shape == (0,) and st0 == dict(stats, reported=0)
    finally:
        res.close()
        uniq.close()
        casc.close()


# ------------------------------------------------------------------------------------------------------------------ the command line
def _cli(argv, env=None):
    cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); import mirge3_amd; from mirge3_amd.cli import main; main()" % ROOT]
    r = subprocess.run(cmd + list(argv), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_cli_writes_what_the_writers_make_of_the_restatement(tmp_path, made):
    """(the CLI is what this test is about: one run with the switch, one without)"""
    libs, samples, want = made
    names = ["S1", "S2"]
    files = []
    for nm, reads in zip(names, samples):
        p = tmp_path / f"{nm}.fastq"
        p.write_text("".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(reads)))
        files.append(str(p))
    env = {k: v for k, v in os.environ.items() if k not in (CHUNK, "MIRGE_NEAR_FORCE64", "WORLD_SIZE")}
    base = ["-s", ",".join(files), "-lib", LIBS4, "-on", "human", "-db", "miRBase", "-o", str(tmp_path), "-shh", "-m", "8"]
    K = 4
    _cli(base + ["-dn", "near", "--unmapped-nearest", str(K)], env)
    _cli(base + ["-dn", "plain"], env)
    near, plain = tmp_path / "near", tmp_path / "plain"
    for f in ("unmapped.csv", "mapped.csv", "miR.Counts.csv", "miR.RPM.csv", "annotation.report.csv"):
        assert (near / f).read_bytes() == (plain / f).read_bytes(), f
    assert sorted(set(os.listdir(near)) - set(os.listdir(plain))) == [nearest.SUMMARY_NAME, nearest.FILE_NAME]
    seqs, counts = read_unmapped_csv(near / "unmapped.csv", names)
    assert len(seqs) >= 800 and all(s in want for s in seqs)
    rows = [i for i, s in enumerate(seqs) if near_restate.reported(s, want[s][0], K)]
    assert len(rows) >= 200
    hits = dict(row=np.array(rows), **{k: np.array([want[seqs[i]][j] for i in rows]) for j, k in enumerate(FIELDS)})
    hp = libs["hairpin"]
    hp_names, hp_seqs = nearest.hairpin_names(hp), hp.seqs.to_list()
    index = nearest.mature_index(nearest.mature_tables(LIBS4, "human", "miRBase", libs["mirna"].names, hp), hp_names, hp_seqs)
    text = (near / nearest.FILE_NAME).read_text()
    assert text == nearest.file_text(names, seqs, counts, hits, hp_names, hp_seqs, index)
    summary = nearest.summary_rows(names, [len(s) for s in seqs], counts, hits, K)
    assert (near / nearest.SUMMARY_NAME).read_text() == nearest.summary_text(names, summary, K)
    # a subsequence of unmapped.csv with equal counts
    body = [ln.split(",") for ln in text.split("\n")[1:] if ln]
    at = {s: i for i, s in enumerate(seqs)}
    where = [at[f[0]] for f in body]
    assert where == sorted(where) == rows
    assert [[int(x) for x in f[-2:]] for f in body] == [counts[i].tolist() for i in where]
    assert sum(1 for f in body if f[6]) >= 50 and any("/" in f[6] for f in body)  # the mature column is filled where a canonical is overlapped
    log = (near / "run.log").read_text()
    for nm, row in zip(names, summary):
        assert nearest.log_line(nm, row, K) in log
    assert "unmapped nearest" not in (plain / "run.log").read_text()

"""``--umi-cluster directional`` without a GPU: the closed form the device computes against UMI-tools' sequential search on random UMI
sets (tests/umi_restate.py), the ``mirge_umi`` struct, and the command line's refusals."""
import subprocess
import sys
import os

import numpy as np
import pytest

import umi_restate
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_closed_form_equals_the_sequential_search_on_random_sets():
    """3 000 sets over a 2-letter alphabet of short UMIs (dense graphs: long chains of ties, components of count-1 nodes that touch big
    nodes), counts skewed towards 1 and 2: the number of searches with ties by first appearance, with ties reversed, and the founders of
    the closed form never differ"""
    rng = np.random.default_rng(1)
    alphabets = ("AC", "ACG", "ACGT")
    for k in range(3000):
        f, b = ((2, 2), (0, 5), (4, 0), (3, 3))[k % 4]
        inserts = ["GATTACAGATTACA", "TTGACCA"][: 1 + k % 2]
        letters = alphabets[k % 3]
        tagged = set()
        for _ in range(int(rng.integers(1, 40))):
            u = "".join(letters[int(x)] for x in rng.integers(0, len(letters), f + b))
            ins = inserts[int(rng.integers(0, len(inserts)))]
            tagged.add(u[:f] + ins + u[f:])
        tagged = sorted(tagged)
        order = rng.permutation(len(tagged))
        tagged = [tagged[i] for i in order]
        counts = rng.choice([1, 1, 1, 2, 2, 3, 4, 5, 9, 30], size=len(tagged)).tolist()
        flags = umi_restate.founders(tagged, counts, list(range(len(tagged))), f, b)  # asserts the three counts
        per_insert = umi_restate.insert_counts(tagged, flags, f, b)
        assert all(v >= 1 for v in per_insert.values())  # every insert keeps a founder


def test_founders_of_a_known_network():
    # UMI-tools' own example shape: a hub of 456 with one-letter variants of 2 and 72, and a variant of the 72's of 1; a lone 90
    t = {"ACGT": 456, "TCGT": 2, "CCGT": 2, "ACAT": 72, "AAAT": 90, "ACAG": 1}
    tagged = [u + "GATTACAGATTACAGA" for u in t]
    flags = umi_restate.founders(tagged, list(t.values()), list(range(len(t))), 4, 0)
    # ACGT founds; TCGT, CCGT, ACAT hang off it (456 >= 2*72 - 1); ACAG off ACAT; AAAT is a neighbour of ACAT only: 72 < 2*90 - 1
    assert flags == [1, 0, 0, 0, 1, 0]


def test_the_struct():
    u = _ffi.MirgeUmi.make(4, 4, dedup=True, cluster="directional")
    assert (u.front, u.back, u.qiagen, u.dedup, u.cluster) == (4, 4, 0, 2, "directional")
    assert _ffi.MirgeUmi.make(4, 4, dedup=True).dedup == 1 and _ffi.MirgeUmi.make(4, 4, dedup=True, cluster="none").dedup == 1
    assert _ffi.MirgeUmi.make(4, 4).dedup == 0 and _ffi.MirgeUmi.make(0, 12, True, True).dedup == 1
    for bad in (dict(front=4, back=4, cluster="directional"), dict(front=20, back=20, dedup=True, cluster="directional"),
                dict(front=0, back=0, dedup=True, cluster="directional"), dict(front=4, back=4, dedup=True, cluster="adjacency")):
        with pytest.raises(ValueError):
            _ffi.MirgeUmi.make(**bad)
    from types import SimpleNamespace
    from mirge3_amd.collapse import umi_from_args
    assert umi_from_args(SimpleNamespace(uniq_mol_ids="4,4", umiDedup=True, umi_cluster="directional")).dedup == 2
    assert umi_from_args(SimpleNamespace(uniq_mol_ids="4,4", umiDedup=True, umi_cluster="none")).dedup == 1
    assert umi_from_args(SimpleNamespace(uniq_mol_ids="4,4", umiDedup=True)).dedup == 1


@pytest.mark.parametrize("extra", [["-umi", "4,4", "--umi-cluster", "directional"], ["-umi", "20,20", "-udd", "--umi-cluster", "directional"],
                                   ["-umi", "0,0", "-udd", "--umi-cluster", "directional"], ["-umi", "4,4", "-udd", "--umi-cluster", "adjacency"]])
def test_the_command_line_refuses_before_it_writes(tmp_path, extra):
    s = tmp_path / "s.fastq"
    s.write_text("@r\nACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIII\n")
    out = tmp_path / "out"
    out.mkdir()
    cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); import mirge3_amd; from mirge3_amd.cli import main; main()" % ROOT,
           "-s", str(s), "-lib", str(tmp_path), "-on", "human", "-o", str(out), "-shh"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--umi-cluster" in r.stderr
    assert list(out.iterdir()) == []

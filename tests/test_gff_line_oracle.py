"""The oracle's restatement of one whole LINE of the miRTop GFF3 (oracle.gff_line, oracle.gff_uid: create_gff,
summary.py:131-192, and miRgeEssential.UID, :364-370) against what the reference wrote and returned (golden cases 4 and 6),
and the host writer's UID rule (uid_append, csrc/native_host.hpp, reached through mirge_gff_write) against the restatement on
every last stretch there is.  No GPU: the device writer is compared with both in tests/test_gff_device_gpu.py."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import oracle
from helpers import GOLDEN
from test_a2i_gff_oracle import GFF_A2I_CASES, _case4_gff_tables


@pytest.mark.parametrize("case_name", GFF_A2I_CASES)
def test_gff_line_restatement_equals_the_reference_file(case_name):
    """every line below the head of the file create_gff wrote, byte for byte, from the name, the read and the counts alone"""
    case, mat, pre, pre_of = _case4_gff_tables(case_name)
    lines = open(os.path.join(case.dir, "sample_miRge3.gff")).read().splitlines(keepends=True)
    assert lines[2].startswith("## source-ontology: ")
    source = lines[2].split(": ")[1].strip()
    n = n_with_n = 0
    prefixes = set()
    for ln in lines:
        if ln.startswith("#"):
            continue
        f = ln.rstrip("\n").split("\t")
        attrs = dict(x.split("=", 1) for x in f[8].split("; "))
        assert attrs["Expression"] == attrs["Hits"]
        counts = [int(x) for x in attrs["Expression"].split(",")]
        assert len(counts) == len(case.samples)
        # (the name as printed: the golden cases do not keep the frame's NAME column, so what gff_names does to a ``.SNP``
        # suffix and to a ``-3p`` / ``-5p`` name without annotation is pinned only in tests/test_gff_device_gpu.py, on hand-made
        # names and against gff.resolve_names, not against the reference)
        printed, master, parent, precursor = oracle.gff_names(f[0], mat, pre_of, pre)
        assert printed == f[0]
        assert oracle.gff_line(printed, source, master, attrs["Read"], precursor, parent, counts) == ln, (f[0], attrs["Read"])
        n += 1
        n_with_n += "N" in attrs["Read"]
        prefixes.add(attrs["UID"][:3])
    assert n > 650 and n_with_n > 0 and prefixes == {"ref", "iso", "."}
    # a row whose name resolves to nothing has no line
    assert oracle.gff_names("no-such-miR-3p", mat, pre_of, pre) is None
    assert oracle.gff_line("no-such-miR", source, None, "ACGT", None, None, [1]) is None


@pytest.mark.parametrize("case_name", GFF_A2I_CASES)
def test_gff_uid_restatement_equals_the_reference_function(case_name):
    d = json.load(open(os.path.join(GOLDEN, case_name, "a2i_direct.json")))
    assert len(d["uid"]) >= 7
    for seq, prefix, uid in d["uid"]:
        assert oracle.gff_uid(seq, prefix) == uid, seq


def test_host_uid_rule_equals_the_restatement_on_every_last_stretch(tmp_path):
    """uid_append on all 4 + 16 + 64 + 256 + 1024 strings of 1..5 bases, alone and behind one full stretch: one exact
    (kind = 1) row per string through mirge_gff_write, the UID field of every line against oracle.gff_uid"""
    import mirge3_amd  # noqa: F401
    from mirge3_amd import _ffi, gff
    from mirge3_amd.seqio import FlatSeqs
    tails = ["".join(t) for k in range(1, 6) for t in itertools.product("ACGT", repeat=k)]
    assert len(tails) == 4 + 16 + 64 + 256 + 1024
    reads = tails + ["GATCA" + t for t in tails]
    n = len(reads)
    recs = np.zeros(n, dtype=gff.RECORD)
    recs["kind"], recs["start"], recs["vlen"] = 1, 1, 2
    for k, r in enumerate(reads):
        cigar = f"{len(r)}M".encode()
        recs["end"][k], recs["clen"][k], recs["text"][k] = len(r), len(cigar), b"NA" + cigar
    seqs, names, parents = FlatSeqs.from_list(reads), FlatSeqs.from_list(["miR-x"]), FlatSeqs.from_list(["mir-x"])
    counts = np.arange(1, n + 1, dtype=np.uint32).reshape(n, 1)
    zero = np.zeros(n, dtype=np.int32)
    path = tmp_path / "uid.gff"
    p = lambda a: C.c_void_p(a.ctypes.data)  # hand-wrapped, as an outside caller of _ffi.load() would: passes the binding unchecked
    _ffi._check(_ffi.load().mirge_gff_write(
        str(path).encode(), b"# head\n", b"miRBase22", p(recs), C.c_int64(n), p(np.ascontiguousarray(seqs.data)),
        p(np.ascontiguousarray(seqs.offsets, dtype=np.int64)), p(counts), C.c_int32(1), p(zero), p(np.ascontiguousarray(names.data)),
        p(np.ascontiguousarray(names.offsets, dtype=np.int64)), C.c_int64(1), p(zero), p(np.ascontiguousarray(parents.data)),
        p(np.ascontiguousarray(parents.offsets, dtype=np.int64)), C.c_int64(1), C.c_void_p(0), C.c_int64(n)), "mirge_gff_write")
    lines = path.read_text().splitlines(keepends=True)
    assert lines[0] == "# head\n" and len(lines) == n + 1
    one_symbol = two_symbols = 0
    for k, (r, ln) in enumerate(zip(reads, lines[1:])):
        want = oracle.gff_uid(r, "ref")
        assert ln.split("; UID=")[1].split(";")[0] == want, r
        # ... and the whole line: these rows are their own canonical at the start of a precursor that is the read itself
        assert ln == oracle.gff_line("miR-x", "miRBase22", r, r, r, "mir-x", [k + 1]), r
        if len(r) < 5:
            one_symbol += len(want.split("-")[2]) == 1
            two_symbols += len(want.split("-")[2]) == 2
    assert one_symbol == 4 + 16 + 12 and two_symbols == 52 + 256  # numbers 0..31 take one symbol, 32..339 two

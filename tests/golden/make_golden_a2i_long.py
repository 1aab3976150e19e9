#!/usr/bin/env python3
"""Generate tests/golden/a2i_long_direct.json: the REFERENCE's own ``align2TargetSeq`` / ``judgeAllign``, ``A2IEditing`` and
``mismatchCountAnalysis`` (mirge2_tRF_a2i.py:246-518) on canonical sequences of 26..32 nt and reads of up to 35 nt -- the lengths
that tests/golden/case*_gff_a2i/a2i_direct.json (make_golden.py, targets of 18..25 nt) does not reach: the top of the packed
64-bit target, overlaps of 32 bases, census columns 21..26 and reads of two packed words.

Runs only where /root/reference exists (never on the GPU box, never from a test); what is committed is data, in the schema of
a2i_direct.json.  Recipe as in make_golden.py: the stand-ins of tests/golden/stubs at import time, ``Bio.pairwise2`` among them, and
only (target, read) pairs whose best score lies on ONE diagonal, so that the stand-in's tie rule decides nothing.

The targets are made here: 8 per length 26..32.  Per target, reads of Lt-4 .. Lt+3 nt that start at target base -1 .. +2, with
0..3 substitutions, planted A -> G (one of them as far towards the census limit Lt - 6 as the target allows) and a `retained` subset.
The script asserts that the file holds what it is made for before it writes.

usage: python tests/golden/make_golden_a2i_long.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "stubs"))
sys.path.insert(1, "/root/reference")

import numpy as np  # noqa: E402

from Bio import pairwise2 as standin  # noqa: E402
from mirge.libs import mirge2_tRF_a2i as ref_a2i  # noqa: E402  (the reference)

OUT = os.path.join(HERE, "a2i_long_direct.json")
LENGTHS = range(26, 33)
PER_LENGTH = 8


def rnd(rng, n):
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=n))


def sub(seq, pos, to):
    return seq[:pos] + to + seq[pos + 1:]


def one_diagonal(target, read):
    return len(standin.align.diagonals_at_best(target, read, 2, -1, -20, -20)) == 1


def make_target(rng, L):
    """random, with an A in the last five census columns (Lt - 10 .. Lt - 6) and no base run a read could slide along"""
    while True:
        t = rnd(rng, L)
        if "A" in t[L - 10:L - 5] and all(t[k:k + 4] != t[k] * 4 for k in range(L - 3)):
            return t


def make_read(rng, target, d5, length, n_sub, a2g):
    """the read that starts at target base d5 (d5 < 0: -d5 bases of its own first) and is `length` nt long"""
    L = len(target)
    body = target[max(d5, 0):]
    q = rnd(rng, max(-d5, 0)) + body
    q = q[:length] + rnd(rng, max(0, length - len(q)))
    for _ in range(n_sub):
        p = int(rng.integers(0, len(q)))
        q = sub(q, p, "ACGT"[int(rng.integers(0, 4))])
    if a2g is not None:  # target base a2g (an A) read as G
        j = a2g - d5
        if 0 <= j < len(q):
            q = sub(q, j, "G")
    return q


def main():
    rng = np.random.Generator(np.random.PCG64(2632))
    groups = []
    for L in LENGTHS:
        for k in range(PER_LENGTH):
            target = make_target(rng, L)
            a_all = [q for q in range(L - 5) if target[q] == "A"]
            a_high = max(a_all)
            reads, counts = [], []
            # the corners first: the longest read at every 5' offset and the shortest at an outer one, then random ones
            plan = [(d5, L + 3, 0, None) for d5 in (-1, 0, 1, 2)] + [(2 if k % 2 else -1, L - 4, 0, None)]
            plan += [(int(rng.integers(-1, 3)), L + int(rng.integers(1, 4)), 1, a_high), (0, L + 3, 0, a_high)]
            for _ in range(int(rng.integers(1, 4))):
                plan.append((int(rng.integers(-1, 3)), L + int(rng.integers(-4, 4)), int(rng.choice([0, 0, 1, 1, 2, 3])),
                             a_all[int(rng.integers(0, len(a_all)))] if rng.random() < 0.4 else None))
            for d5, length, n_sub, a2g in plan:
                q = make_read(rng, target, d5, length, n_sub, a2g)
                assert L - 4 <= len(q) <= L + 3
                if q in reads or not one_diagonal(target, q):
                    continue
                reads.append(q); counts.append(int(rng.integers(1, 500)))
            assert len(reads) >= 6, (target, len(reads))
            retained = {q: True for q in reads if rng.random() < 0.7}
            aligned, states = ref_a2i.align2TargetSeq(target, reads)
            with open(os.devnull, "w") as devnull:
                kept, plist, pcount, pratio, ppval, count_true, seq_true, canon = ref_a2i.A2IEditing(
                    target, reads, counts, "x", devnull, retained, 'A', 'G')
            mm = ref_a2i.mismatchCountAnalysis(target, reads, counts, retained)
            groups.append(dict(target=target, reads=reads, counts=counts, retained=sorted(retained),
                               aligned=aligned, states=[bool(x) for x in states],
                               a2i=dict(kept=kept, positions=plist, count={str(k): v for k, v in pcount.items()},
                                        ratio={str(k): v for k, v in pratio.items()},
                                        pvalue={str(k): float(v) for k, v in ppval.items()}, countSumTrue=count_true,
                                        seqCountTrue=seq_true, canonicalSeqCount=canon),
                               mismatch_census=[list(t) for t in mm]))
    # ---- the file holds what it is made for
    assert len(groups) >= 50
    for L in LENGTHS:
        assert sum(len(g["target"]) == L for g in groups) >= 6
    long_states = [s for g in groups for q, s in zip(g["reads"], g["states"]) if len(q) >= 32]
    assert len(long_states) >= 40 and True in long_states and False in long_states, (len(long_states), set(long_states))
    assert {len(q) for g in groups for q in g["reads"]} >= set(range(22, 36))
    assert max(p for g in groups for p in g["a2i"]["positions"]) - 1 >= 22  # (positions are 1-based)
    with open(OUT, "w") as fh:
        json.dump(dict(note="outputs of the reference's align2TargetSeq/judgeAllign, A2IEditing, mismatchCountAnalysis "
                            "(mirge2_tRF_a2i.py:246-518) on targets of 26..32 nt and reads of up to 35 nt; pairwise2 = tests/golden/stubs "
                            "stand-in, only pairs whose best score lies on one diagonal; made by tests/golden/make_golden_a2i_long.py",
                       groups=groups), fh, indent=0)
    print(len(groups), "groups,", sum(len(g["reads"]) for g in groups), "reads,", len(long_states), "of 32 nt and more (",
          sum(long_states), "accepted ),", os.path.getsize(OUT), "bytes ->", OUT)


if __name__ == "__main__":
    main()

"""The tRNA fragment kernels on the CPU: ``csrc/kernels_trf.hpp`` itself compiled for the host (tests/hostsim/trf_sim.cpp) against a
brute-force enumeration of every window and against ``assign_cluster`` / ``getDistance2`` / ``trfTypes`` restated here from the
reference (mirge2_tRF_a2i.py:22-79, summary.py:649-674).  The helpers below are shared with the GPU tests (tests/test_trf_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "trf_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libtrfsim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")
TYPES = ("tRF-whole", "5'-half", "5'-tRF", "3'-half", "3'-tRF", "i-tRF", "tRF-1")
MATURE_PASS, PRIMARY_PASS = 2, 3
MATURE_POL = dict(mode=1, mm=1, seedlen=28, maxtotal=1)
PRIMARY_POL = dict(mode=1, mm=0, seedlen=28, maxtotal=0, ttail=1)


# ---- restatements of the reference
def trf_type(L, pre, start, tlen, ac):
    """trfTypes (summary.py:649-674); ``ac`` = 0-based anticodon start"""
    if pre:
        return "tRF-1"
    if start == 0:
        if start + L == tlen:
            return "tRF-whole"
        if ac - 2 <= start + L - 1 <= ac + 1:
            return "5'-half"
        return "5'-tRF"
    if tlen - 1 - 2 <= start + L - 1 <= tlen - 1:
        return "3'-half" if ac - 1 <= start <= ac + 2 else "3'-tRF"
    return "i-tRF"


def add_dash(seq, total, start, end):
    return "-" * (start - 1) + seq + "-" * (total - end)


def coordinate(d):
    return len(d) - len(d.lstrip("-")) + 1, len(d.rstrip("-"))


def distance2(s1, s2):
    sub = 0
    for k in range(len(s1)):
        try:
            if s1[k] != "-" and s2[k] != "-" and s1[k] != s2[k]:
                sub += 1
        except IndexError:
            sub += 1
    c1, c2 = coordinate(s1), coordinate(s2)
    return abs(c1[0] - c2[0]) + abs(c1[1] - c2[1]) + sub


def assign_cluster(dashed, trfs):
    """``trfs``: {dashed string: cluster name} of the row's tRNA, or None -> (distance, nearest cluster name or None)"""
    if trfs is None:
        return 100, None
    dl = sorted((distance2(dashed, s), name) for s, name in trfs.items())
    return dl[0]


# ---- brute force: every window of a concatenated library
class Text:
    def __init__(self, refs):
        self.refs = list(refs)
        self.start = np.zeros(len(self.refs) + 1, dtype=np.int64)
        np.cumsum([len(r) + 1 for r in self.refs], out=self.start[1:])
        self.t = np.frombuffer(("#".join(self.refs) + "#").upper().replace("U", "T").encode(), dtype=np.uint8)
        bad = ~np.isin(self.t, np.frombuffer(b"ACGT", dtype=np.uint8))
        self.badsum = np.concatenate([[0], np.cumsum(bad)])

    def windows(self, read, max_mm, cand=None):
        """[(global position, mismatches)] of every window without an invalid base and at most ``max_mm`` mismatches; N in the read
        is a mismatch.  ``cand``: only these positions are looked at (an exact prefilter, see ``prefilter``)"""
        L, n = len(read), self.t.shape[0]
        if n < L:
            return []
        s = np.frombuffer(read.encode(), dtype=np.uint8)
        pos = np.arange(n - L + 1) if cand is None else np.asarray([p for p in cand if 0 <= p <= n - L], dtype=np.int64)
        if pos.size == 0:
            return []
        mm = np.zeros(pos.shape[0], dtype=np.int32)
        for i in range(L):
            mm += self.t[pos + i] != s[i]
        ok = (self.badsum[pos + L] - self.badsum[pos] == 0) & (mm <= max_mm)
        return [(int(p), int(m)) for p, m in zip(pos[ok], mm[ok])]

    def where(self, g):
        r = int(np.searchsorted(self.start, g, side="right")) - 1
        return r, g - int(self.start[r])

    def prefilter(self):
        """positions by the 8-mer that starts there, for ``candidates``"""
        code = np.full(256, 255, dtype=np.uint32)
        for k, ch in enumerate(b"ACGT"):
            code[ch] = k
        c = code[self.t]
        n = c.shape[0] - 7
        h = np.zeros(n, dtype=np.uint32)
        badw = np.zeros(n, dtype=bool)
        for i in range(8):
            h |= (c[i:i + n] & 3) << (2 * i)
            badw |= c[i:i + n] == 255
        h[badw] = 0xFFFFFFFF
        order = np.argsort(h, kind="stable")
        self._h_sorted, self._h_order = h[order], order

    def candidates(self, read):
        """a superset of the windows with at most one mismatch of a read of 16 nt or more: its first or its second 8 bases are exact"""
        out = set()
        for a in (0, 8):
            blk = read[a:a + 8]
            if "N" in blk:
                continue
            key = sum("ACGT".index(ch) << (2 * i) for i, ch in enumerate(blk))
            lo, hi = np.searchsorted(self._h_sorted, key, side="left"), np.searchsorted(self._h_sorted, key, side="right")
            out.update(int(p) - a for p in self._h_order[lo:hi])
        return sorted(out)


def classify(reads, mature, primary, fast=False):
    """what the cascade's passes 2 and 3 answer, by brute force -> (pass int8, mm int8, {read index: [(ref, off)]} in library order)"""
    ps, mm, hits = np.full(len(reads), -1, np.int8), np.full(len(reads), -1, np.int8), {}
    for i, rd in enumerate(reads):
        w = mature.windows(rd, 1, mature.candidates(rd) if fast else None)
        if w:
            best = min(m for _, m in w)
            ps[i], mm[i] = MATURE_PASS, best
            hits[i] = sorted(mature.where(g) for g, m in w if m == best)
            continue
        m = re.search("T{3,}$", rd)
        if m and m.start() > 0:
            head = rd[:m.start()]
            w = primary.windows(head, 0, primary.candidates(head) if fast and len(head) >= 16 else None)
            if w:
                ps[i], mm[i] = PRIMARY_PASS, 0
                hits[i] = sorted(primary.where(g) for g, _ in w)
    return ps, mm, hits


def expected_records(reads, rows, ps, mm, hits, mature, anticodon):
    out = []
    for k, i in enumerate(rows):
        for ref, off in hits[i]:
            pre = ps[i] == PRIMARY_PASS
            ty = trf_type(len(reads[i]), pre, off, 0 if pre else len(mature.refs[ref]), 0 if pre else anticodon[ref])
            out.append((k, ref, off, int(mm[i]), 1 if pre else 0, TYPES.index(ty)))
    return out


# ---- a small synthetic tRNA library with the traps the kernels can fall into
def synth_case(seed=3, n_random=260):
    rng = np.random.default_rng(seed)
    rnd = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, n))
    mature = [rnd(int(L)) for L in rng.integers(70, 96, 10)]
    mature.append(mature[0])                                          # the same sequence under another name
    v = list(mature[1]); v[33] = "ACGT"[("ACGT".index(v[33]) + 1) % 4]
    mature.append("".join(v))                                         # one base apart
    rep = rnd(20)
    mature.append(rnd(12) + rep + rnd(9) + rep + rnd(14))             # a 20-mer twice
    mature.append(rnd(30) + "N" + rnd(44))                            # a reference N
    mature.append(mature[2][:40] + rnd(35))                           # a shared 5' half
    anticodon = [int(rng.integers(30, 38)) for _ in mature]
    primary = [rnd(int(rng.integers(3, 9))) + m.replace("N", "A") + rnd(int(rng.integers(4, 12))) + "TTTT" for m in mature[:8]]
    primary.append(primary[0])
    reads = []
    mut = lambda s, p: s[:p] + "ACGT"[("ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4] + s[p + 1:]
    for m in mature:
        reads += [m, m[:int(rng.integers(16, 40))], m[-int(rng.integers(16, 40)):]]
    for r, m in enumerate(mature):                                    # the four boundary values of each half test, and one beyond
        if "N" in m:
            continue
        ac = anticodon[r]
        reads += [m[:e + 1] for e in range(ac - 3, ac + 3)]
        reads += [m[s:] for s in range(ac - 2, ac + 4)] + [m[s:len(m) - d] for s in (ac, 5) for d in (1, 2, 3)]
    base = mature[3]
    reads += [mut(base[:31], p) for p in range(31)]                   # the single mismatch in every place of a one-word read
    reads += [mut(base[:64], p) for p in range(0, 64, 3)] + [mut(base, p) for p in range(0, len(base), 5)]
    reads += [base[:20] + "N" + base[21:40], "N" + base[1:30], base[10:41][:-1] + "N", base[:8] + "N" + base[9:20] + "N" + base[21:33]]
    reads += [rep, rep + mature[12][32:41], mature[12][:32]]          # two windows on one reference
    cat = "".join(mature)
    reads += [cat[len(mature[0]) - 10:len(mature[0]) + 12], mature[0][-12:] + mature[1][:10]]  # would straddle two references
    for r, p in enumerate(primary):
        body = p[:-4]
        reads += [body[-20:] + "TTT", body[-25:] + "TTTTT", body[5:40] + "TTT", body[-18:] + "TTTTTTT", p[-30:]]
    for _ in range(n_random):
        src = mature[int(rng.integers(0, len(mature)))]
        L = int(rng.integers(16, min(96, len(src) + 1)))
        o = int(rng.integers(0, len(src) - L + 1))
        s = src[o:o + L].replace("N", "A")
        k = int(rng.integers(0, 4))
        reads.append(s if k == 0 else (mut(s, int(rng.integers(0, L))) if k < 3 else mut(mut(s, 2), L - 3)))
    reads += [rnd(int(L)) for L in rng.integers(16, 96, 30)]
    reads = list(dict.fromkeys(reads))                                # unique, as a collapse result
    return mature, primary, anticodon, reads


# ---- the simulation
def _pol(kw):
    from_fields = ("mode", "mm", "seedlen", "maxtotal", "trim5", "trim3", "ttail", "len_lt", "len_gt", "reserved")
    return [int(kw.get(f, 0)) for f in from_fields]


@pytest.fixture(scope="module")
def sim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("kernels_trf.hpp", "mirge_core.hpp", "mirge_libbuild.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-pthread", "-o", SO, SRC])
    lib = C.CDLL(SO)
    lib.sim_trf_hits.restype = C.c_longlong
    return lib


def _flat(strs):
    off = np.zeros(len(strs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strs], out=off[1:])
    return np.frombuffer(("".join(strs) or "\0").encode(), dtype=np.uint8).copy(), off


@pytest.fixture(scope="module")
def case():
    mature, primary, anticodon, reads = synth_case()
    tm, tp = Text(mature), Text(primary)
    ps, mm, hits = classify(reads, tm, tp)
    return dict(mature=mature, primary=primary, anticodon=anticodon, reads=reads, tm=tm, tp=tp, ps=ps, mm=mm, hits=hits)


def run_sim_hits(sim, case, rows, entries_all):
    rd, roff = _flat(case["reads"])
    libs = [_flat(case["mature"]), _flat(case["primary"])]
    seqs = (C.c_void_p * 2)(*[d.ctypes.data for d, _ in libs])
    offs = (C.c_void_p * 2)(*[o.ctypes.data for _, o in libs])
    ns = (C.c_int64 * 2)(len(case["mature"]), len(case["primary"]))
    pol = np.asarray([_pol(MATURE_POL), _pol(PRIMARY_POL)], dtype=np.int32)
    cls_pass = (C.c_int32 * 2)(MATURE_PASS, PRIMARY_PASS)
    ac = np.asarray(case["anticodon"], dtype=np.int32)
    rows = np.asarray(rows, dtype=np.int64)
    cap = 1 << 16
    o = dict(row=np.zeros(cap, np.uint32), ref=np.zeros(cap, np.uint32), off=np.zeros(cap, np.int32), mm=np.zeros(cap, np.uint8),
             cls=np.zeros(cap, np.uint8), type=np.zeros(cap, np.uint8))
    p = lambda a: C.c_void_p(a.ctypes.data)
    n = sim.sim_trf_hits(p(rd), p(roff), C.c_int64(len(case["reads"])), p(case["ps"]), p(case["mm"]), seqs, offs, ns, p(pol), cls_pass,
                         p(ac), p(rows), C.c_int64(rows.shape[0]), C.c_int32(1 if entries_all else 0), C.c_longlong(cap),
                         *(p(o[k]) for k in ("row", "ref", "off", "mm", "cls", "type")))
    assert n >= 0, n
    return [tuple(int(o[k][i]) for k in ("row", "ref", "off", "mm", "cls", "type")) for i in range(n)]


def test_case_holds_what_it_is_for(case):
    """the synthetic library and reads exercise what the issue lists"""
    ps, mm, hits, reads = case["ps"], case["mm"], case["hits"], case["reads"]
    assert (ps == MATURE_PASS).sum() > 200 and (ps == PRIMARY_PASS).sum() > 10 and (ps < 0).sum() > 10
    assert any(len(reads[i]) <= 31 for i in hits) and any(32 <= len(reads[i]) <= 64 for i in hits) and any(len(reads[i]) > 64 for i in hits)
    assert any(mm[i] == 1 and "N" in reads[i] for i in hits)
    assert any(len(h) > 1 and len({r for r, _ in h}) == 1 for h in hits.values())     # two windows on one reference
    assert any(len({r for r, _ in h}) > 1 for h in hits.values())                     # several references
    rows = sorted(hits)
    recs = expected_records(reads, rows, ps, mm, hits, case["tm"], case["anticodon"])
    assert {r[5] for r in recs} == set(range(7))                                      # every trfTypes branch
    assert any(off == 0 for _, _, off, _, _, _ in recs)
    assert any(c == 0 and off + len(reads[rows[k]]) == len(case["mature"][ref]) for k, ref, off, _, c, _ in recs)


@pytest.mark.parametrize("entries_all", [False, True], ids=["bitmap-csr", "entries"])
def test_hits_equal_brute_force(sim, case, entries_all):
    rows = sorted(case["hits"])
    rng = np.random.default_rng(1)
    rng.shuffle(rows)  # (mapped.csv's order is not the handle's)
    got = run_sim_hits(sim, case, rows, entries_all)
    want = expected_records(case["reads"], rows, case["ps"], case["mm"], case["hits"], case["tm"], case["anticodon"])
    assert got == want  # as sorted lists: a duplicate or a miss shows


def test_hits_refuse_a_row_of_another_class(sim, case):
    other = int(np.nonzero(case["ps"] < 0)[0][0])
    rd, roff = _flat(case["reads"])
    with pytest.raises(AssertionError):
        run_sim_hits(sim, case, [other], False)


def test_prefilter_is_exact(case):
    """the 8-mer prefilter the GPU test's brute force uses on its large library finds what the plain enumeration finds"""
    tm, tp = Text(case["mature"]), Text(case["primary"])
    tm.prefilter(); tp.prefilter()
    ps, mm, hits = classify(case["reads"], tm, tp, fast=True)
    assert np.array_equal(ps, case["ps"]) and np.array_equal(mm, case["mm"]) and hits == case["hits"]


# ---- assignment
def synth_infor(mature, seed=5):
    """predefined tRFs per reference: {ref index: {dashed string: cluster name}}; references 1 and 4 have none"""
    rng = np.random.default_rng(seed)
    infor = {}
    for r, m in enumerate(mature):
        if r in (1, 4):
            continue
        d = {}
        n = int(rng.integers(1, 41)) if r != 0 else 40
        for k in range(n):
            L = int(rng.integers(14, 45))
            s = int(rng.integers(1, len(m) - L + 2))
            seq = m[s - 1:s - 1 + L].replace("N", "A")
            if k % 5 == 0:  # a sequence that differs from the library's in a base
                p = int(rng.integers(0, L))
                seq = seq[:p] + "ACGT"[("ACGT".index(seq[p]) + 1) % 4] + seq[p + 1:]
            total = len(m) - (int(rng.integers(1, 30)) if k % 4 == 0 else 0)  # a sequence column shorter than the tRNA
            d[add_dash(seq, total, s, s + L - 1)] = "tRNA%d_Cluster%d" % (r, int(rng.integers(0, 1000)))
        infor[r] = d
    return infor


def infor_tables(infor, n_refs):
    """the CSR ``mirge_trf_assign`` takes"""
    ref_ptr, strings, names = [0], [], []
    tref = np.full(n_refs, -1, dtype=np.int32)
    for k, r in enumerate(sorted(infor)):
        tref[r] = k
        for s, name in infor[r].items():
            strings.append(s.encode()); names.append(name)
        ref_ptr.append(len(strings))
    rank_of = {nm: i for i, nm in enumerate(sorted(set(names)))}
    cs, ce = zip(*(coordinate(s.decode()) for s in strings))
    return tref, np.asarray(ref_ptr, np.int64), strings, names, np.asarray(cs, np.int32), np.asarray(ce, np.int32), \
        np.asarray([rank_of[nm] for nm in names], np.int32)


def assign_rows(case, infor, n=500, seed=8):
    """rows (read index, reference, 1-based start) from the hits, plus displaced ones so that distances spread around the cutoff"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in sorted(case["hits"]):
        if case["ps"][i] != MATURE_PASS:
            continue
        for ref, off in case["hits"][i]:
            rows.append((i, ref, off + 1))
            rows.append((i, ref, max(1, off + 1 + int(rng.integers(-6, 7)))))
    rng.shuffle(rows)
    return rows[:n]


def expected_assign(case, infor, rows):
    out = []
    for i, ref, start in rows:
        rd, tlen = case["reads"][i], len(case["mature"][ref])
        dashed = add_dash(rd, tlen, start, start + len(rd) - 1)
        d, name = assign_cluster(dashed, infor.get(ref))
        out.append((d, name))
    return out


def test_assign_equals_the_restatement(sim, case):
    infor = synth_infor(case["mature"])
    tref, ref_ptr, strings, names, cs, ce, rank = infor_tables(infor, len(case["mature"]))
    rows = assign_rows(case, infor)
    want = expected_assign(case, infor, rows)
    assert any(d == 8 for d, _ in want) and any(d == 9 for d, _ in want) and any(n is None for _, n in want)
    assert any(len(s) < len(case["mature"][r]) for r in infor for s in infor[r])  # unequal string lengths
    rd, roff = _flat(case["reads"])
    read = np.asarray([r[0] for r in rows], np.int64)
    tr = tref[[r[1] for r in rows]].astype(np.int32)
    start = np.asarray([r[2] for r in rows], np.int32)
    soff = np.zeros(len(strings) + 1, np.uint32)
    np.cumsum([len(s) for s in strings], out=soff[1:])
    blob = np.frombuffer(b"".join(strings), np.uint8).copy()
    dist, trf = np.zeros(len(rows), np.int32), np.zeros(len(rows), np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    ptr = ref_ptr.astype(np.uint32)
    rc = sim.sim_trf_assign(p(rd), p(roff), C.c_int64(len(case["reads"])), C.c_int64(len(rows)), p(read), p(tr), p(start),
                            C.c_int64(ref_ptr.shape[0] - 1), p(ptr), C.c_int64(len(strings)), p(soff), p(blob),
                            p(cs), p(ce), p(rank), p(dist), p(trf))
    assert rc == 0
    got = [(int(d), names[t] if t >= 0 else None) for d, t in zip(dist, trf)]
    assert got == want


def test_assign_ties_go_to_the_name_first_in_string_order(sim):
    """two tRFs at the same distance: Python's tuple sort takes the cluster name that sorts first, whichever line came first"""
    m = "ACGTTGCAAGGCTTACGGATCCATGACCTGAAGTCCATTGCAGTCAAGGT"
    read = m[10:30]
    for names in (("x_Cluster9", "x_Cluster10"), ("x_Cluster10", "x_Cluster9")):
        infor = {0: {add_dash(m[8:30], len(m), 9, 30): names[0], add_dash(m[10:32], len(m), 11, 32): names[1]}}
        want = assign_cluster(add_dash(read, len(m), 11, 30), infor[0])
        assert want == (2, "x_Cluster10")
        tref, ref_ptr, strings, nm, cs, ce, rank = infor_tables(infor, 1)
        rd, roff = _flat([read])
        soff = np.zeros(3, np.uint32)
        np.cumsum([len(s) for s in strings], out=soff[1:])
        blob = np.frombuffer(b"".join(strings), np.uint8).copy()
        dist, trf = np.zeros(1, np.int32), np.zeros(1, np.int32)
        p = lambda a: C.c_void_p(a.ctypes.data)
        row, tr, start, ptr = np.zeros(1, np.int64), np.zeros(1, np.int32), np.asarray([11], np.int32), ref_ptr.astype(np.uint32)
        rc = sim.sim_trf_assign(p(rd), p(roff), C.c_int64(1), C.c_int64(1), p(row), p(tr), p(start), C.c_int64(1), p(ptr), C.c_int64(2),
                                p(soff), p(blob), p(cs), p(ce), p(rank), p(dist), p(trf))
        assert rc == 0 and (int(dist[0]), nm[int(trf[0])]) == want

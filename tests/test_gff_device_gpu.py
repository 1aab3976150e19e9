"""The miRTop GFF3 formatted on the device (mirge_gff_write_device: k_gff_select, k_gff_rows, k_isotype, k_gff_line, the chunked
copy and its writer threads) against the host route (records to the host, mirge_gff_write) and against the oracle's restatement
of a line (oracle.gff_line, pinned on the reference's own file in tests/test_gff_line_oracle.py).

Two cases.  A hand-made library and read set that holds every edge of k_gff_line by construction: reads of 16-47 nt in both
width groups, every residue of the length modulo 5 in each, an N before and behind the word boundary, counts of one to six
digits with zeros among them, names without a line in the middle of the file, row orders that are not the identity, canonicals
beyond k_isotype's register form and beyond 40 nt.  And a synthetic sample whose text is just long enough for three 8 MiB chunks."""
import functools

import numpy as np
import pytest

import oracle
from helpers import write_gff_name_files
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, gff, synth
from mirge3_amd.cascade import Cascade, EXACT_PASS, ISO_PASS
from mirge3_amd.seqio import FlatSeqs, Library

pytestmark = pytest.mark.gpu

SOURCE = "miRBase22"
CHUNK = 8 << 20  # CH of mirge_gff_write_device (csrc/native_iso.hpp)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- the directed case
COUNT_MENU = [0, 1, 9, 10, 99, 100, 999, 1000, 99_999, 100_000]


def _rnd(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def _other(rng, base):
    return [b for b in "ACGT" if b != base][int(rng.integers(0, 3))]


@functools.lru_cache(maxsize=None)
def directed_case():
    """-> dict: the miRNA and hairpin libraries, the name tables as the reference reads them, the unique reads with the miRNA
    each was made from, and their counts in three samples.  Pure host work, seeded."""
    rng = np.random.default_rng(20261018)
    # (name in the library, canonical length, what is special about it)
    spec = [(f"hsa-miR-{L}-5p", L, "") for L in range(18, 41)]                    # every canonical length 18..40
    spec += [("hsa-miR-41-5p", 41, ""), ("hsa-miR-44-3p", 44, "")]                # beyond 40 nt: rows that went untyped, and so without a line, while MIRGE_ISO_MAXA was 40
    spec += [("hsa-miR-first-5p", 23, "start"), ("hsa-miR-firstlong-5p", 34, "start")]  # at the precursor's first base: start0 = 1
    spec += [("hsa-miR-orphan-5p", 22, "orphan"), ("hsa-miR-orphanlong-3p", 35, "orphan")]  # no annotation: no line
    spec += [("hsa-miR-stem-3p", 21, "stem")]                                     # only 'hsa-miR-stem' is annotated
    spec += [("hsa-miR-var-5p.SNP", 24, "snp")]                                   # printed without the suffix
    spec += [(f"hsa-miR-b{L}-3p", L, "") for L in (30, 31, 32, 33, 34, 38, 25, 26, 36)]
    names, lib_seqs, sources, offs, hp_names, hp_seqs = [], [], [], [], [], []
    mirDict, pre_of = {}, {}
    for k, (nm, L, what) in enumerate(spec):
        master = _rnd(rng, L)
        f5 = "" if what == "start" else _rnd(rng, int(rng.integers(20, 31)))
        pre = f5 + master + _rnd(rng, int(rng.integers(20, 31)))
        lib_seq = master
        if what == "snp":  # the library holds the variant, the mature FASTA and the precursor the canonical
            lib_seq = master[:11] + _other(rng, master[11]) + master[12:]
        printed = nm.split(".")[0]
        printed = printed[:-3] if what == "stem" else printed
        mirDict[printed] = master
        if what != "orphan":
            pre_of[printed] = f"hsa-mir-h{k}"
        names.append(nm); lib_seqs.append(lib_seq); offs.append(len(f5))
        sources.append(f5 + lib_seq + pre[len(f5) + L:])  # what this miRNA's templated reads are cut from
        hp_names.append(f"hsa-mir-h{k}"); hp_seqs.append(pre)

    def hairpin_takes(r, src, s):
        # pass 1 of the cascade (-n 1, reads of 26 nt and more): at most 1 mismatch in the first 28 bases and 2 in all
        mm = [r[i] != src[s + i] for i in range(len(r))]
        return len(r) > 25 and sum(mm[:28]) <= 1 and sum(mm) <= 2

    reads = {}  # read -> miRNA index
    what_of = [what for _, _, what in spec]

    def put(m, r, s):
        """read r made from miRNA m, cut from sources[m] at s.  A read of 26 nt and more that the hairpin pass would take
        never reaches the isomiR pass (cascade.PASSES: passes 1 and 8): its first base, which the isomiR pass trims
        (-5 1), is replaced, and one base of the first 28 substituted, until the hairpin pass lets it go.  So every row of
        26 nt and more is an isomiR with two substitutions at least: ``ref-`` UIDs occur only in the one-word group, by construction
        (the exact pass stops below 26 nt, so the cascade has no exact miRNA row of more than 31 nt to give)."""
        src, o, lc = sources[m], offs[m], len(lib_seqs[m])
        r = list(r)
        if hairpin_takes(r, src, s):
            r[0] = _other(rng, src[s]) if r[0] == src[s] else r[0]
        while hairpin_takes(r, src, s):
            q = int(rng.integers(1, min(28, len(r) - 2)))
            if r[q] == src[s + q]:
                r[q] = _other(rng, r[q])
        r = "".join(r)
        # the isomiR pass (-5 1 -3 2 -v 2): the read without its first and its last two bases lies inside the miRNA, 2 mismatches
        assert s + 1 >= o and s + len(r) - 2 <= o + lc, (names[m], r)
        if sum(r[i] != src[s + i] for i in range(1, len(r) - 2)) <= 2 and 16 <= len(r) <= 47:
            reads.setdefault(r, m)

    for m in range(len(spec)):
        src, o, lc = sources[m], offs[m], len(lib_seqs[m])
        for e5 in (1, 0, -1, -2):            # 5' end: one templated base more .. two fewer
            for e3 in (-3, -2, -1, 0, 1, 2):  # 3' end
                s, e = o - e5, o + lc + e3
                if s < 0 or e - s < 16:       # (a canonical at its precursor's first base has no templated 5' extension)
                    continue
                t = src[s:e]
                put(m, t, s)
                if e3 in (-2, 0, 2):          # one substitution
                    q = int(rng.integers(1, len(t) - 2))
                    put(m, t[:q] + _other(rng, t[q]) + t[q + 1:], s)
                if e3 == 0:                   # non-templated 3' additions of one and two bases
                    for k in (1, 2):
                        put(m, t + "".join(_other(rng, src[e + i]) for i in range(k)), s)
                    if what_of[m] == "start" and e5 == 0:  # ... and a 5' addition where the precursor has nothing in front
                        reads.setdefault(_rnd(rng, 1) + t, m)
                if e3 in (-1, 1):             # one N: below base 32, and once more at base 32 or later where the read has one
                    q = int(rng.integers(1, min(len(t) - 2, 28)))
                    put(m, t[:q] + "N" + t[q + 1:], s)
                    if len(t) > 32:
                        q = int(rng.integers(32, len(t)))
                        put(m, t[:q] + "N" + t[q + 1:], s)
    # reads of 16..23 nt cut from inside the canonicals of 36 nt and more: the isomiR pass aligns a short read anywhere inside a
    # long canonical.  With a canonical of up to 40 nt they are pairs for k_isotype's register form (the two sequences share 64
    # positions), with a longer one for its array form alone (MIRGE_ISO_FAST_MAXA)
    rng_short = np.random.default_rng(41)
    for m in range(len(spec)):
        src, o, lc = sources[m], offs[m], len(lib_seqs[m])
        if lc < 36:
            continue
        for lb in (16, 18, 19, 20, 21, 22, 23):
            s = o + int(rng_short.integers(0, lc - lb + 1))
            t = src[s:s + lb]
            put(m, t, s)
            q = int(rng_short.integers(1, lb - 2))
            put(m, t[:q] + _other(rng_short, t[q]) + t[q + 1:], s)
    seqs = list(reads)
    U = len(seqs)
    # counts: every value of the menu in every sample; large ones are few, to keep the raw sample small
    counts = rng.choice(COUNT_MENU[:4], size=(U, 3), p=[0.3, 0.3, 0.2, 0.2]).astype(np.int64)
    cells = rng.permutation(U * 3)
    at = 0
    for v, how_many in ((99, 120), (100, 120), (999, 30), (1000, 30), (99_999, 5), (100_000, 5)):
        counts.reshape(-1)[cells[at:at + how_many]] = v
        at += how_many
    counts[counts.sum(axis=1) == 0, 1] = 1  # (a read no sample holds is no read)
    return dict(names=names, lib_seqs=lib_seqs, hp_names=hp_names, hp_seqs=hp_seqs, mirDict=mirDict, pre_of=pre_of,
                reads=seqs, made_from=np.array([reads[s] for s in seqs]), counts=counts)


def raw_sample(case, seed=7):
    """the unique reads repeated to their counts, sample by sample, and shuffled -> (raw reads, sample id per read)"""
    counts = case["counts"]
    U, S = counts.shape
    u = np.repeat(np.repeat(np.arange(U), S), counts.reshape(-1))
    sid = np.repeat(np.tile(np.arange(S), U), counts.reshape(-1))
    perm = np.random.default_rng(seed).permutation(u.shape[0])
    return FlatSeqs.from_list(case["reads"]).take(u[perm]), sid[perm].astype(np.int32)


@pytest.fixture(scope="module")
def directed(ctx, tmp_path_factory):
    case = directed_case()
    mir = Library(case["names"], FlatSeqs.from_list(case["lib_seqs"]))
    hp = Library(case["hp_names"], FlatSeqs.from_list(case["hp_seqs"]))
    casc = Cascade(ctx, {"mirna": mir, "hairpin": hp})
    args = write_gff_name_files(tmp_path_factory.mktemp("directed_libs"), case["mirDict"], case["pre_of"])
    pre = dict(zip(case["hp_names"], case["hp_seqs"]))
    pre[case["hp_names"][-1]] = ""  # the reference's parser leaves the last precursor of the index empty (summary.py:819-826)
    raw, sid = raw_sample(case)
    yield dict(case=case, casc=casc, args=args, pre=pre, raw=_ffi.DeviceReads.pack(ctx, raw), sid=sid)
    casc.close()


def _head(base_names):
    return ("# GFF3 adapted for miRNA sequencing data\n## VERSION 0.0.1\n## source-ontology: " + SOURCE + "\n## COLDATA: " +
            ",".join(base_names) + "\n")


def _both_routes(tmp_path, tag, args, base_names, casc, uniq, res, fetched, order):
    """the file by the device route and by the host route -> (device text, host text, lines the device call returned, the host
    route's records and their rows)"""
    seqs, ps, ref, counts = fetched
    (tmp_path / (tag + "_device")).mkdir()
    (tmp_path / (tag + "_host")).mkdir()
    d = gff.write_gff_device(args, tmp_path / (tag + "_device"), "miRBase", base_names, casc, uniq, res, order)
    h = gff.write_gff(args, tmp_path / (tag + "_host"), "miRBase", base_names, casc, uniq, res, seqs, ps, ref, counts, order)
    assert d["records"] is None
    return ((tmp_path / (tag + "_device") / "sample_miRge3.gff").read_bytes(), (tmp_path / (tag + "_host") / "sample_miRge3.gff").read_bytes(),
            d["lines"], h["records"], h["rows"])


def _file_rows(ps, order):
    """the file's rows: the exact-miRNA rows of the frame in frame order, then its isomiR rows (summary.py:50-60)"""
    po = ps[order]
    return np.concatenate([order[po == EXACT_PASS], order[po == ISO_PASS]]), int((po == EXACT_PASS).sum())


def _assert_same_lines(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (what, k, a, b)
    assert len(got) == len(want), (what, len(got), len(want))


def _directed_run(directed, tmp_path, S):
    case, casc, args, pre = directed["case"], directed["casc"], directed["args"], directed["pre"]
    base_names = [f"sample{s}" for s in range(S)]
    uniq = directed["raw"].collapse(directed["sid"], S) if S > 1 else directed["raw"].collapse()
    res = casc.run(uniq)
    seqs = uniq.unpack()
    ps, ref, _, _ = res.fetch()
    counts, _ = uniq.counts()
    fetched = (seqs, ps, ref, counts)
    useq = seqs.to_list()
    lens = seqs.lengths
    # ---- the case is what it claims to be
    want = case["counts"] if S > 1 else case["counts"].sum(axis=1, keepdims=True)
    at = {s: k for k, s in enumerate(case["reads"])}
    back = np.array([at[s] for s in useq])
    assert len(useq) == len(case["reads"]) > 1500 and np.array_equal(counts.astype(np.int64), want[back])
    assert np.isin(ps, (EXACT_PASS, ISO_PASS)).all() and np.array_equal(ref, case["made_from"][back])  # every read is a miRNA row
    assert (ps == EXACT_PASS).sum() > 100 and (ps == ISO_PASS).sum() > 1000
    gc = uniq.group_counts()  # width classes (reads of up to 31 nt in one word, up to 64 nt in two, ...) without an N, then with one
    half = len(gc) // 2
    assert gc[0] > 300 and gc[1] > 300 and gc[half] > 50 and gc[half + 1] > 50 and gc.sum() == gc[[0, 1, half, half + 1]].sum() == len(useq)
    has_n = np.array(["N" in s for s in useq])
    assert any(s.find("N") >= 32 for s in useq) and any(0 <= s.find("N") < 32 < len(s) for s in useq)
    for group in (lens <= 31, lens > 31):  # both width groups hold miRNA rows (every read is one), with and without an N
        assert (group & has_n).any() and {int(x) % 5 for x in lens[group & ~has_n]} == {0, 1, 2, 3, 4}
    assert set(range(16, 44)) <= {int(x) for x in lens}
    mlen = np.array([len(s) for s in case["lib_seqs"]])[ref]
    assert ((mlen == 38) & (lens == 41)).any() and (mlen + lens > 64).sum() > 100 and (mlen > 40).sum() > 50
    # short reads inside long canonicals: pairs the register form takes (canonical of 36..40 nt) and pairs of a canonical beyond it
    assert ((mlen >= 36) & (mlen <= 40) & (lens <= 23)).sum() > 40 and ((mlen > 40) & (lens <= 23)).sum() > 20
    if S > 1:
        assert {int(x) for x in np.unique(counts)} == set(COUNT_MENU)
        zeros = (counts == 0).sum(axis=1)
        assert (zeros == 1).any() and (zeros == 2).any() and (counts[:, 1:] == 0).any() and (counts[:, 0] == 0).any()
    else:
        assert counts.max() >= 100_000 and counts.min() >= 1
    # ---- the restatement of every row's line (None: the name has no annotation)
    lines = []
    for i in range(len(useq)):
        nm = oracle.gff_names(case["names"][ref[i]], case["mirDict"], case["pre_of"], pre)
        lines.append(None if nm is None else oracle.gff_line(nm[0], SOURCE, nm[1], useq[i], nm[3], nm[2], counts[i]))
    assert sum(ln is None for ln in lines) > 40
    fields = [ln.split("\t") for ln in lines if ln]
    assert any(f[0] == "hsa-miR-first-5p" and f[2:4] == ["ref_miRNA", "1"] for f in fields)  # start0 = 1
    assert any(f[0] == "hsa-miR-stem" for f in fields) and any(f[0] == "hsa-miR-var-5p" for f in fields)
    frame = uniq.sorted_order() if S > 1 else uniq.first_appearance_order()
    # a second order: the frame's rows shuffled (seeded, and a function of the sequences: the handle order of a collapse is not)
    by_seq = np.array(sorted(range(len(useq)), key=lambda i: useq[i]), dtype=np.int64)
    shuffled = by_seq[np.random.default_rng(14).permutation(len(useq))]
    for tag, order in (("frame", frame), ("shuffled", shuffled)):
        assert sorted(order.tolist()) == list(range(len(useq)))
        dev, host, n_lines, recs, rows = _both_routes(tmp_path, f"S{S}_{tag}", args, base_names, casc, uniq, res, fetched, order)
        my_rows, n_exact = _file_rows(ps, order)
        assert np.array_equal(rows, my_rows)
        # rows without a line stand inside both blocks, not at their ends
        for block in (recs["kind"][:n_exact], recs["kind"][n_exact:]):
            none = np.nonzero(block == 0)[0]
            assert none.size > 5 and none[0] > 0 and none[-1] < len(block) - 1 and block[0] != 0 and block[-1] != 0, (tag, none)
        assert [k == 0 for k in recs["kind"]] == [lines[i] is None for i in my_rows]
        assert not np.array_equal(order, np.arange(len(order)))
        # 1. the two routes write the same bytes
        assert dev == host, (tag, _first_difference(dev, host))
        # 2. every line is the restatement's, in the file's row order; rows of the names without annotation are absent
        text = dev.decode()
        assert text.startswith(_head(base_names))
        expected = [lines[i] for i in my_rows if lines[i] is not None]
        _assert_same_lines(text[len(_head(base_names)):].splitlines(keepends=True), expected, (S, tag))
        # 3. the line count the device call returns
        assert n_lines == text.count("\n") - 4 == len(expected)
    res.close(); uniq.close()


def _first_difference(a: bytes, b: bytes):
    n = min(len(a), len(b))
    bad = np.nonzero(np.frombuffer(a, np.uint8, n) != np.frombuffer(b, np.uint8, n))[0]
    k = int(bad[0]) if bad.size else n
    lo = a.rfind(b"\n", 0, k) + 1
    return dict(at=k, sizes=(len(a), len(b)), device=a[lo:lo + 400], host=b[lo:lo + 400])


def test_directed_gff_three_samples(directed, tmp_path):
    """S = 3: counts of one to six digits and zeros inside a row, the frame in sorted order and shuffled"""
    _directed_run(directed, tmp_path, 3)


def test_directed_gff_one_sample(directed, tmp_path):
    """the same reads as one sample, the counts summed: the frame in the order of first appearance and shuffled"""
    _directed_run(directed, tmp_path, 1)


def test_a_canonical_longer_than_48_nt_is_refused(directed, tmp_path):
    """k_isotype types canonicals of up to 48 nt (MIRGE_ISO_MAXA).  A longer one is an error of both routes, the device writer and
    the records for the host writer, not a file that silently lacks its rows; one of exactly 48 nt is taken."""
    casc = directed["casc"]
    uniq = directed["raw"].collapse()
    res = casc.run(uniq)
    ps = res.fetch()[0]
    order = uniq.first_appearance_order()
    rows, _ = _file_rows(ps, order)
    tables = dict(gff.name_tables(directed["args"], "miRBase", casc))
    longest = max(range(len(tables["masters"])), key=lambda k: len(tables["masters"][k]))
    assert len(tables["masters"][longest]) == 44
    for extra, refused in ((4, False), (5, True)):
        tables["masters"] = [m + "ACGTA"[:extra] if k == longest else m for k, m in enumerate(tables["masters"])]
        path = tmp_path / f"plus{extra}.gff"
        if refused:
            with pytest.raises(RuntimeError, match="longer than 48 nt"):
                gff.write_gff_device_with(tables, path, "miRBase", ["S1"], casc, uniq, res, order)
            with pytest.raises(RuntimeError, match="longer than 48 nt"):
                gff.isomir_records(casc, uniq, res, tables, rows.astype(np.int64))
        else:
            out = gff.write_gff_device_with(tables, path, "miRBase", ["S1"], casc, uniq, res, order)
            recs = gff.isomir_records(casc, uniq, res, tables, rows.astype(np.int64))
            assert out["lines"] == int((recs["kind"] != 0).sum()) == path.read_bytes().count(b"\n") - 4 > 1500
        tables["masters"] = [m[:44] if k == longest else m for k, m in enumerate(tables["masters"])]
    res.close(); uniq.close()


# ---------------------------------------------------------------- more than one text chunk
N_CHUNK_READS = 200_000  # raw reads whose miRNA rows give a body of a little more than two chunks (asserted below)


def test_gff_text_of_three_chunks(ctx, tmp_path):
    """A body of more than 2 x 8 MiB (three chunks, the last one short; several writer threads): the device file equals the host
    route's byte for byte, and the lines at and next to every chunk boundary, the first and last lines and 2 000 random ones
    equal the restatement (all of them would take minutes of difflib)."""
    sl = synth.make_libraries(seed=20260101, scale="small")
    casc = Cascade(ctx, sl.libs)
    reads = synth.make_reads(sl, N_CHUNK_READS, seed=5, mix=dict(exact=0.25, isomir=0.55, hairpin=0.1, random=0.1), n_frac=0.02)
    raw = _ffi.DeviceReads.pack(ctx, reads)
    uniq = raw.collapse()
    res = casc.run(uniq)
    mir, hp = sl.libs["mirna"], sl.libs["hairpin"]
    mirDict = dict(zip(mir.names, mir.seqs.to_list()))
    pre_of = {nm: hp.names[int(sl.mir_hairpin[k])] for k, nm in enumerate(mir.names)}
    pre = dict(zip(hp.names, hp.seqs.to_list()))
    pre[hp.names[-1]] = ""
    args = write_gff_name_files(tmp_path / "libs", mirDict, pre_of)
    seqs = uniq.unpack()
    ps, ref, _, _ = res.fetch()
    counts, _ = uniq.counts()
    order = uniq.first_appearance_order()
    dev, host, n_lines, recs, rows = _both_routes(tmp_path, "chunks", args, ["S1"], casc, uniq, res, (seqs, ps, ref, counts), order)
    head = _head(["S1"]).encode()
    assert dev.startswith(head)
    body = dev[len(head):]
    body_bytes = len(body)
    print(f"gff body: {body_bytes} bytes, {n_lines} lines, {len(rows)} miRNA rows of {len(uniq)} unique reads")
    assert 2 * CHUNK < body_bytes < 3 * CHUNK
    assert dev == host, _first_difference(dev, host)
    my_rows, _ = _file_rows(ps, order)
    assert np.array_equal(rows, my_rows)
    resolved = {nm: oracle.gff_names(nm, mirDict, pre_of, pre) for nm in mir.names}
    with_line = [int(i) for i in my_rows if resolved[mir.names[ref[i]]] is not None]
    got = body.split(b"\n")
    assert got[-1] == b"" and len(got) - 1 == len(with_line) == n_lines == dev.count(b"\n") - 4
    ends = np.cumsum([len(g) + 1 for g in got[:-1]])  # ends[k] = offset behind line k
    pick = {0, len(with_line) - 1}
    for k in range(1, 3):
        at = int(np.searchsorted(ends, k * CHUNK, side="right"))  # the line that holds byte k * CHUNK of the body
        assert (ends[at - 1] if at else 0) <= k * CHUNK < ends[at]
        pick |= {at - 1, at, at + 1}
    pick |= {int(x) for x in np.random.default_rng(3).integers(0, len(with_line), size=2000)}
    for k in sorted(pick):
        i = with_line[k]
        nm = resolved[mir.names[ref[i]]]
        want = oracle.gff_line(nm[0], SOURCE, nm[1], seqs.get(i), nm[3], nm[2], counts[i])
        assert got[k] + b"\n" == want.encode(), (k, got[k], want)
    res.close(); uniq.close(); raw.close(); casc.close()

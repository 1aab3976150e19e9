"""A small BAM / BAI reader for the ``--sorted-bam`` tests: ``zlib`` + ``struct``, written from the SAM specification (sections 4.1,
4.2, 5.2, 5.3) and from the issue's description of the index -- not from the code under test.

``read_bgzf`` checks every member (magic, the BC subfield, BSIZE, CRC-32, ISIZE, the EOF block at the end) and reports its deflate
block type; ``decode_bam`` turns the records back into SAM lines and gives every record its virtual offsets; ``build_bai`` is the
tests' own index builder; ``parse_bai`` / ``query`` answer a region query the way a reader of the index does."""
import bisect
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_SEQ = "=ACMGRSVTWYHKDBN"


def read_bgzf(data):
    """-> [dict(at, bsize, payload, btype)] of every member but the EOF block, which must end the file"""
    assert data.endswith(EOF_BLOCK), "no EOF block at the end"
    members, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04", f"member at {at}: no gzip header with FEXTRA"
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        assert xlen == 6 and data[at + 12:at + 16] == b"BC\x02\x00", f"member at {at}: no BC subfield"
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert bsize <= 65536 and at + bsize <= len(data)
        cdata = data[at + 18:at + bsize - 8]
        crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
        z = zlib.decompressobj(-15)
        payload = z.decompress(cdata) + z.flush()
        assert z.eof and not z.unused_data, f"member at {at}: the deflate stream does not fill cdata exactly"
        assert len(payload) == isize and isize <= 65536 and zlib.crc32(payload) & 0xFFFFFFFF == crc, f"member at {at}: ISIZE / CRC-32"
        # (btype: of the member's FIRST deflate block; single = that block is also its last)
        members.append(dict(at=at, bsize=bsize, payload=payload, btype=(cdata[0] >> 1) & 3, single=bool(cdata[0] & 1)))
        at += bsize
    assert members[-1]["at"] == len(data) - 28 and members[-1]["payload"] == b""
    assert all(m["payload"] for m in members[:-1]), "an empty member in front of the EOF block"
    return members[:-1] + [members[-1]]


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14: return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17: return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20: return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23: return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26: return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def decode_bam(data):
    """-> dict(text, refs [(name, length)], lines [SAM line without newline], recs [(refID, pos, end, vbeg, vend)], members)"""
    members = read_bgzf(data)
    body = members[:-1]
    stream = b"".join(m["payload"] for m in body)
    starts, u = [], 0
    for m in body:
        starts.append(u)
        u += len(m["payload"])
    sizes = {len(m["payload"]) for m in body[:-1]}
    assert len(sizes) <= 1 and (not sizes or len(body[-1]["payload"]) <= max(sizes)), "members of different uncompressed sizes"
    block = sizes.pop() if sizes else max(len(stream), 1)
    offs = [m["at"] for m in members]  # (the EOF block's offset is the last)

    def voff(v):  # a position on a member boundary -- the end of the stream included -- belongs to the member that follows
        k = bisect.bisect_right(starts, v) - 1 if v < len(stream) else len(body)
        return (offs[k] << 16) | (v - starts[k] if k < len(body) else 0)
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    text = stream[8:8 + l_text]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", stream, at)[0]
        name = stream[at + 4:at + 4 + l_name]
        assert name.endswith(b"\0")
        refs.append((name[:-1].decode(), struct.unpack_from("<i", stream, at + 4 + l_name)[0]))
        at += 8 + l_name
    lines, recs = [], []
    while at < len(stream):
        size = struct.unpack_from("<i", stream, at)[0]
        refid, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", stream, at + 4)
        p = at + 36
        qname = stream[p:p + l_name]
        assert qname.endswith(b"\0") and b"\0" not in qname[:-1]
        p += l_name
        cigar = ""
        for k in range(n_cig):
            w = struct.unpack_from("<I", stream, p + 4 * k)[0]
            cigar += f"{w >> 4}{'MIDNSHP=X'[w & 15]}"
        p += 4 * n_cig
        packed = stream[p:p + (l_seq + 1) // 2]
        seq = "".join(_SEQ[(packed[k >> 1] >> (4 if k % 2 == 0 else 0)) & 15] for k in range(l_seq))
        if l_seq % 2:
            assert packed[-1] & 15 == 0
        p += (l_seq + 1) // 2
        qual = "".join(chr(q + 33) for q in stream[p:p + l_seq])
        p += l_seq
        tags = []
        while p < at + 4 + size:
            tag, typ = stream[p:p + 2].decode(), chr(stream[p + 2])
            if typ == "C":
                tags.append(f"{tag}:i:{stream[p + 3]}")
                p += 4
            else:
                assert typ == "Z", typ
                e = stream.index(b"\0", p + 3)
                tags.append(f"{tag}:Z:{stream[p + 3:e].decode()}")
                p = e + 1
        assert p == at + 4 + size, "a record's fields do not fill block_size"
        assert (nref, npos, tlen, n_cig) == (-1, -1, 0, 1) and bin_ == reg2bin(pos, pos + l_seq)
        assert [t[:2] for t in tags] == ["XA", "MD", "NM"]
        lines.append("\t".join([qname[:-1].decode(), str(flag), refs[refid][0], str(pos + 1), str(mapq), cigar, "*", "0", "0", seq, qual] + tags))
        recs.append((refid, pos, pos + l_seq, voff(at), voff(at + 4 + size)))
        at += 4 + size
    assert at == len(stream)
    return dict(text=text, refs=refs, lines=lines, recs=recs, members=members, block=block)


def sort_key(line, refid_of):
    f = line.split("\t")
    return (refid_of[f[2]], int(f[3]) - 1, 1 if int(f[1]) & 16 else 0)


def build_bai(n_ref, recs):
    """the index the issue describes, from the decoded records (refID, pos, end, vbeg, vend) in file order"""
    out = b"BAI\1" + struct.pack("<i", n_ref)
    for ref in range(n_ref):
        mine = [r for r in recs if r[0] == ref]
        runs = []  # maximal runs of consecutive records with one bin: [bin, vbeg, vend]
        for _, pos, end, vb, ve in mine:
            b = reg2bin(pos, end)
            if runs and runs[-1][0] == b:
                runs[-1][2] = ve
            else:
                runs.append([b, vb, ve])
        bins = {}
        for b, vb, ve in runs:
            chunks = bins.setdefault(b, [])
            if chunks and chunks[-1][1] == vb:  # adjacent runs, contiguous in the file
                chunks[-1][1] = ve
            else:
                chunks.append([vb, ve])
        n_win = max(((end - 1) >> 14) + 1 for _, _, end, _, _ in mine) if mine else 0
        lin = [None] * n_win
        for _, pos, end, vb, _ in mine:
            for w in range(pos >> 14, ((end - 1) >> 14) + 1):
                if lin[w] is None:
                    lin[w] = vb
        for w in reversed(range(n_win - 1)):
            if lin[w] is None:
                lin[w] = lin[w + 1]
        out += struct.pack("<i", len(bins) + (1 if mine else 0))
        for b in sorted(bins):
            out += struct.pack("<Ii", b, len(bins[b]))
            for vb, ve in bins[b]:
                out += struct.pack("<QQ", vb, ve)
        if mine:
            out += struct.pack("<IiQQQQ", 37450, 2, mine[0][3], mine[-1][4], len(mine), 0)
        out += struct.pack("<i", n_win) + b"".join(struct.pack("<Q", v) for v in lin)
    return out + struct.pack("<Q", 0)


def parse_bai(data):
    assert data[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", data, 4)[0]
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", data, at)[0]
        at += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", data, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if b == 37450:
                meta = chunks
            else:
                bins[b] = chunks
        n_intv = struct.unpack_from("<i", data, at)[0]
        lin = list(struct.unpack_from(f"<{n_intv}Q", data, at + 4))
        at += 4 + 8 * n_intv
        refs.append(dict(bins=bins, meta=meta, lin=lin))
    assert struct.unpack_from("<Q", data, at)[0] == 0 and at + 8 == len(data)
    return refs


def query(index, recs, refid, beg, end):
    """indices of the records that overlap [beg, end) of reference refid, found through the index as a reader would"""
    ref = index[refid]
    w = beg >> 14
    min_off = ref["lin"][w] if w < len(ref["lin"]) else (ref["lin"][-1] if ref["lin"] else 0)
    chunks = [c for b in reg2bins(beg, end) for c in ref["bins"].get(b, []) if c[1] > min_off]
    hit = set()
    for k, (rid, pos, rend, vb, _) in enumerate(recs):
        if any(cb <= vb < ce for cb, ce in chunks) and rid == refid and pos < end and rend > beg:
            hit.add(k)
    return hit


def brute(recs, refid, beg, end):
    return {k for k, (rid, pos, rend, _, _) in enumerate(recs) if rid == refid and pos < end and rend > beg}

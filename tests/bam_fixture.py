"""A BAM / BGZF writer for the tests (struct and zlib only), after the SAM
specification, sections 4.1 (BGZF) and 4.2 (BAM).  It writes what it is told,
wrong records included: the damage cases of tests/golden/make_golden_bam.py
come from here."""
import os
import struct
import zlib

NT16 = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=XB"           # op codes 0..9; 10..15 are given as integers
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_block(data: bytes, level: int = 6) -> bytes:
    assert len(data) <= 65280
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    head = struct.pack("<4BI2BH2BHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(body) + 25)
    return head + body + struct.pack("<II", zlib.crc32(data), len(data))


def bgzf(data: bytes, block: int = 65280, eof: bool = True, level: int = 6) -> bytes:
    """data in blocks of `block` bytes of text each, then the EOF block."""
    out = [bgzf_block(data[i:i + block], level) for i in range(0, len(data), block)]
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def bgzf_blocks(raw: bytes):
    """[(offset, size)] of the blocks of a BGZF file made by bgzf()."""
    out, at = [], 0
    while at < len(raw):
        size = struct.unpack_from("<H", raw, at + 16)[0] + 1
        out.append((at, size))
        at += size
    return out


def cigar_words(cigar):
    """[(op, length)] with op a letter of OPS or an op code -> uint32 words."""
    return [(n << 4) | (OPS.index(op) if isinstance(op, str) else op) for op, n in cigar]


def ref_len(cigar) -> int:
    return sum(w >> 4 for w in cigar_words(cigar) if (w & 15) in (0, 2, 3, 7, 8))


def query_len(cigar) -> int:
    return sum(w >> 4 for w in cigar_words(cigar) if (w & 15) in (0, 1, 4, 7, 8))


def reg2bin(beg: int, end: int) -> int:
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def record(tid, pos, flag, cigar, seq, name=b"r", mapq=30, aux=b"", l_seq=None, block_size=None) -> bytes:
    """One alignment record with its block_size word.  seq: letters of NT16;
    l_seq / block_size: values to write in place of the true ones."""
    words = cigar_words(cigar)
    nib = [NT16.index(ch) for ch in seq] + [0]
    packed = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(seq), 2))
    name = name + b"\0"
    end = pos + (ref_len(cigar) or 1)
    body = struct.pack("<iiBBHHHIiii", tid, pos, len(name), mapq, reg2bin(max(pos, 0), max(end, 1)), len(words), flag,
                       len(seq) if l_seq is None else l_seq, -1, -1, 0)
    body += name + struct.pack("<%dI" % len(words), *words) + packed + b"\xff" * len(seq) + aux
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def header(refs, text: str = None) -> bytes:
    """refs: [(name, length)]."""
    if text is None:
        text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    out = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    return out


def bam(refs, records, block: int = 65280, eof: bool = True) -> bytes:
    return bgzf(header(refs) + b"".join(records), block, eof)


def random_cigar(rng, n_ops: int, max_len: int = 12, ops="MMMM=XIDNSHP"):
    """n_ops operations (numpy Generator rng), clips only at the ends; the ops
    string weights the choice, integers 9..15 may be mixed in by the caller."""
    out = []
    for i in range(n_ops):
        op = ops[int(rng.integers(0, len(ops)))]
        if op in "SH" and 0 < i < n_ops - 1:
            op = "M"
        out.append((op, int(rng.integers(1, max_len + 1))))
    return out


def split_bam(raw: bytes):
    """(header bytes, [record bytes]) of a sound BGZF BAM."""
    text = b"".join(zlib.decompress(raw[o + 18:o + n - 8], -15) for o, n in bgzf_blocks(raw))
    l_text, = struct.unpack_from("<i", text, 4)
    at = 12 + l_text
    for _ in range(struct.unpack_from("<i", text, at - 4)[0]):
        at += 8 + struct.unpack_from("<i", text, at)[0]
    head, recs = text[:at], []
    while at < len(text):
        n = 4 + struct.unpack_from("<i", text, at)[0]
        recs.append(text[at:at + n])
        at += n
    return head, recs


def derive(src: str, dst: str) -> None:
    """The working directory of the golden cases (tests/golden/bam/manifest.json)
    from the committed files of src: links to them, the same BAM under the two
    index names and beside an index with a wrong magic, and the damaged files,
    all cut from small.bam (200 records in 1 KB blocks)."""
    def put(name, data):
        with open(os.path.join(dst, name), "wb") as f:
            f.write(data)

    def get(name):
        with open(os.path.join(src, name), "rb") as f:
            return f.read()

    for fn in os.listdir(src):
        os.symlink(os.path.join(os.path.abspath(src), fn), os.path.join(dst, fn))
    a, index = get("a.bam"), get("a.index")
    for name, idx_name, idx in (("a_i.bam", "a_i.bam.bai", index), ("a_j.bam", "a_j.bai", index),
                                ("a_k.bam", "a_k.bam.bai", b"BAJ\1" + index[4:])):
        put(name, a)
        put(idx_name, idx)
    put("long_i.bam", get("long.bam"))
    put("long_i.bam.bai", get("long.index"))
    raw = get("small.bam")
    head, small = split_bam(raw)
    blocks = bgzf_blocks(raw)
    put("d_noeof.bam", raw[:blocks[-1][0]])
    off, size = blocks[len(blocks) // 2]
    put("d_midblock.bam", raw[:off + size // 2])
    # a block border inside a record: the text before block k does not end where a record ends
    ends, at = set(), len(head)
    for r in small:
        at += len(r)
        ends.add(at)
    k = next(k for k in range(len(blocks) // 3, len(blocks)) if k * 1024 not in ends and k * 1024 > len(head))
    put("d_border.bam", raw[:blocks[k][0]])
    off, size = blocks[len(blocks) // 2 + 1]
    flipped = bytearray(raw)
    flipped[off + 18 + (size - 26) // 2] ^= 0x10
    put("d_flip.bam", bytes(flipped))
    bad = record(0, 1500, 0, [("M", 20), ("I", 2)], "ACGT" * 5, name=b"bad")          # CIGAR asks 22 bases, l_seq 20
    for name, n in (("d_mismatch.bam", 1), ("d_mismatch_twice.bam", 2), ("d_mismatch_thrice.bam", 3)):
        put(name, bgzf(head + b"".join(small[:90]) + bad * n + b"".join(small[90:]), 1024))
    # the reference reads in batches of 1,000: here the failed read is the first of its batch, once
    put("d_mismatch_batch.bam", bgzf(head + b"".join(small[:200] * 5) + bad + b"".join(small[:50])))
    bs8 = record(0, 1500, 0, [("M", 4)], "ACGT", name=b"bs8", block_size=8)
    put("d_bs8.bam", bgzf(head + b"".join(small[:110]) + bs8 + b"".join(small[110:]), 1024))

"""Cases for the device BGZF inflater (tests/test_bgzf_fixture.py on the CPU,
tests/test_bgzf.py on the GPU, tools/bgzf_inflate_asan.sh under the sanitizers).

The statement every decoder here is held to is zlib's: `statement(payload,
isize, crc)` runs zlib.decompressobj(-15) over a member's payload; the block is
ok iff the stream reaches its end, the text has ISIZE bytes and zlib.crc32 of
it is the trailer's.  Bytes behind the final deflate block are ignored, as the
host reader's bgzf_inflate ignores them.  One rule is BGZF's, not deflate's: a
block holds at most 65,536 bytes of text, so a larger ISIZE is never ok (the
host reader refuses such a member before it inflates it).

Helpers: a BGZF writer with a chosen level, strategy, payload size and XLEN; a
bit-level writer; a hand-written fixed-Huffman encoder for any sequence of
literals and (length, distance) pairs; a writer of dynamic headers from chosen
code lengths and a chosen run-length coding of them; and `inspect`, a plain
Python inflater that reports what a stream contains (block types, code
lengths, repeat codes, length and distance symbols with their extra bits), so
that the test of this fixture can show that every class holds what it is named
for.

`python3 tests/bgzf_fixture.py DIR` writes every case as DIR/<name>.bgzf, a run
of BGZF members, for tools/bgzf_inflate_check.cpp.
"""
import os
import random
import struct
import sys
import zlib

MAX_TEXT = 65536
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
DEXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

# status codes (VC_BGZF_E* of include/vafc.h)
(EBTYPE, ESTORED, ETOOMANY, ELENS, EREPEAT, ENOEOB, ESYMBOL, EDIST, EPAST, ESHORT, EINPUT, ECRC, EISIZE) = range(1, 14)


# ---------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------

def statement(payload: bytes, isize: int, crc: int):
    """(ok, text) of one member under zlib; text is None where zlib gives none."""
    if isize > MAX_TEXT:
        return False, None
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(payload)
        text += d.flush()
    except zlib.error:
        return False, None
    if not d.eof:
        return False, None
    return (len(text) == isize and zlib.crc32(text) == crc), text


# ---------------------------------------------------------------------------
# BGZF members
# ---------------------------------------------------------------------------

class Member:
    """One BGZF member: payload, trailer, extra-field padding; `code` is the
    status the case is built to end in (None: whatever the statement says)."""

    def __init__(self, payload, isize, crc, xpad=0, bc_first=True, code=None):
        self.payload, self.isize, self.crc, self.xpad, self.bc_first, self.code = bytes(payload), isize, crc, xpad, bc_first, code

    def raw(self) -> bytes:
        # xpad 0, or a second subfield of xpad >= 4 bytes in all
        pad = b"" if self.xpad == 0 else b"XP" + struct.pack("<H", self.xpad - 4) + bytes(self.xpad - 4)
        xlen = 6 + len(pad)
        total = 12 + xlen + len(self.payload) + 8
        assert total <= 65536, total
        bc = b"BC\x02\x00" + struct.pack("<H", total - 1)
        extra = bc + pad if self.bc_first else pad + bc
        return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + self.payload +
                struct.pack("<II", self.crc & 0xFFFFFFFF, self.isize & 0xFFFFFFFF))

    def payload_offset(self) -> int:
        return 12 + 6 + self.xpad

    def verdict(self):
        return statement(self.payload, self.isize, self.crc)


def member_of(text: bytes, payload: bytes, **kw) -> Member:
    return Member(payload, len(text), zlib.crc32(text), **kw)


EOF_MEMBER = Member(b"\x03\x00", 0, 0)
assert len(EOF_MEMBER.raw()) == 28


def deflate_raw(text: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_SYNC_FLUSH) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b"", 0
    for f in flush_at:
        out += c.compress(text[at:f]) + c.flush(flush)
        at = f
    return out + c.compress(text[at:]) + c.flush()


def wrap(text: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, payload_size=65280, xpad=0):
    """text as BGZF members of payload_size bytes of text each (the last shorter)."""
    return [member_of(text[i:i + payload_size], deflate_raw(text[i:i + payload_size], level, strategy), xpad=xpad)
            for i in range(0, max(len(text), 1), payload_size)]


def bgzf_bytes(text: bytes, level=6, payload_size=65280, eof=True) -> bytes:
    ms = wrap(text, level, payload_size=payload_size) if text else []
    return b"".join(m.raw() for m in ms) + (EOF_MEMBER.raw() if eof else b"")


# ---------------------------------------------------------------------------
# bit-level writing
# ---------------------------------------------------------------------------

class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        """n bits of v, least significant first (header fields, extra bits)."""
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        """A Huffman code of n bits, most significant first."""
        for i in range(n - 1, -1, -1):
            self.bits((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


def canonical_codes(lengths):
    """RFC 1951 3.2.2: {symbol: (code, length)} of the symbols with a length."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32


def length_symbol(length):
    s = max(i for i in range(29) if LBASE[i] <= length)
    return s, length - LBASE[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DBASE[i] <= dist)
    return s, dist - DBASE[s]


def put_ops(w: BitWriter, ops, lit_codes, dist_codes):
    """ops: ("lit", byte) | ("match", length, dist) | ("match", length, dist, length symbol) |
    ("raw_l", literal/length symbol) | ("raw_d", distance symbol, extra value, extra bits) | ("eob",)"""
    for op in ops:
        if op[0] == "lit":
            w.code(*lit_codes[op[1]])
        elif op[0] == "eob":
            w.code(*lit_codes[256])
        elif op[0] == "raw_l":
            w.code(*lit_codes[op[1]])
        elif op[0] == "raw_d":
            w.code(*dist_codes[op[1]])
            w.bits(op[2], op[3])
        else:
            length, dist = op[1], op[2]
            if len(op) > 3:
                ls, le = op[3], length - LBASE[op[3]]
                assert 0 <= le < (1 << LEXTRA[ls])
            else:
                ls, le = length_symbol(length)
            w.code(*lit_codes[257 + ls])
            w.bits(le, LEXTRA[ls])
            ds, de = dist_symbol(dist)
            w.code(*dist_codes[ds])
            w.bits(de, DEXTRA[ds])


def expand(ops) -> bytes:
    """The text a valid op sequence stands for."""
    out = bytearray()
    for op in ops:
        if op[0] == "lit":
            out.append(op[1])
        elif op[0] == "match":
            assert 1 <= op[2] <= len(out), (op, len(out))
            for _ in range(op[1]):
                out.append(out[-op[2]])
    return bytes(out)


def fixed_block(w: BitWriter, ops, final=True, eob=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    put_ops(w, list(ops) + ([("eob",)] if eob else []), canonical_codes(FIXED_LIT_LENS), canonical_codes(FIXED_DIST_LENS))


def fixed_stream(ops) -> bytes:
    w = BitWriter()
    fixed_block(w, ops)
    return w.done()


def complete_lengths(n):
    """Lengths of a complete code of n >= 2 symbols."""
    k = n.bit_length() - 1
    short = (2 << k) - n
    return [k] * short + [k + 1] * (n - short) if k else [1, 1]


def rle_lengths(seq, use=(16, 17, 18)):
    """seq as code-length symbols [(symbol, extra value)], greedily with the repeat codes allowed."""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 11 and 18 in use:
            n = min(run, 138)
            out.append((18, n - 11))
        elif v == 0 and run >= 3 and 17 in use:
            n = min(run, 10)
            out.append((17, n - 3))
        elif v != 0 and run >= 4 and 16 in use:
            n = min(run - 1, 6)
            out.append((v, 0))
            out.append((16, n - 3))
            n += 1
        else:
            n = 1
            out.append((v, 0))
        i += n
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dynamic_header(w: BitWriter, hlit, hdist, cl_lens, cl_ops, final=True, hclen=None):
    """The header of a dynamic block, as told: cl_lens {code-length symbol: length}, cl_ops the coded lengths."""
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    if hclen is None:
        hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens.get(s, 0)])
    w.bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.bits(cl_lens.get(s, 0), 3)
    codes = canonical_codes([cl_lens.get(s, 0) for s in range(19)])
    for s, extra in cl_ops:
        w.code(*codes[s])
        if s >= 16:
            w.bits(extra, CL_EXTRA[s])


def dynamic_block(w: BitWriter, lit_lens, dist_lens, ops, final=True, use=(16, 17, 18), eob=True):
    """A well-formed dynamic block with these code lengths (HLIT = len(lit_lens), HDIST = len(dist_lens))."""
    cl_ops = rle_lengths(list(lit_lens) + list(dist_lens), use)
    used = sorted({s for s, _ in cl_ops})
    if len(used) == 1:
        used.append(0 if used[0] != 0 else 1)   # the code-length code must be complete
    cl_lens = dict(zip(used, complete_lengths(len(used))))
    dynamic_header(w, len(lit_lens), len(dist_lens), cl_lens, cl_ops, final)
    put_ops(w, list(ops) + ([("eob",)] if eob else []), canonical_codes(lit_lens), canonical_codes(dist_lens))
    return cl_ops


# ---------------------------------------------------------------------------
# a plain inflater that reports what it saw
# ---------------------------------------------------------------------------

class _Bits:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def peek(self, n):
        """n <= 16 bits, zeros behind the end."""
        i = self.pos >> 3
        return (int.from_bytes(self.d[i:i + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def skip(self, n):
        self.pos += n
        if self.pos > 8 * len(self.d):
            raise ValueError("input exhausted")

    def take(self, n):
        v = self.peek(n)
        self.skip(n)
        return v


def _table(lengths):
    """(longest code, [(symbol, length) or None] indexed by that many input bits)."""
    mx = max(lengths) if lengths else 0
    if mx == 0:
        return 1, [None, None]
    tab = [None] * (1 << mx)
    for s, (c, l) in canonical_codes(lengths).items():
        rev = int(format(c, "0%db" % l)[::-1], 2)
        tab[rev::1 << l] = [(s, l)] * (1 << (mx - l))
    return mx, tab


def _decode(b, t):
    e = t[1][b.peek(t[0])]
    if e is None:
        raise ValueError("no such code")
    b.skip(e[1])
    return e[0]


def inspect(payload: bytes):
    """(text, info) of a valid raw deflate stream.  info: btypes, stored (lengths of stored blocks), headers (one
    dict per dynamic block: hlit, hdist, hclen, cl_syms, crossing (a repeat that runs from the literal/length
    lengths into the distance lengths), max_lit, max_dist, n_dist), lsyms {(length symbol, extra value)},
    dsyms {(distance symbol, extra value)}, matches [(length, distance, offset of the match)]."""
    b = _Bits(payload)
    out = bytearray()
    info = dict(btypes=[], stored=[], headers=[], lsyms=set(), dsyms=set(), matches=[], literals=0)
    while True:
        final, btype = b.take(1), b.take(2)
        info["btypes"].append(btype)
        if btype == 0:
            b.pos = (b.pos + 7) & ~7
            n, nn = b.take(16), b.take(16)
            if n != nn ^ 0xFFFF:
                raise ValueError("stored lengths")
            if (b.pos >> 3) + n > len(payload):
                raise ValueError("input exhausted")
            out += payload[b.pos >> 3:(b.pos >> 3) + n]
            b.pos += 8 * n
            info["stored"].append(n)
        elif btype == 3:
            raise ValueError("block type 3")
        else:
            if btype == 1:
                lit, dist = FIXED_LIT_LENS, FIXED_DIST_LENS
            else:
                hlit, hdist, hclen = 257 + b.take(5), 1 + b.take(5), 4 + b.take(4)
                cl = [0] * 19
                for s in CL_ORDER[:hclen]:
                    cl[s] = b.take(3)
                t, lens, syms, crossing = _table(cl), [], set(), False
                while len(lens) < hlit + hdist:
                    s = _decode(b, t)
                    syms.add(s)
                    at = len(lens)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.take(2))
                    elif s == 17:
                        lens += [0] * (3 + b.take(3))
                    else:
                        lens += [0] * (11 + b.take(7))
                    if s >= 16 and at < hlit < len(lens):
                        crossing = True
                if len(lens) > hlit + hdist:
                    raise ValueError("repeat past the end")
                lit, dist = lens[:hlit], lens[hlit:]
                info["headers"].append(dict(hlit=hlit, hdist=hdist, hclen=hclen, cl_syms=syms, crossing=crossing,
                                            max_lit=max(lit), max_dist=max(dist), n_dist=sum(1 for x in dist if x)))
            lt, dt = _table(lit), _table(dist)
            while True:
                s = _decode(b, lt)
                if s < 256:
                    out.append(s)
                    info["literals"] += 1
                elif s == 256:
                    break
                else:
                    s -= 257
                    if s >= 29:
                        raise ValueError("length symbol")
                    e = b.take(LEXTRA[s])
                    d = _decode(b, dt)
                    if d >= 30:
                        raise ValueError("distance symbol")
                    de = b.take(DEXTRA[d])
                    length, distance = LBASE[s] + e, DBASE[d] + de
                    if distance > len(out):
                        raise ValueError("distance too far")
                    info["lsyms"].add((s, e))
                    info["dsyms"].add((d, de))
                    info["matches"].append((length, distance, len(out)))
                    for _ in range(length):
                        out.append(out[-distance])
        if final:
            return bytes(out), info


# ---------------------------------------------------------------------------
# texts
# ---------------------------------------------------------------------------

def fastq_text(seed, n_bytes, read_len=150) -> bytes:
    rng = random.Random(seed)
    out, i = [], 0
    size = 0
    while size < n_bytes:
        seq = "".join(rng.choice("ACGT") for _ in range(read_len))
        qual = "".join(rng.choice("FFFFFF:,#") for _ in range(read_len))
        rec = "@SRR1.%d %d/1\n%s\n+\n%s\n" % (i, i, seq, qual)
        out.append(rec)
        size += len(rec)
        i += 1
    return "".join(out).encode()[:n_bytes]


def random_bytes(seed, n) -> bytes:
    return random.Random(seed).randbytes(n)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------

def _grow(ops, size, target):
    """Matches of 258 bytes at distance 64 until the text has `target` bytes."""
    while size < target:
        n = min(258, target - size)
        if n < 3:
            ops += [("lit", 0x2E)] * n
        else:
            ops.append(("match", n, 64))
        size += n
    return size


def hand_all_codes():
    """Every length code and every distance code at both ends of its extra-bit range."""
    ops = [("lit", 33 + i) for i in range(64)]
    size = 64
    lengths = [l for s in range(29) for l in sorted({LBASE[s], LBASE[s] + (1 << LEXTRA[s]) - 1})]
    k = 0
    for ds in range(30):
        for d in sorted({DBASE[ds], DBASE[ds] + (1 << DEXTRA[ds]) - 1}):
            size = _grow(ops, size, d)
            ops.append(("match", lengths[k % len(lengths)], d))
            size += lengths[k % len(lengths)]
            k += 1
    for l in lengths:   # every length once more, at a short distance
        ops.append(("match", l, 1 + l % 70))
        size += l
    ops.append(("match", 258, 300, 27))   # 258 as code 284 with all five extra bits set
    size += 258
    assert size <= MAX_TEXT
    return ops


def hand_edges():
    """The cooperative copy's edges: distances 1, 2, 3, 63, 64, 65 with lengths on both sides of them and of 64
    and 128, length 3 and 258, distance 1 with length 258, a match that starts at the block's first byte."""
    ops = [("lit", 97), ("match", 258, 1), ("match", 3, 1)]
    size = 262
    ops += [("lit", 65 + i % 26) for i in range(70)]
    size += 70
    for d in (1, 2, 3, 63, 64, 65):
        for l in sorted({3, 4, max(3, d - 1), max(3, d), max(3, d + 1), 62, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 257, 258}):
            ops.append(("lit", 48 + (l + d) % 10))   # the period is not what the last copy left
            ops.append(("match", l, d))
            size += 1 + l
    ops.append(("match", 100, size))   # its source is the block's first byte
    return ops


def hand_far():
    """Distance 32,768, from the first byte and later."""
    ops = [("lit", 33 + i) for i in range(64)]
    size = _grow(ops, 64, 32768)
    ops += [("match", 258, 32768), ("match", 3, 32768), ("lit", 10), ("match", 200, 32768), ("match", 258, 32767)]
    return ops


def _member_from_ops(ops, dynamic=None, **kw):
    text = expand(ops)
    if dynamic is None:
        payload = fixed_stream(ops)
    else:
        w = BitWriter()
        dynamic_block(w, *dynamic, ops)
        payload = w.done()
    return member_of(text, payload, **kw)


def _dyn_with(use, lit, dist, ops):
    w = BitWriter()
    dynamic_block(w, lit, dist, ops, use=use)
    return member_of(expand(ops), w.done())


def malformed_cases():
    """{name: Member}, each built to end in the status code it carries."""
    out = {}
    good_text = fastq_text(5, 3000)
    good = deflate_raw(good_text, 6)
    crc = zlib.crc32(good_text)

    w = BitWriter()
    w.bits(1, 1), w.bits(3, 2)
    out["bad_btype3"] = Member(w.done(), 0, 0, code=EBTYPE)

    out["bad_stored_nlen"] = Member(b"\x01\x05\x00\xfa\xfe" + b"hello", 5, zlib.crc32(b"hello"), code=ESTORED)

    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(30, 5), w.bits(0, 5), w.bits(0, 4), w.bits(0, 32)
    out["bad_hlit_287"] = Member(w.done() + bytes(8), 0, 0, code=ETOOMANY)
    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(30, 5), w.bits(0, 4), w.bits(0, 32)
    out["bad_hdist_31"] = Member(w.done() + bytes(8), 0, 0, code=ETOOMANY)

    # the code-length code: four codes of one bit; one code of one bit
    w = BitWriter()
    dynamic_header(w, 257, 1, {16: 1, 17: 1, 18: 1, 0: 1}, [])
    out["bad_cl_oversubscribed"] = Member(w.done() + bytes(16), 0, 0, code=ELENS)
    w = BitWriter()
    dynamic_header(w, 257, 1, {0: 1}, [])
    out["bad_cl_incomplete"] = Member(w.done() + bytes(16), 0, 0, code=ELENS)
    # the literal/length code: three codes of one bit (symbols 0, 1 and 256)
    w = BitWriter()
    dynamic_header(w, 257, 1, {0: 1, 1: 2, 18: 2},
                   [(1, 0), (1, 0), (18, 127), (18, 116 - 11), (1, 0), (0, 0)])   # 2 + 138 + 116 = 256 lengths, then 256, then the distance
    out["bad_lit_oversubscribed"] = Member(w.done() + bytes(16), 0, 0, code=ELENS)
    # ... incomplete: symbols 0 and 256 of two bits each
    w = BitWriter()
    dynamic_header(w, 257, 1, {0: 1, 2: 2, 18: 2}, [(2, 0), (0, 0), (18, 127), (18, 116 - 11), (2, 0), (0, 0)])
    out["bad_lit_incomplete"] = Member(w.done() + bytes(16), 0, 0, code=ELENS)

    w = BitWriter()
    dynamic_header(w, 257, 1, {16: 1, 0: 1}, [(16, 0)])
    out["bad_repeat_first"] = Member(w.done() + bytes(16), 0, 0, code=EREPEAT)
    w = BitWriter()
    dynamic_header(w, 257, 1, {18: 1, 0: 1}, [(18, 127), (18, 127)])   # 276 lengths where 258 are due
    out["bad_repeat_past_end"] = Member(w.done() + bytes(16), 0, 0, code=EREPEAT)

    w = BitWriter()
    dynamic_header(w, 257, 1, {1: 1, 18: 2, 0: 2}, [(1, 0), (1, 0), (18, 127), (18, 118 - 11)])   # 2 + 138 + 118 = 258, 256 has none
    out["bad_no_eob"] = Member(w.done() + bytes(16), 0, 0, code=ENOEOB)

    w = BitWriter()
    fixed_block(w, [("lit", 120), ("raw_l", 286)])
    out["bad_lit_symbol_286"] = Member(w.done() + bytes(4), 1, zlib.crc32(b"x"), code=ESYMBOL)
    w = BitWriter()
    fixed_block(w, [("lit", 120), ("lit", 121), ("lit", 122), ("raw_l", 257), ("raw_d", 30, 0, 0)])
    out["bad_dist_symbol_30"] = Member(w.done() + bytes(4), 6, 0, code=ESYMBOL)
    # bits that are no code: a distance code of one bit, and the other bit sent
    w = BitWriter()
    dynamic_block(w, complete_lengths(258), [1], [("lit", 65), ("raw_l", 257)], eob=False)
    w.bits(1, 1)   # the distance code has only "0"
    w.bits(0, 30)
    out["bad_unassigned_code"] = Member(w.done() + bytes(4), 4, 0, code=ESYMBOL)

    out["bad_distance_too_far"] = Member(fixed_stream([("lit", 97), ("raw_l", 257), ("raw_d", 1, 0, 0)]), 4, 0, code=EDIST)
    out["bad_distance_at_start"] = Member(fixed_stream([("raw_l", 257), ("raw_d", 0, 0, 0)]), 3, 0, code=EDIST)

    out["bad_isize_small"] = Member(good, len(good_text) - 1, crc, code=EPAST)
    out["bad_isize_large"] = Member(good, len(good_text) + 1, crc, code=ESHORT)
    out["bad_isize_zero"] = Member(good, 0, crc, code=EPAST)
    out["bad_match_past_isize"] = Member(fixed_stream([("lit", 97), ("match", 258, 1)]), 200, 0, code=EPAST)
    out["bad_stored_past_isize"] = Member(deflate_raw(b"0123456789", 0), 9, zlib.crc32(b"012345678"), code=EPAST)
    out["bad_truncated"] = Member(good[:len(good) // 2], len(good_text), crc, code=EINPUT)
    out["bad_truncated_stored"] = Member(deflate_raw(b"0123456789", 0)[:-3], 10, zlib.crc32(b"0123456789"), code=EINPUT)
    out["bad_empty_payload"] = Member(b"", 0, 0, code=EINPUT)
    out["bad_not_final"] = Member(deflate_raw(b"abc", 6, flush_at=(3,))[:-2], 3, zlib.crc32(b"abc"), code=EINPUT)   # ends after a sync flush
    out["bad_crc"] = Member(good, len(good_text), crc ^ 0x00010000, code=ECRC)
    big = bytes(65537)
    out["bad_isize_65537"] = Member(deflate_raw(big, 6), 65537, zlib.crc32(big), code=EISIZE)
    return out


def truncations():
    """One small member cut at every byte of its payload (the member itself stays whole)."""
    text = b"truncate me, truncate me again: " * 3 + bytes(range(40))
    payload = deflate_raw(text, 9)
    return text, payload, [Member(payload[:k], len(text), zlib.crc32(text)) for k in range(len(payload))]


def kinds_cases():
    out = {}
    fq = fastq_text(1, 65280)
    out["stored_level0"] = wrap(random_bytes(2, 1000), 0)
    t = fastq_text(3, 2000)
    out["stored_empty_sync"] = [member_of(t, deflate_raw(t, 6, flush_at=(700,)))]
    out["stored_65280"] = wrap(random_bytes(4, 65280), 0)
    for n in (0, 1, 2, 3):
        out["fixed_%d" % n] = [member_of(b"xyz"[:n], deflate_raw(b"xyz"[:n], 6, zlib.Z_FIXED))]
    out["fixed_text"] = wrap(fastq_text(6, 3000), 6, zlib.Z_FIXED)
    for lvl in (1, 6, 9):
        out["dynamic_l%d" % lvl] = wrap(fq, lvl)
    out["huffman_only"] = wrap(fq[:20000], 6, zlib.Z_HUFFMAN_ONLY)
    out["rle"] = wrap((b"aaaaaaaaaaaaaaaabbbbbbbbbbbbbbbbbbbbbbbbbcccccccccccccccd" * 300 + fq[:5000]), 6, zlib.Z_RLE)
    t = fastq_text(7, 30000)
    out["multi_full_flush"] = [member_of(t, deflate_raw(t, 6, flush_at=(5000, 5001, 20000), flush=zlib.Z_FULL_FLUSH))]
    out["multi_sync_flush"] = [member_of(t, deflate_raw(t, 6, flush_at=(1, 9000, 9000, 29999)))]
    out["eof_at_end"] = wrap(fq[:5000], 6) + [EOF_MEMBER]
    out["eof_in_middle"] = wrap(fq[:5000], 6) + [EOF_MEMBER] + wrap(fq[5000:9000], 1) + [EOF_MEMBER, EOF_MEMBER]
    out["trailing_bytes_in_payload"] = [member_of(fq[:900], deflate_raw(fq[:900], 6) + b"\xff\x00garbage")]
    return out


def size_cases():
    out = {}
    out["isize_0"] = [member_of(b"", deflate_raw(b"", 6)), EOF_MEMBER, member_of(b"", deflate_raw(b"", 0))]
    out["isize_1"] = [member_of(b"\n", deflate_raw(b"\n", 6)), member_of(b"\xff", deflate_raw(b"\xff", 0))]
    out["isize_65280"] = wrap(fastq_text(8, 65280), 6)
    t = fastq_text(9, 65536)
    out["isize_65536"] = [member_of(t, deflate_raw(t, 6)), member_of(t, deflate_raw(t, 1))]
    return out


def hand_cases():
    out = {}
    out["hand_all_codes"] = [_member_from_ops(hand_all_codes())]
    out["hand_edges"] = [_member_from_ops(hand_edges())]
    out["hand_far"] = [_member_from_ops(hand_far())]
    return out


def header_cases():
    out = {}
    # a code of 1, 2, ..., 14, 15 and 15 bits: 'A'..'O' and the end-of-block code
    lit = [0] * 257
    for i in range(15):
        lit[65 + i] = i + 1
    lit[256] = 15
    ops = [("lit", 65 + (i * i) % 15) for i in range(400)] + [("lit", 79), ("lit", 78), ("lit", 79)]
    out["dyn_15_bit_code"] = [_member_from_ops(ops, (lit, [0]))]
    # one distance code, of one bit, used (the incomplete set deflate allows)
    ops = [("lit", 120), ("match", 5, 1), ("lit", 121), ("match", 3, 1), ("match", 4, 1)]
    out["dyn_one_distance_code"] = [_member_from_ops(ops, (complete_lengths(260), [1]))]
    text_ops = [("lit", c) for c in b"minimum header"]
    out["dyn_min"] = [_member_from_ops(text_ops, (complete_lengths(257), [1]))]   # 257 codes: no length code exists
    out["dyn_min_nodist"] = [_member_from_ops(text_ops, (complete_lengths(257), [0]))]
    ops = [("lit", 33 + i) for i in range(64)]
    _grow(ops, 64, 24577 + 300)
    ops += [("match", 258, 24577), ("match", 257, 24700, 27), ("match", 258, 24578), ("lit", 255)]
    out["dyn_max"] = [_member_from_ops(ops, (complete_lengths(286), complete_lengths(30)))]
    # the repeat codes one by one: literal/length lengths with runs of equal values and of zeros
    lit = [8] * 254 + [9, 9, 9, 10] + [0] * 19 + [10]
    dist = [0, 0, 0, 2, 2, 2, 2]
    ops = [("lit", c) for c in b"repeat codes "] + [("match", 3, 4), ("match", 70, 7), ("match", 82, 12)]
    for use in ((16,), (17,), (18,), (16, 17, 18)):
        out["dyn_repeat_" + "_".join(map(str, use))] = [_dyn_with(use, lit, dist, ops)]
    # repeats that run from the literal/length lengths into the distance lengths: zeros (18), and equal lengths (16)
    lit = [8] * 254 + [9, 9, 9, 10, 10] + [0] * 20
    dist = [0] * 8 + [1, 1]
    out["dyn_repeat_crossing_18"] = [_dyn_with((18,), lit, dist, [("lit", c) for c in b"crossing zeros, twice over"] + [("match", 4, 17), ("match", 3, 30)])]
    out["dyn_repeat_crossing_16"] = [_dyn_cross16()]
    return out


def _dyn_cross16():
    # literal/length lengths end ... 9, 9 (254, 255, 256 -> 9, 9 and one more nine-bit pair), the distance lengths
    # begin 9, 9, 9, ...: a run of nines across the border, coded as 9 then repeats of code 16
    lit = [8] * 254 + [9, 9, 9, 9]            # 258 symbols: 254/256 + 4/512 = 1
    dist = [9, 9] + [1, 2, 3, 4, 5, 6, 7, 8]  # 2/512 + 255/256 = 1
    ops = [("lit", c) for c in b"crossing nines"] + [("match", 3, 2), ("match", 3, 1)]
    w = BitWriter()
    seq = lit + dist
    # hand-made coding: everything plain but the run over the border: lit[254..257] + dist[0..1] = six nines
    cl_ops = [(v, 0) for v in seq[:254]] + [(9, 0), (16, 5 - 3)] + [(v, 0) for v in seq[260:]]
    used = sorted({s for s, _ in cl_ops})
    cl_lens = dict(zip(used, complete_lengths(len(used))))
    dynamic_header(w, len(lit), len(dist), cl_lens, cl_ops)
    put_ops(w, ops + [("eob",)], canonical_codes(lit), canonical_codes(dist))
    return member_of(expand(ops), w.done())


def layout_cases():
    """Payloads at every offset mod 16 of the batch: the size of a second extra subfield (0, or 4 to 19 bytes) moves
    member i's payload to offset i mod 16."""
    t = fastq_text(11, 40000)
    ms, at = [], 0
    for i in range(16):
        piece = t[i * 2000:(i + 1) * 2000 + i]
        xpad = (i - at - 18) % 16
        xpad += 16 if 1 <= xpad <= 3 else 0
        ms.append(member_of(piece, deflate_raw(piece, 1 + i % 9), xpad=xpad, bc_first=i % 2 == 0))
        at += len(ms[-1].raw())
    return {"layout_xlen": ms}


def neighbour_case():
    """A bad block between good neighbours."""
    fq = fastq_text(12, 9000)
    a, c = wrap(fq[:4000], 6)[0], wrap(fq[4000:], 6)[0]
    bad = malformed_cases()["bad_distance_too_far"]
    return {"bad_between_good": [a, bad, c, malformed_cases()["bad_crc"], a]}


def all_cases():
    """{name: [Member, ...]}: every case as one batch."""
    out = {}
    out.update(kinds_cases())
    out.update(size_cases())
    out.update(hand_cases())
    out.update(header_cases())
    out.update(layout_cases())
    out.update({k: [v] for k, v in malformed_cases().items()})
    out["truncated_at_every_byte"] = truncations()[2]
    out.update(neighbour_case())
    return out


_CACHE = {}


def cases():
    if "all" not in _CACHE:
        _CACHE["all"] = all_cases()
    return _CACHE["all"]


def verdicts(members):
    """[(ok, text)] under the statement."""
    return [m.verdict() for m in members]


def write_cases(directory):
    os.makedirs(directory, exist_ok=True)
    for name, ms in cases().items():
        with open(os.path.join(directory, name + ".bgzf"), "wb") as f:
            for m in ms:
                f.write(m.raw())


if __name__ == "__main__":
    write_cases(sys.argv[1])

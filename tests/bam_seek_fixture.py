"""What a seeking bam-vaf-counter pass is tested with (include/vafc.h, item 9 of
the bam contract and "Many short record chains of one text"), struct and zlib
only:

  decode       a BGZF BAM as members, text and records with their virtual offsets
  write_bai    a BAI after the SAM specification, 5.2: reg2bin per record, the
               chunks of each bin, the linear index, the metadata pseudo-bin
  py_plan      a plain statement of the plan rule over the bytes of a BAI
  covered      the coverage property: every record that overlaps a region
               starts inside exactly one span
  walk_piece   a serial statement of the piece walk
  CLASSES      texts and pieces for the device's piece walk, one class per edge
  sorted_bam   a coordinate-sorted file of short records in small members

Importing it reads no file and needs no GPU.  Run as a program it writes the
piece classes as case files for the stand-alone checker
(tools/bam_index_check.cpp, tools/bam_index_asan.sh):
    python3 tests/bam_seek_fixture.py <dir>"""
import os
import struct
import sys
import zlib
from collections import namedtuple

import numpy as np

import bam_fixture as F
import bam_text_fixture as T
from bam_statement import count_records

META_BIN = 37450
MAX_POS = 1 << 29
OK, CUT, SHORT, NOROOM = 0, 1, 2, 3

Member = namedtuple("Member", "coff size toff isize")
Rec = namedtuple("Rec", "voff end_voff toff tid pos end")
Decoded = namedtuple("Decoded", "members text body refs recs size")


# ---------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------

def bgzf_var(text: bytes, sizes, eof: bool = True) -> bytes:
    """text in members whose text sizes cycle through `sizes`."""
    out, at, i = [], 0, 0
    while at < len(text):
        n = sizes[i % len(sizes)]
        out.append(F.bgzf_block(text[at:at + n]))
        at += n
        i += 1
    return b"".join(out) + (F.EOF_BLOCK if eof else b"")


def voff_of(members, t: int, size: int) -> int:
    """The virtual offset of text offset t: in the member that holds byte t,
    or at the start of whatever follows the last member."""
    lo, hi = 0, len(members)
    while lo < hi:
        mid = (lo + hi) // 2
        if members[mid].toff + members[mid].isize <= t:
            lo = mid + 1
        else:
            hi = mid
    if lo == len(members):
        return min(size, members[-1].coff + members[-1].size) << 16
    return members[lo].coff << 16 | (t - members[lo].toff)


def decode(raw: bytes) -> Decoded:
    members, parts, toff = [], [], 0
    for coff, size in F.bgzf_blocks(raw):
        text = zlib.decompress(raw[coff + 18:coff + size - 8], -15)
        if text:
            members.append(Member(coff, size, toff, len(text)))
        parts.append(text)
        toff += len(text)
    text = b"".join(parts)
    l_text, = struct.unpack_from("<i", text, 4)
    at = 12 + l_text
    refs = []
    for _ in range(struct.unpack_from("<i", text, at - 4)[0]):
        l_name, = struct.unpack_from("<i", text, at)
        refs.append(text[at + 4:at + 4 + l_name - 1].decode("latin-1"))
        at += 8 + l_name
    body, recs = at, []
    while at < len(text):
        bl, tid, pos, l_qname, _mapq, _bin, n_cigar = struct.unpack_from("<iiiBBHH", text, at)
        words = struct.unpack_from("<%dI" % n_cigar, text, at + 36 + l_qname)
        rlen = sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8))
        recs.append(Rec(voff_of(members, at, len(raw)), voff_of(members, at + 4 + bl, len(raw)), at, tid, pos, pos + (rlen or 1)))
        at += 4 + bl
    return Decoded(members, text, body, refs, recs, len(raw))


# ---------------------------------------------------------------------------
# the index
# ---------------------------------------------------------------------------

def write_bai(d: Decoded, meta: bool = True, no_coor: bool = True) -> bytes:
    """The BAI of a coordinate-sorted file.  A bin's chunks: runs of records of
    that bin that follow one another in the file.  The linear index: per 16 KB
    window the lowest offset of a record that overlaps it, windows no record
    overlaps taking the entry before them (as samtools fills them)."""
    out = [b"BAI\1", struct.pack("<i", len(d.refs))]
    unplaced = sum(1 for r in d.recs if r.tid < 0)
    for tid in range(len(d.refs)):
        bins, linear, last_bin = {}, [], None
        mine = [r for r in d.recs if r.tid == tid]
        for r in mine:
            b = F.reg2bin(r.pos, r.end)
            if b == last_bin:
                bins[b][-1][1] = r.end_voff
            else:
                bins.setdefault(b, []).append([r.voff, r.end_voff])
            last_bin = b
            for w in range(r.pos >> 14, ((r.end - 1) >> 14) + 1):
                if w >= len(linear):
                    linear += [0] * (w + 1 - len(linear))
                if linear[w] == 0:
                    linear[w] = r.voff
        for w in range(1, len(linear)):
            if linear[w] == 0:
                linear[w] = linear[w - 1]
        n_bin = len(bins) + (1 if meta and mine else 0)
        out.append(struct.pack("<i", n_bin))
        for b in sorted(bins):
            out.append(struct.pack("<Ii", b, len(bins[b])))
            for beg, end in bins[b]:
                out.append(struct.pack("<QQ", beg, end))
        if meta and mine:
            out.append(struct.pack("<IiQQQQ", META_BIN, 2, mine[0].voff, mine[-1].end_voff, len(mine), 0))
        out.append(struct.pack("<i", len(linear)))
        out.append(struct.pack("<%dQ" % len(linear), *linear))
    if no_coor:
        out.append(struct.pack("<Q", unplaced))
    return b"".join(out)


def parse_bai(raw: bytes, n_ref: int):
    """[(bins {bin: [(beg, end)]}, linear)] per reference, or None where the
    index is not usable for seeking."""
    at = 8
    if len(raw) < 8 or raw[:4] != b"BAI\1":
        return None
    n, = struct.unpack_from("<I", raw, 4)
    if n != n_ref:
        return None
    refs = []
    try:
        for _ in range(n):
            n_bin, = struct.unpack_from("<I", raw, at)
            at += 4
            if n_bin > (len(raw) - at) // 8:
                return None
            bins = {}
            for _b in range(n_bin):
                b, n_chunk = struct.unpack_from("<II", raw, at)
                at += 8
                if n_chunk > (len(raw) - at) // 16:
                    return None
                chunks = [struct.unpack_from("<QQ", raw, at + 16 * k) for k in range(n_chunk)]
                at += 16 * n_chunk
                if b == META_BIN:
                    continue
                if b in bins or any(e < s for s, e in chunks):
                    return None
                bins[b] = chunks
            n_intv, = struct.unpack_from("<I", raw, at)
            at += 4
            if n_intv > (len(raw) - at) // 8:
                return None
            linear = list(struct.unpack_from("<%dQ" % n_intv, raw, at))
            at += 8 * n_intv
            refs.append((bins, linear))
    except struct.error:
        return None
    return refs if len(raw) - at in (0, 8) else None


def reg2bins(beg: int, end: int):
    end -= 1
    out = [0]
    for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(base + (beg >> shift), base + (end >> shift) + 1)
    return out


def py_plan(index: bytes, n_ref: int, regions):
    """Item 9: regions [(tid, s, e)] -> [(beg, end)], or None."""
    refs = parse_bai(index, n_ref)
    if refs is None or any(e > MAX_POS for _t, _s, e in regions):
        return None
    chunks = []
    for tid, s, e in regions:
        bins, linear = refs[tid]
        min_off = linear[s >> 14] if s >> 14 < len(linear) else 0
        for b in reg2bins(s, e):
            chunks += [c for c in bins.get(b, ()) if c[1] > min_off]
    spans = []
    for beg, end in sorted(chunks):
        if spans and beg >> 16 <= spans[-1][1] >> 16:
            spans[-1][1] = max(spans[-1][1], end)
        else:
            spans.append([beg, end])
    return [tuple(s) for s in spans]


def wanted(d: Decoded, regions):
    """The records that overlap a region."""
    by_tid = {}
    for t, s, e in regions:
        by_tid.setdefault(t, []).append((s, e))
    return [r for r in d.recs if any(r.pos < e and r.end > s for s, e in by_tid.get(r.tid, ()))]


def covered(d: Decoded, regions, spans):
    """None if the spans ascend, are disjoint in members and every wanted
    record starts inside exactly one; else what is wrong."""
    for a, b in zip(spans, spans[1:]):
        if not (a[0] < a[1] and a[1] >> 16 < b[0] >> 16):
            return "spans %r and %r share a member or do not ascend" % (a, b)
    for r in wanted(d, regions):
        n = sum(1 for beg, end in spans if beg <= r.voff < end)
        if n != 1:
            return "the record at %#x (tid %d, pos %d) starts inside %d spans" % (r.voff, r.tid, r.pos, n)
    return None


def span_members(d: Decoded, spans):
    """The indices of the members a seeking pass reads for the spans."""
    at = {m.coff: i for i, m in enumerate(d.members)}
    out = set()
    for beg, end in spans:
        i = at[beg >> 16]
        while i < len(d.members) and d.members[i].coff <= end >> 16:
            out.add(i)
            i += 1
    return out


# ---------------------------------------------------------------------------
# the piece walk
# ---------------------------------------------------------------------------

def walk_piece(text: bytes, entry: int, stop: int, limit: int):
    """(status, offsets of the records walked, missing bytes)."""
    limit = min(limit, len(text))
    stop, o = min(stop, limit), min(entry, limit)
    found = []
    while o < stop:
        if limit - o < 4:
            return CUT, found, 0
        bl, = struct.unpack_from("<i", text, o)
        if bl < 32:
            return SHORT, found, 0
        if bl > limit - o - 4:
            return CUT, found, bl - (limit - o - 4)
        found.append(o)
        o += 4 + bl
    return OK, found, 0


PieceCase = namedtuple("PieceCase", "rows ref_names text pieces note")
PieceWant = namedtuple("PieceWant", "per_piece emitted recs irregular bases plain weighted n_short n_cut")


def expect_pieces(case: PieceCase) -> PieceWant:
    """per_piece: (status, found offsets, missing); emitted: the offsets of
    the OK pieces; recs / irregular: what the check makes of them."""
    per = [walk_piece(case.text, *p) for p in case.pieces]
    emitted = [o for st, found, _m in per if st == OK for o in found]
    recs, irregular = [], []
    for o in emitted:
        ok, rec = T.classify(case.text, o)
        (recs if ok else irregular).append(rec if ok else o)
    tid_of = {nm: i for i, nm in enumerate(case.ref_names)}
    tids = [tid_of.get(r[0], -1) for r in case.rows]
    regs = T.regions_of(T.Case(case.rows, case.ref_names, [], ""))
    return PieceWant(per, emitted, recs, irregular, sum(r[4] for r in recs), count_records(case.rows, tids, recs),
                     count_records(case.rows, tids, recs, regs), sum(1 for p in per if p[0] == SHORT),
                     sum(1 for p in per if p[0] == CUT))


def _records(seed, n, **kw):
    rng = np.random.default_rng(seed)
    return [T.rnd_record(rng, i, **kw) for i in range(n)]


def _pcase(text, pieces, note):
    return PieceCase(T.dense_rows(), T.NAMES, text, pieces, note)


def members_of_text(n: int, step: int):
    """Borders of members of `step` bytes of text: [0, step, ..., n]."""
    return list(range(0, n, step)) + [n]


def class_entry():
    recs = _records(61, 30)
    text, st = b"".join(recs), T.starts_of(recs)
    b = members_of_text(len(text), 300)
    mid = next(s for s in st if b[1] < s < b[2])
    assert 0 in st and mid not in b
    return _pcase(text, [(0, st[7], b[2]), (mid, st[20], len(text))], "entry at a member's byte 0 and in mid-member")


def class_stop():
    recs = _records(62, 20)
    text, st = b"".join(recs), T.starts_of(recs)
    return _pcase(text, [(st[2], st[9], len(text)), (st[2], st[9] + 1, len(text))],
                  "stop exactly on a record start (not taken) and one byte past it (taken)")


def class_straddle():
    recs = _records(63, 12)
    text, st = b"".join(recs), T.starts_of(recs)
    border = st[5] + 20                     # a member border inside record 5
    return _pcase(text, [(st[3], st[8], len(text)), (st[3], border + 1, len(text))],
                  "a record straddling a member border inside a piece (border at %d)" % border)


def class_cut():
    recs = _records(64, 10)
    text, st = b"".join(recs), T.starts_of(recs)
    last = st[6]
    pieces = [(st[1], last + 1, last + j) for j in (0, 1, 3, 4, 5, 36, len(recs[6]) - 1, len(recs[6]))]
    return _pcase(text, pieces, "the last wanted record running past limit, with 4 or more of its bytes and with fewer")


def class_empty():
    recs = _records(65, 10)
    text, st = b"".join(recs), T.starts_of(recs)
    n = len(text)
    return _pcase(text, [(st[3], st[3], n), (n + 50, n + 90, n), (st[4], st[2], n), (st[5], st[7], st[5]), (n + 5, n + 9, n + 99),
                         (st[1], st[3], n)], "empty pieces: entry == stop, entry > limit, entry > stop, limit == entry")


def class_adjacent():
    recs = _records(66, 40)
    text, st = b"".join(recs), T.starts_of(recs)
    n = len(text)
    return _pcase(text, [(st[2], st[15], n), (st[15], st[31], n), (st[31], n, n)],
                  "pieces where one's stop is the next one's entry: each record once")


def class_bad_entry():
    recs = _records(67, 16) + [F.record(0, 50, 0, [("M", 400)], "ACGT" * 100, name=b"big")] + _records(68, 6)
    text, st = b"".join(recs), T.starts_of(recs)
    n = len(text)
    q = st[16] + len(recs[16]) - 390        # inside the qualities: 0xff bytes, a negative block_size
    z = st[3] + 13                          # inside the fixed fields: mapq, bin, n_cigar read as a block_size
    # an entry 4 bytes into a record: tid and what follows read as a record whose fields do not fit
    odd = F.record(0, 1500, 0, [("M", 40)], "ACGT" * 10, name=b"odd", aux=b"XXZ" + b"a" * 60 + b"\0")
    odd = T.patched(odd, 4, struct.pack("<i", 40))      # tid 40 = a block_size of 40 for a walk that enters at byte 4
    bad = T.irregular_record("qlen")
    text2 = text + odd + bad + b"".join(_records(69, 3))
    pieces = [(q, n, n), (z, st[9], n), (st[1], st[4], n), (n + 4, n + 5, len(text2)), (n + len(odd), len(text2), len(text2))]
    case = _pcase(text2, pieces, "an entry that is no record start (short, cut or irregular) and an irregular record")
    per = [walk_piece(text2, *p) for p in pieces]
    assert per[0][0] == SHORT and per[3][0] == OK and not T.classify(text2, n + 4)[0] and per[4][0] == OK
    return case


def class_count(n_pieces: int):
    recs = _records(70 + n_pieces, 3 * n_pieces + 4)
    text, st = b"".join(recs), T.starts_of(recs)
    pieces = []
    for i in range(n_pieces):
        if i % 3 == 1:
            pieces.append((st[2 * i], st[2 * i], len(text)))                # an empty one between
        else:
            pieces.append((st[2 * i], st[2 * i + 2], len(text)))
    return _pcase(text, pieces, "%d pieces with empty ones between" % n_pieces)


def class_mod4():
    recs = _records(80, 48)
    pieces, parts, at = [], [], 0
    for shift in range(4):
        pad = b"\x07" * (shift + 1)
        parts.append(pad)
        at += len(pad)
        st = T.starts_of(recs[12 * shift:12 * shift + 12], at)
        body = b"".join(recs[12 * shift:12 * shift + 12])
        parts.append(body)
        pieces.append((st[0], st[-1] + 1, at + len(body)))
        at += len(body)
    text = b"".join(parts)
    assert {o % 4 for p in pieces for o in walk_piece(text, *p)[1]} == {0, 1, 2, 3}
    return _pcase(text, pieces, "records at every start offset mod 4")


def class_long():
    rng = np.random.default_rng(81)
    recs = _records(82, 6) + [T.rnd_record(rng, 7, n_ops=130, pos=100, tid=0), T.rnd_record(rng, 8, n_ops=70, pos=300, tid=1)] + \
        _records(83, 6)
    text, st = b"".join(recs), T.starts_of(recs)
    return _pcase(text, [(st[1], st[5], len(text)), (st[5], st[9], len(text)), (st[9], len(text), len(text))],
                  "long-CIGAR records above the long threshold inside a piece")


PIECE_COUNTS = (1, 63, 64, 65, 200)
CLASSES = {"entry": class_entry, "stop": class_stop, "straddle": class_straddle, "cut": class_cut, "empty": class_empty,
           "adjacent": class_adjacent, "bad_entry": class_bad_entry, "mod4": class_mod4, "long": class_long}
CLASSES.update({"n_%d" % n: (lambda n=n: class_count(n)) for n in PIECE_COUNTS})

_cases, _wants = {}, {}


def case_of(name: str) -> PieceCase:
    if name not in _cases:
        _cases[name] = CLASSES[name]()
    return _cases[name]


def want_of(name: str) -> PieceWant:
    if name not in _wants:
        _wants[name] = expect_pieces(case_of(name))
    return _wants[name]


# ---------------------------------------------------------------------------
# a sorted file
# ---------------------------------------------------------------------------

SORTED_REFS = [("chr1", 1 << 28), ("chr2", 1 << 28)]
SORTED_REGIONS = [(0, 40_000, 41_500), (0, 9_000_000, 9_002_000), (1, 70_000_000, 70_001_000)]
SORTED_SIZES = (400, 1024, 777, 512, 911)


def sorted_records(seed: int = 7, n: int = 3000, clusters=None):
    """n short records in coordinate order: clusters around the regions and a
    thin spread over both references between them."""
    rng = np.random.default_rng(seed)
    clusters = SORTED_REGIONS if clusters is None else clusters
    where = []
    for tid, s, e in clusters:
        where += [(tid, int(p)) for p in rng.integers(max(0, s - 300), e + 100, n // (4 * len(clusters)))]
    while len(where) < n:
        where.append((int(rng.integers(0, 2)), int(rng.integers(0, (1 << 28) - 1000))))
    where.sort()
    out = []
    for i, (tid, pos) in enumerate(where):
        cigar = F.random_cigar(rng, int(rng.integers(1, 5)), 40, ops="MMMM=XIDS")
        seq = "".join("ACGT"[j] for j in rng.integers(0, 4, F.query_len(cigar)))
        out.append(F.record(tid, pos, 0, cigar, seq, name=b"s%d" % i))
    return out


def sorted_rows(regions=None, refs=None):
    """A panel whose merged regions are `regions`: every position of each."""
    regions = SORTED_REGIONS if regions is None else regions
    refs = SORTED_REFS if refs is None else refs
    rows = []
    for tid, s, e in regions:
        rows += [(refs[tid][0], p, "ACGT"[p % 4], "ACGT"[(p + 1 + p % 3) % 4]) for p in range(s, e)]
    return rows


def sorted_bam(records=None, sizes=SORTED_SIZES, refs=None) -> bytes:
    records = sorted_records() if records is None else records
    return bgzf_var(F.header(SORTED_REFS if refs is None else refs) + b"".join(records), sizes)


# ---------------------------------------------------------------------------
# case files for the stand-alone checker
# ---------------------------------------------------------------------------

def piece_case_file(case: PieceCase, want: PieceWant) -> bytes:
    """magic, n_pieces, text_len; per piece entry, stop, limit, then status,
    found, missing; then the text."""
    out = [struct.pack("<4sIQ", b"VBP1", len(case.pieces), len(case.text))]
    for p, (st, found, missing) in zip(case.pieces, want.per_piece):
        out.append(struct.pack("<QQQIIQ", p[0], p[1], p[2], st, len(found), missing))
    return b"".join(out) + case.text


def write_cases(dst: str) -> int:
    for name in CLASSES:
        with open(os.path.join(dst, "%s.vbp" % name), "wb") as f:
            f.write(piece_case_file(case_of(name), want_of(name)))
    return len(CLASSES)


if __name__ == "__main__":
    print("%d cases" % write_cases(sys.argv[1]))

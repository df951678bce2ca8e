"""Texts for the device's BAM text scan (vc_bam_scan_text_*, csrc/vafc_bam_text.h),
one class per edge, and a plain-Python statement of what a scan must report.

A class is a set of scans of texts built with bam_fixture.record: (text, entry,
cuts, final).  The statement walks a text serially: a record is a block_size
>= 32 that lies whole inside the text, the walk stops at a smaller block_size
and at a record the text cuts off, and a record found is regular or irregular
by the tests of the host reader (include/vafc.h, "Records found, checked and
counted in inflated BAM text").  The expected counts are
bam_statement.count_records over the regular records; tests/test_bam_text_fixture.py
shows that these are the records tests/test_bam.py's read_bam_py yields.

Run as a program it writes every scan as a case file for the stand-alone
checker (tools/bam_text_check.cpp, tools/bam_text_asan.sh):
    python3 tests/bam_text_fixture.py <dir>
Importing it reads no file and needs no GPU."""
import os
import struct
import sys
from collections import namedtuple

import numpy as np

import bam_fixture as F
from bam_statement import QUERY_OPS, count_records, py_build_regions

NONE = 0xFFFFFFFFFFFFFFFF
CHAIN = 3                    # VBT_CHAIN: plausible records in a row that make a guess
ROW_MAX = (1 << 31) - 2      # the largest row start a pattern file may carry

# rewalk: None = unstated, "zero" = every segment starts at a record start,
# "some" = a guess is known to be wrong
Scan = namedtuple("Scan", "text entry cuts final rewalk")
Case = namedtuple("Case", "rows ref_names scans note")

NAMES = ["chr1", "chr2"]


# ---------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------

def fields_fit(text, o, bl):
    l_qname = text[o + 12]
    n_cigar, = struct.unpack_from("<H", text, o + 16)
    l_seq, = struct.unpack_from("<i", text, o + 20)
    return l_seq >= 0 and l_qname >= 1 and 4 * n_cigar + l_qname + (l_seq + 1) // 2 + l_seq <= bl - 32


def classify(text, o):
    """The record found at o: (True, (tid, pos, flag, words, l_seq, bases)) or
    (False, why)."""
    bl, tid, pos, l_qname, _mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiiBBHHHi", text, o)
    if l_seq < 0:
        return False, "l_seq"
    if l_qname < 1:
        return False, "name"
    if not fields_fit(text, o, bl):
        return False, "fit"
    at = o + 36 + l_qname
    words = list(struct.unpack_from("<%dI" % n_cigar, text, at))
    has_aux = 4 * n_cigar + l_qname + (l_seq + 1) // 2 + l_seq < bl - 32
    if words and words[0] == (l_seq << 4 | 4) & 0xFFFFFFFF and tid >= 0 and pos >= 0 and has_aux:
        return False, "cg"              # the CG tag may lie in the aux bytes: the host reader looks
    if words and l_seq > 0 and not flag & 4 and sum(w >> 4 for w in words if (w & 15) in QUERY_OPS) != l_seq:
        return False, "qlen"
    return True, (tid, pos, flag, words, l_seq, bytes(text[at + 4 * n_cigar:at + 4 * n_cigar + (l_seq + 1) // 2]))


Walk = namedtuple("Walk", "consumed found recs irregular short_stop bases")


def walk_text(text, entry, final) -> Walk:
    """found: offsets of all records; recs: the regular ones; irregular:
    offsets, the final piece's cut record whose fields do not fit among them."""
    o, found, stop = entry, [], None
    while o < len(text):
        if len(text) - o < 4:
            stop = "fit"
            break
        bl, = struct.unpack_from("<i", text, o)
        if bl < 32:
            stop = "short"
            break
        if bl > len(text) - o - 4:
            stop = "fit"
            break
        found.append(o)
        o += 4 + bl
    recs, irregular = [], []
    for f in found:
        ok, rec = classify(text, f)
        if ok:
            recs.append(rec)
        else:
            irregular.append(f)
    if final and stop == "fit" and len(text) - o >= 36 and not fields_fit(text, o, struct.unpack_from("<i", text, o)[0]):
        irregular.append(o)
    return Walk(o, found, recs, irregular, stop == "short", sum(r[4] for r in recs))


def plausible(text, o, n_ref):
    """The guess's rule at o < len(text): (ok, where the chain goes on)."""
    n = len(text)
    if n - o < 4:
        return True, n
    bl, = struct.unpack_from("<i", text, o)
    if bl < 32:
        return False, n
    nxt = o + 4 + bl
    if n - o < 36:
        return True, nxt
    tid, pos = struct.unpack_from("<ii", text, o + 4)
    next_tid, = struct.unpack_from("<i", text, o + 24)
    if not (-1 <= tid < n_ref and -1 <= next_tid < n_ref and pos >= -1):
        return False, nxt
    if not fields_fit(text, o, bl):
        return False, nxt
    nul = o + 36 + text[o + 12] - 1
    return nul >= n or text[nul] == 0, nxt


def guess(text, a, b, n_ref):
    """The first offset of [a, b) with CHAIN plausible records in a row, or
    fewer that leave the segment; None without one."""
    for o in range(a, b):
        p, ok = o, True
        for _ in range(CHAIN):
            ok, nxt = plausible(text, p, n_ref)
            if not ok or nxt >= b:
                break
            p = nxt
        if ok:
            return o
    return None


def segments(scan: Scan):
    edges = [0] + [min(c, len(scan.text)) for c in scan.cuts] + [len(scan.text)]
    return [(a, max(a, b)) for a, b in zip(edges, edges[1:])]


# ---------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------

def dense_rows(step=3, top=2400):
    rows = []
    for c in NAMES:
        for p in range(0, top, step):
            rows.append((c, p, "ACGT"[(p // step) % 4], "ACGT"[(p // step + 1 + p % 3) % 4]))
    return rows


def rnd_record(rng, i, n_ops=None, flag=0, tid=None, pos=None, name=None, aux=b""):
    n_ops = int(rng.integers(1, 7)) if n_ops is None else n_ops
    cigar = F.random_cigar(rng, n_ops, 9 if n_ops < 60 else 3) if n_ops else []
    l_seq = F.query_len(cigar) if cigar else int(rng.integers(1, 30))
    seq = "".join("ACGT"[j] for j in rng.integers(0, 4, l_seq))
    tid = int(rng.integers(0, 2)) if tid is None else tid
    pos = int(rng.integers(0, 2300)) if pos is None else pos
    name = (b"q%d" % i) + b"x" * (i % 4) if name is None else name     # the names move the CIGAR through every offset mod 4
    return F.record(tid, pos, flag, cigar, seq, name=name, aux=aux)


def starts_of(records, at=0):
    out = []
    for r in records:
        out.append(at)
        at += len(r)
    return out


def patched(rec: bytes, off: int, data: bytes) -> bytes:
    return rec[:off] + data + rec[off + len(data):]


def member_cuts(n: int, step: int):
    return list(range(step, n, step))


def _case(scans, note, rows=None, names=None):
    return Case(dense_rows() if rows is None else rows, NAMES if names is None else names, scans, note)


# ---------------------------------------------------------------------------
# the classes
# ---------------------------------------------------------------------------

def class_mod4(long_ops: bool):
    rng = np.random.default_rng(41 + long_ops)
    scans = []
    for shift in range(4):
        recs = [rnd_record(rng, i, n_ops=(70, 130, 65)[i % 3] if long_ops else None) for i in range(24)]
        text = b"\x07" * shift + b"".join(recs)
        st = starts_of(recs, shift)
        assert {s % 4 for s in st} == {0, 1, 2, 3}
        scans.append(Scan(text, shift, st[3::5], True, "zero" if shift == 0 else None))
        scans.append(Scan(text, shift, member_cuts(len(text), 500 if long_ops else 97), True, None))
    return _case(scans, "record starts and CIGARs at every offset mod 4, %s CIGARs" % ("long" if long_ops else "short"))


def class_cut_in_head():
    rng = np.random.default_rng(43)
    recs = [rnd_record(rng, i) for i in range(9)]
    text, st = b"".join(recs), starts_of(recs)
    scans = [Scan(text, 0, [st[4] + j], True, None) for j in range(1, 36)]
    scans += [Scan(text, 0, [st[2] + j, st[4] + (j * 7) % 36, st[7] + 35 - j], True, None) for j in range(1, 36)]
    return _case(scans, "a cut inside each of the 36 leading bytes of a record")


def class_cut_at_start():
    rng = np.random.default_rng(44)
    recs = [rnd_record(rng, i) for i in range(40)]
    text, st = b"".join(recs), starts_of(recs)
    return _case([Scan(text, 0, st[1:], True, "zero"), Scan(text, 0, st[5::7], True, "zero"),
                  Scan(text, st[3], st[5::7], True, None)], "every cut exactly at a record start")


def class_span_three():
    rng = np.random.default_rng(45)
    big = rnd_record(rng, 99, n_ops=40, pos=100)
    recs = [rnd_record(rng, i) for i in range(5)] + [big] + [rnd_record(rng, i) for i in range(5, 10)]
    text, st = b"".join(recs), starts_of(recs)
    a = st[5]
    assert len(big) > 200
    return _case([Scan(text, 0, [a + 60, a + 120], True, None), Scan(text, 0, [a - 10, a + 40, a + len(big) - 5], True, None)],
                 "a record spanning three segments")


def class_no_start():
    rng = np.random.default_rng(46)
    big = F.record(0, 50, 0, [("M", 400)], "ACGT" * 100, name=b"big")
    recs = [rnd_record(rng, i) for i in range(4)] + [big] + [rnd_record(rng, i) for i in range(4, 8)]
    text, st = b"".join(recs), starts_of(recs)
    q = st[4] + len(big) - 390            # inside the qualities (0xff: no block_size)
    sc = Scan(text, 0, [q, q + 300], True, None)
    assert guess(text, q, q + 300, 2) is None
    return _case([sc], "a segment with no record start and no guess")


def class_tiny_segments():
    rng = np.random.default_rng(47)
    recs = [rnd_record(rng, i) for i in range(30)]
    text, st = b"".join(recs), starts_of(recs)
    scans = []
    for s in (st[3], st[3] + 2, st[10] + 17):
        scans.append(Scan(text, 0, [s, s + 1, s + 36, s + 72, s + 109], True, None))      # 1, 35, 36, 37 bytes
    scans.append(Scan(text, 0, list(range(1, 600)), True, None))
    return _case(scans, "segments of 1, 35, 36 and 37 bytes")


def decoy_chain(n=4):
    """n whole record images that pass the plausibility rule, back to back."""
    return b"".join(F.record(0, 7 + i, 0, [("M", 2)], "AC", name=b"d") for i in range(n))


def class_decoy(where: str):
    rng = np.random.default_rng(48)
    dc = decoy_chain()
    if where == "qual":
        l_seq = len(dc) + 20
        host = F.record(1, 30, 0, [("M", l_seq)], "ACGT" * (l_seq // 4), name=b"host")
        at = len(host) - l_seq + 9         # inside the qualities
        host = patched(host, at, dc)
    else:
        aux = b"XBBC" + struct.pack("<I", len(dc) + 8) + b"\x01" * 3 + dc + b"\x01" * 5
        host = F.record(1, 30, 0, [("M", 8)], "ACGTACGT", name=b"host", aux=aux)
        at = host.index(dc)
    recs = [rnd_record(rng, i) for i in range(6)] + [host] + [rnd_record(rng, i) for i in range(6, 14)]
    text, st = b"".join(recs), starts_of(recs)
    d = st[6] + at
    scans = [Scan(text, 0, [d, st[10]], True, "some"), Scan(text, 0, [st[2], d], True, "some")]
    for sc in scans:
        assert guess(sc.text, d, segments(sc)[sc.cuts.index(d) + 1][1], 2) == d
    return _case(scans, "a plausible chain of record images inside %s, at a segment's start" % (
        "the qualities" if where == "qual" else "an aux B array"))


def class_n_ref0():
    rng = np.random.default_rng(49)
    recs = [rnd_record(rng, i, tid=-1, pos=-1) for i in range(20)]
    text = b"".join(recs)
    return _case([Scan(text, 0, starts_of(recs)[2::3], True, "zero"), Scan(text, 0, member_cuts(len(text), 64), True, None)],
                 "a header without references: every tid is -1", names=[])


def class_fields():
    """tid = -1, n_cigar = 0, l_seq = 0, pos at 2^31 - 1, flags 0x4, 0x200, 0x400."""
    rng = np.random.default_rng(50)
    recs = []
    for i in range(60):
        k = i % 10
        if k == 0:
            recs.append(rnd_record(rng, i, tid=-1))
        elif k == 1:
            recs.append(rnd_record(rng, i, n_ops=0))
        elif k == 2:
            recs.append(F.record(0, 40 + i, 0, [("M", 10)], "", name=b"noseq"))               # l_seq = 0 beside a CIGAR
        elif k == 3:
            recs.append(F.record(1, 40 + i, 0, [], "", name=b"nothing"))
        elif k == 4:
            recs.append(F.record(0, (1 << 31) - 1, 0, [("M", 3)], "ACG", name=b"top"))
        elif k == 5:
            recs.append(F.record(0, ROW_MAX - 2, 0, [("M", 5)], "ACGTA", name=b"top2"))
        elif k == 6:
            recs.append(rnd_record(rng, i, flag=(0x4, 0x200, 0x400)[i // 10 % 3]))
        elif k == 7:
            recs.append(F.record(0, 10 + i, 0x4, [("M", 20), ("I", 2)], "ACGT" * 5, name=b"unmapped"))   # 0x4: no length test
        else:
            recs.append(rnd_record(rng, i))
    text, st = b"".join(recs), starts_of(recs)
    rows = dense_rows() + [("chr1", ROW_MAX, "G", "C"), ("chr1", ROW_MAX - 1, "T", "C")]
    return _case([Scan(text, 0, st[1::4], True, "zero"), Scan(text, 0, member_cuts(len(text), 211), True, None)],
                 "tid -1, n_cigar 0, l_seq 0, pos 2^31 - 1, flags 0x4 0x200 0x400", rows=rows)


def irregular_record(kind: str) -> bytes:
    good = F.record(0, 1500, 0, [("M", 20)], "ACGT" * 5, name=b"bad")
    if kind == "fit":
        return F.record(0, 1500, 0, [("M", 20)], "ACGT" * 5, name=b"bad", l_seq=4000)
    if kind == "name":
        return patched(good, 12, b"\0")
    if kind == "l_seq":
        return patched(good, 20, struct.pack("<i", -1))
    if kind == "qlen":
        return F.record(0, 1500, 0, [("M", 20), ("I", 2)], "ACGT" * 5, name=b"bad")
    if kind == "cg":
        return F.record(0, 1500, 0, [("S", 20), ("N", 30)], "ACGT" * 5, name=b"bad", aux=b"NMC\x01")
    if kind == "bs8":
        return F.record(0, 1500, 0, [("M", 4)], "ACGT", name=b"bs8", block_size=8)
    raise KeyError(kind)


IRREGULAR = ("fit", "name", "l_seq", "qlen", "cg", "bs8")


def class_irregular(kind: str):
    rng = np.random.default_rng(51)
    recs = [rnd_record(rng, i) for i in range(30)]
    bad = irregular_record(kind)
    parts = recs[:17] + [bad] + recs[17:]
    text, st = b"".join(parts), starts_of(parts)
    scans = [Scan(text, 0, st[4::5], True, None), Scan(text, 0, member_cuts(len(text), 150), True, None),
             Scan(text, 0, [], False, None)]
    if kind != "bs8":
        two = b"".join(recs[:5] + [bad] + recs[5:9] + [bad] + recs[9:])
        scans.append(Scan(two, 0, member_cuts(len(two), 120), True, None))
    return _case(scans, "an irregular record (%s) in the middle of good ones" % kind)


def class_last_cut():
    rng = np.random.default_rng(52)
    recs = [rnd_record(rng, i) for i in range(6)]
    last = F.record(0, 33, 0, [("M", 8)], "ACGTACGT", name=b"z")
    head = b"".join(recs)
    scans = []
    for j in range(0, len(last)):
        for final in (True, False):
            scans.append(Scan(head + last[:j], 0, [len(head)] if j % 2 else member_cuts(len(head) + j, 70), final, None))
    # the cut record's fields do not fit: the host reader drops it and reads on, so it is irregular when final
    bad = irregular_record("fit")
    for j in (36, 40, len(bad) - 1):
        for final in (True, False):
            scans.append(Scan(head + bad[:j], 0, [len(head)], final, None))
    return _case(scans, "a last record cut at every byte, as a final and as a non-final piece")


def class_count(n: int):
    rng = np.random.default_rng(53 + n)
    recs = [rnd_record(rng, i, n_ops=(70 if i % 97 == 5 else None)) for i in range(n)]
    text, st = b"".join(recs), starts_of(recs)
    scans = [Scan(text, 0, member_cuts(len(text), 1024), True, None)]
    if n:
        scans.append(Scan(text, 0, st[1::16], True, "zero"))
    return _case(scans, "%d records" % n, rows=dense_rows(step=11))


COUNTS = (0, 1, 63, 64, 65, 2000)

CLASSES = {
    "mod4_short": lambda: class_mod4(False),
    "mod4_long": lambda: class_mod4(True),
    "cut_in_head": class_cut_in_head,
    "cut_at_start": class_cut_at_start,
    "span_three": class_span_three,
    "no_start": class_no_start,
    "tiny_segments": class_tiny_segments,
    "decoy_qual": lambda: class_decoy("qual"),
    "decoy_aux": lambda: class_decoy("aux"),
    "n_ref0": class_n_ref0,
    "fields": class_fields,
    "last_cut": class_last_cut,
}
CLASSES.update({"irr_" + k: (lambda k=k: class_irregular(k)) for k in IRREGULAR})
CLASSES.update({"n_%d" % n: (lambda n=n: class_count(n)) for n in COUNTS})

_cases = {}


def case_of(name: str) -> Case:
    if name not in _cases:
        _cases[name] = CLASSES[name]()
    return _cases[name]


def row_tids(case: Case):
    tid_of = {nm: i for i, nm in enumerate(case.ref_names)}
    return [tid_of.get(r[0], -1) for r in case.rows]


def regions_of(case: Case):
    tid_of = {nm: i for i, nm in enumerate(case.ref_names)}
    return [(tid_of[c], s, e) for c, s, e in py_build_regions(case.rows) if c in tid_of]


_expected = {}


def expected(name: str):
    """Per scan of the class: (Walk, plain counts, weighted counts); computed once."""
    if name not in _expected:
        case = case_of(name)
        tids, regs = row_tids(case), regions_of(case)
        out, memo = [], {}
        for sc in case.scans:
            key = (sc.text, sc.entry, sc.final)
            if key not in memo:
                w = walk_text(sc.text, sc.entry, sc.final)
                memo[key] = (w, count_records(case.rows, tids, w.recs), count_records(case.rows, tids, w.recs, regs))
            out.append(memo[key])
        _expected[name] = out
    return _expected[name]


# ---------------------------------------------------------------------------
# case files for the stand-alone checker
# ---------------------------------------------------------------------------

REWALK = {None: 0, "zero": 1, "some": 2}


def case_file(case: Case, sc: Scan, w: Walk) -> bytes:
    """magic, n_ref, final, rewalk rule, entry, n_cuts, text_len, then what the
    scan must report, the cuts, the offsets of the records found, the text."""
    head = struct.pack("<4siIIQQQ", b"VBT1", len(case.ref_names), 1 if sc.final else 0, REWALK[sc.rewalk], sc.entry,
                       len(sc.cuts), len(sc.text))
    want = struct.pack("<QQQQIII4x", w.consumed, len(w.recs), w.bases, min(w.irregular) if w.irregular else NONE,
                       len(w.irregular), 1 if w.short_stop else 0, len(w.found))
    return head + want + struct.pack("<%dQ" % len(sc.cuts), *sc.cuts) + struct.pack("<%dI" % len(w.found), *w.found) + sc.text


def write_cases(dst: str) -> int:
    n = 0
    for name in CLASSES:
        case = case_of(name)
        for i, (sc, (w, _p, _q)) in enumerate(zip(case.scans, expected(name))):
            with open(os.path.join(dst, "%s.%03d.vbt" % (name, i)), "wb") as f:
                f.write(case_file(case, sc, w))
            n += 1
    return n


if __name__ == "__main__":
    print("%d cases" % write_cases(sys.argv[1]))

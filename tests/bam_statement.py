"""The counting part of the bam-vaf-counter contract (include/vafc.h, items 2
to 6) as plain Python over records (tid, pos, flag, CIGAR words, l_seq, packed
bases), and the helpers that hand the same records and rows to a BamCounter.
tests/test_bam.py pins it to the reference's goldens through its own BAM
reader; tests/test_bam_edges*.py use it on records built by hand.  Importing
this module reads no file and needs no GPU."""
import struct

import numpy as np

import bam_fixture as F

SKIP = 0x4 | 0x200 | 0x400
REF_OPS, QUERY_OPS, MATCH_OPS = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8), (0, 7, 8)


def rec_end(rec):
    rlen = sum(w >> 4 for w in rec[3] if (w & 15) in REF_OPS)
    return rec[1] + (rlen or 1)


def walk(rec, row_pos):
    """Item 3 for one row: ("base", letter, op before the match block), ("gap",
    op) inside D / N, or None."""
    _tid, pos, _flag, words, l_seq, seq = rec
    cur, rp, prev = pos, 0, None
    for w in words:
        op, n = w & 15, w >> 4
        if op in MATCH_OPS:
            if cur <= row_pos < cur + n:
                q = rp + row_pos - cur
                if q >= l_seq:          # item 8: past the bases, nothing counts
                    return None
                nib = seq[q >> 1] & 15 if q & 1 else seq[q >> 1] >> 4
                return ("base", F.NT16[nib], prev)
            cur += n
            rp += n
        elif op in (1, 4):
            rp += n
        elif op in (2, 3):
            if cur <= row_pos < cur + n:
                return ("gap", op)
            cur += n
        prev = op
    return None


def py_build_regions(rows):
    """build_regions: rows [(chr, pos, ...)] -> [(chr, start, end)]."""
    regs = sorted((r[0], r[1], r[1] + 1) for r in rows)
    out = []
    for chr_, s, e in regs:
        if out and out[-1][0] == chr_ and out[-1][2] >= s:
            out[-1][2] = max(out[-1][2], e)
        else:
            out.append([chr_, s, e])
    return [tuple(r) for r in out]


def count_records(rows, row_tid, recs, regions=None, counts=None, tally=None):
    """Items 2 to 6 over records; regions: [(tid, start, end)] of this file or
    None (w = 1).  counts: uint32[2 * rows], wrapping."""
    counts = np.zeros(2 * len(rows), np.uint32) if counts is None else counts
    by_tid = {}
    for i, t in enumerate(row_tid):
        if t >= 0:
            by_tid.setdefault(t, []).append(i)
    for rec in recs:
        tid, pos, flag = rec[:3]
        if flag & SKIP or tid < 0:
            continue
        end = rec_end(rec)
        w = 1 if regions is None else sum(1 for t, s, e in regions if t == tid and pos < e and end > s)
        if w == 0:
            continue
        for i in by_tid.get(tid, ()):
            if not pos <= rows[i][1] < end:
                continue
            got = walk(rec, rows[i][1])
            if tally is not None and got is not None:
                key = got[0] + str(got[2] if got[0] == "base" else got[1])
                tally[key] = tally.get(key, 0) + 1
            if got is None or got[0] != "base":
                continue
            if got[1] == rows[i][2] or got[1] == rows[i][3]:
                k = 2 * i + (got[1] != rows[i][2])
                counts[k] = (int(counts[k]) + w) & 0xFFFFFFFF
                if tally is not None:
                    tally["hit%s" % got[2]] = tally.get("hit%s" % got[2], 0) + 1
    return counts


def pack(recs):
    """Records of the statement -> (vc_bam_rec array, data)."""
    import vafc
    out = np.zeros(len(recs), vafc.BAM_REC)
    data = bytearray()
    for i, (tid, pos, flag, words, l_seq, seq) in enumerate(recs):
        out[i] = (tid, pos, flag, len(words), l_seq, 0, len(data))
        data += struct.pack("<%dI" % len(words), *words) + seq
        data += b"\0" * (-len(data) % 4)
    return out, np.frombuffer(bytes(data), np.uint8)


def write_rows(rows, path):
    with open(path, "w") as f:
        for i, (c, p, ref, alt) in enumerate(rows):
            f.write("%s\t%d\t%d\trs%d\t%s\t%s\tACGTACGTACGTACGTACGTA\tACGTACGTACCTACGTACGTA\n" % (c, p, p + 1, i, ref, alt))


def make_counter(rows, names, tmp_path):
    import vafc
    path = str(tmp_path / "rows.txt")
    write_rows(rows, path)
    db = vafc.load_patterns(path)
    assert db.n == len(rows)
    return vafc.BamCounter(db, names)

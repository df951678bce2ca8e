"""Deterministic record classes for the two bam kernels (csrc/vafc_bam.hip),
one per branch that the seeded fuzz of tests/test_bam.py never takes:

  S  stride     more long records than the long kernel has waves: the second
                trip of its grid-stride loop, `continue` on w == 0 inside it,
                base_cur / base_rp reset between two records of one wave
  Q  bases      base indices at and past l_seq (contract item 8, bam_hit)
  Z  zero       zero-length operations of every kind, `len > 0` in the long
                kernel and `p < cur + 0` in the short one
  P  positions  rows and walks at the end of the position range: the clamps
                of end and hi to 2^31, `cur < BAM_POS_END`, 64-bit cur
  T  tids       tids past 16 bits, a row at 2^31 - 2 on t beside one at 0 on
                t + 1 (the 33-bit position field of bam_key), records on
                references without rows (`row_key[j] > tid_end`)
  W  weights    regions that touch the record at either end, nested, repeated
                and overlapping regions, the same coordinates on another tid
  B  bounds     descriptors that end exactly at, one byte and one word past
                the end of the data (bam_in_bounds)

Every class is a function returning Case(rows, ref_names, recs, regions,
note): rows [(chr, pos, ref, alt)], records as tests/bam_statement.py takes
them, regions [(tid, start, end)] for the weighted pass (None: the class has
none).  Nothing is random.

All row positions are <= 2^31 - 2.  That is no limit of the kernels:
build_regions forms pos + 1 as an int on the host when a counter is created.
write_rows gives such rows a small end column, which nothing reads.

statement(): the counts of tests/bam_statement.py's count_records, record by
record, so that prefixes and splits of a class share one computation.
model_counts(): the long kernel's walk restated over sorted keys, with named
faults; without a fault it equals the statement (tests/test_bam_edges_fixture.py),
with one it is what a kernel with that fault would count."""
import bisect
from collections import namedtuple

import numpy as np

import bam_fixture as F
from bam_statement import MATCH_OPS, QUERY_OPS, REF_OPS, SKIP, count_records, pack, rec_end

POS_END = 1 << 31            # BAM_POS_END: one past the largest position a row may have
ROW_MAX = POS_END - 2        # the largest row start a pattern file may carry (see above)
NEVER_LONG = 0xFFFFFFFF
THRESHOLDS = (0, 64, NEVER_LONG)
GIGA = (1 << 28) - 1         # the longest operation a CIGAR word holds

Case = namedtuple("Case", "rows ref_names recs regions note")


# ---------------------------------------------------------------------------
# rows and records by position
# ---------------------------------------------------------------------------

def ref_at(p: int) -> str:
    return "ACGT"[p % 4]


def alt_at(p: int) -> str:
    return "ACGT"[(p + 1 + (p // 4) % 3) % 4]        # never the ref


def base_at(p: int) -> str:
    """The base a record shows at reference position p: mostly the ref."""
    return ref_at(p) if p % 3 else alt_at(p)


def row_at(chr_: str, p: int):
    assert -POS_END <= p <= ROW_MAX
    return (chr_, p, ref_at(p), alt_at(p))


def packed(letters: str) -> bytes:
    nib = [F.NT16.index(ch) for ch in letters] + [0]
    return bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(letters), 2))


def record(tid, pos, cigar, l_seq=None, pick=base_at, other="N", flag=0):
    """A record whose match bases show pick(reference position) and whose
    inserted and clipped bases show `other`.  The packed bases always hold the
    whole query; l_seq may say less (class Q)."""
    letters, cur = [], pos
    for w in F.cigar_words(cigar):
        op, n = w & 15, w >> 4
        if op in MATCH_OPS:
            letters += [pick(cur + k) for k in range(n)]
        elif op in QUERY_OPS:
            letters += [other] * n
        if op in REF_OPS:
            cur += n
    letters = "".join(letters)
    return (tid, pos, flag, F.cigar_words(cigar), len(letters) if l_seq is None else l_seq, packed(letters))


def match_blocks(pos, cigar):
    """[(first reference position, length)] of the M / = / X operations."""
    out, cur = [], pos
    for w in F.cigar_words(cigar):
        op, n = w & 15, w >> 4
        if op in MATCH_OPS:
            out.append((cur, n))
        if op in REF_OPS:
            cur += n
    return out


def write_rows(rows, path):
    """tests/bam_statement.py's write_rows with an end column that stays small."""
    with open(path, "w") as f:
        for i, (c, p, ref, alt) in enumerate(rows):
            f.write("%s\t%d\t%d\trs%d\t%s\t%s\tACGTACGTACGTACGTACGTA\tACGTACGTACCTACGTACGTA\n"
                    % (c, p, p + 1 if abs(p) < 1 << 20 else 1, i, ref, alt))


def make_counter(case, tmp_path):
    import vafc
    path = str(tmp_path / "rows.txt")
    write_rows(case.rows, path)
    db = vafc.load_patterns(path)
    assert db.n == len(case.rows)
    return vafc.BamCounter(db, case.ref_names)


# ---------------------------------------------------------------------------
# the classes
# ---------------------------------------------------------------------------

def s_batches(n_cu: int):
    """The long kernel runs min(2 * n_cu, (n + 3) / 4) blocks of four waves: 8 *
    n_cu waves at most, and a second trip of the loop from 8 * n_cu + 1 long
    records on."""
    return (1, 2, 3, 4, 5, 8 * n_cu - 1, 8 * n_cu, 8 * n_cu + 1, 16 * n_cu + 7)


S_SEVENTH = [("S", 2), ("M", 0), ("M", 3), ("I", 1), ("M", 2)]


def class_S(n_cu: int = 256) -> Case:
    n = s_batches(n_cu)[-1]
    rows = [row_at("chr1", 2 * i) for i in range(n)]
    recs, blocked = [], set()
    for i in range(n):
        own = lambda p, i=i: base_at(p) if p == 2 * i else "N"       # counts on its own row only
        recs.append(record(0, 2 * i, S_SEVENTH if i % 7 == 0 else [("M", 1)], pick=own))
        if i % 5 == 0:      # outside every region: the rows it covers have none
            blocked |= {i, i + 1, i + 2} if i % 7 == 0 else {i}
    regions = [(0, 2 * i, 2 * i + 1) for i in range(n) if i not in blocked]
    return Case(rows, ["chr1"], recs, regions,
                "%d records on a row each; every 5th outside all regions, every 7th 2S 0M 3M 1I 2M" % n)


Q_CIGARS = ([("M", 10)], [("S", 3), ("M", 4), ("I", 2), ("M", 5)])


def q_l_seqs(cigar):
    n = F.query_len(cigar)
    return (n, n - 1, n - 2, 1, 0)


def class_Q() -> Case:
    rows, recs, regions = [], [], []
    at = 100
    for cigar in Q_CIGARS:
        for l_seq in q_l_seqs(cigar):
            # every base is the row's ref, the ones behind l_seq as well: the
            # padding nibble of the last byte (odd l_seq) and the byte behind it
            recs.append(record(0, at, cigar, l_seq=l_seq, pick=ref_at, other="N"))
            rows += [row_at("chr1", p) for p in range(at - 1, at + F.ref_len(cigar) + 1)]
            regions += [(0, at, at + 3), (0, at + 2, at + 40)]
            at += 100
    return Case(rows, ["chr1"], recs, regions, "l_seq of query_len, -1, -2, 1 and 0 under 10M and 3S 4M 2I 5M")


Z_OPS = ("M", "D", "N", "I", "S", "=", "X")


def z_long_cigar():
    """130 operations, zero-length ones in lanes 63 and 0 of the wave path's
    groups, a match block behind each pair: a zero-length block that covered
    its position would count that block's first base a second time."""
    cigar = [("M", 2) if i % 2 == 0 else ("D", 1) if i % 4 == 1 else ("I", 1) for i in range(130)]
    cigar[63], cigar[64], cigar[65] = ("M", 0), ("=", 0), ("M", 2)
    cigar[127], cigar[128], cigar[129] = ("X", 0), ("D", 0), ("M", 2)
    return cigar


def class_Z() -> Case:
    rows, recs, regions = [], [], []
    at = 100
    cigars = []
    for z in Z_OPS:
        inner = "M" if z == "S" else z       # clips stand at the ends only
        cigars += [[(z, 0), ("M", 4), ("D", 2), ("M", 4)], [("M", 4), (inner, 0), ("M", 4)],
                   [("M", 4), ("N", 2), ("M", 4), (z, 0)]]
    cigars.append([("S", 3), ("M", 0), ("I", 2), ("D", 0), ("=", 0)])        # rlen 0: end = pos + 1
    cigars.append(z_long_cigar())
    for cigar in cigars:
        # clipped and inserted bases show the ref of the record's first position
        recs.append(record(0, at, cigar, other=ref_at(at)))
        span = max(F.ref_len(cigar), 1)
        rows += [row_at("chr1", p) for p in range(at - 1, at + span + 1)]
        regions += [(0, at, at + 1), (0, at + span - 1, at + span + 5)]
        at += 100 * (1 + span // 100)
    return Case(rows, ["chr1"], recs, regions, "0M 0D 0N 0I 0S 0= 0X at the head, inside and at the tail; rlen 0; 130 ops")


def giga_cigar(reps: int, split: bool = False):
    """3M (2^28 - 1)N, `reps` times, then 3M; split: every N as two."""
    gap = [("N", 1 << 27), ("N", GIGA - (1 << 27))] if split else [("N", GIGA)]
    return ([("M", 3)] + gap) * reps + [("M", 3)]


def padded_to_70(cigar):
    """The same walk as 70 operations for the wave path: `1P`, which does
    nothing, three times behind every operation but the last and five times
    more in front of it; the last block is lane 5 of the second group."""
    assert len(cigar) == 17
    out = []
    for op in cigar[:-1]:
        out += [op] + [("P", 1)] * 3
    return out + [("P", 1)] * 5 + cigar[-1:]


P_STARTS = (100, POS_END - (1 << 28) - 5)


def class_P() -> Case:
    names = ["chrA", "chrB"]
    spots = set()
    for t in (0, 1):
        spots |= {(t, ROW_MAX), (t, ROW_MAX - 1), (t, ROW_MAX - 64), (t, 0), (t, 1)}
    spots.add((1, -1))
    recs = []
    for t in (0, 1):
        recs.append(record(t, POS_END - 10, [("M", 20)]))                # the bases past the range have no rows
        recs.append(record(t, POS_END - 1, [("M", 5)]))                  # starts behind the last row
        for pos in range(-5, 0):
            recs.append(record(t, pos, [("M", 8)]))
    # walks whose cur passes 2^31 (8 gaps) and 2^32 (17 and 23 gaps): 16 gaps
    # advance it by 2^32 + 32, so a cur kept in 32 bits comes back to pos + 32
    walks = [(0, giga_cigar(8)), (1, giga_cigar(17)), (0, giga_cigar(23, True)), (1, padded_to_70(giga_cigar(8)))]
    assert [len(c) for _t, c in walks] == [17, 35, 70, 70]
    for t, cigar in walks:
        for pos in P_STARTS:
            recs.append(record(t, pos, cigar))
            blocks = match_blocks(pos, cigar)
            assert blocks[-1][0] > POS_END and (len(blocks) < 17 or blocks[-1][0] > 1 << 32)
            for k in (0, 6, 7):
                spots |= {(t, p) for p in range(blocks[k][0], blocks[k][0] + 3) if p <= ROW_MAX}
            spots |= {(t, pos + 32 + k) for k in range(3)}               # where the 17th block is, modulo 2^32
    rows = [row_at(names[t], p) for t, p in sorted(spots)]
    regions = [(0, 0, 1000), (0, 50, 150), (0, POS_END - 70, POS_END - 1), (0, POS_END - 3, POS_END - 1),
               (1, -1, 1), (1, 100, 103), (1, POS_END - 12, POS_END - 2), (0, 6 * (1 << 28), 7 * (1 << 28))]
    return Case(rows, names, recs, regions, "rows up to 2^31 - 2, 20M from 2^31 - 10, walks past 2^31 and 2^32, pos < 0")


T_TIDS = (0, 1, 40000, 65535, 65536, 69999)
T_EMPTY = (2, 39999, 50000, 65534, 65537, 69998)      # references without rows, rows on later ones
T_NAMES = 70000


def class_T() -> Case:
    names = ["c%d" % i for i in range(T_NAMES)]
    rows, recs = [], []
    for t in T_TIDS:
        rows += [row_at(names[t], p) for p in (0, 1, 5, ROW_MAX - 1, ROW_MAX)]
        recs.append(record(t, POS_END - 10, [("M", 20)]))                # runs past 2^31
        recs.append(record(t, POS_END - 4, giga_cigar(1)))               # and far past it
        recs.append(record(t, -3, [("M", 8)]))
        recs.append(record(t, 0, [("M", 2), ("D", 3), ("M", 2)]))
    for t in T_EMPTY:
        recs.append(record(t, POS_END - 10, [("M", 20)]))
        recs.append(record(t, -3, [("M", 8)]))
        recs.append(record(t, 0, [("M", 6)]))
    recs.append(record(T_TIDS[-1], POS_END - 1, [("M", 5)]))             # no row anywhere behind it
    regions = []
    for t in (0, 65535):
        regions += [(t, POS_END - 3, POS_END - 1), (t + 1, 0, 1)]
    regions += [(40000, -5, 3), (40000, 0, 1), (69999, 0, POS_END - 1), (12345, 0, 100), (50000, 0, 100)]
    return Case(rows, names, recs, regions, "70,000 references, rows on six of them at both ends of the range")


W_POS, W_LEN = 1000, 10


def w_lists():
    """(what, regions around a record [pos, end) on tid 0, weight), pos = 0."""
    e = W_LEN
    return [("e == pos", [(0, -5, 0)], 0), ("e == pos + 1", [(0, -5, 1)], 1), ("s == end - 1", [(0, e - 1, e + 5)], 1),
            ("s == end", [(0, e, e + 5)], 0), ("inside", [(0, 3, 5)], 1), ("contains", [(0, -10, e + 10)], 1),
            ("three times", [(0, 2, 6)] * 3, 3), ("overlapping", [(0, -3, 4), (0, 2, 20)], 2),
            ("another tid", [(1, -10, e + 10), (1, 3, 5)], 0),
            ("four", [(0, 2, 6)] * 3 + [(0, e - 1, e)], 4), ("five", [(0, -3, 4), (0, 2, 20)] + [(0, 0, 1)] * 3, 5),
            ("all touching", [(0, -5, 0), (0, -5, 1), (0, e - 1, e + 5), (0, e, e + 5)], 2)]


def class_W() -> Case:
    rows, recs, regions = [], [], []
    at = W_POS
    for _what, regs, _w in w_lists():
        recs.append(record(0, at, [("M", W_LEN)], pick=ref_at))
        rows.append(row_at("chr1", at + 4))
        regions += [(t, at + s, at + e) for t, s, e in regs]
        at += 1000
    recs.append(record(0, at, [("S", 5), ("I", 3)], other=ref_at(at)))   # rlen 0 on a one-base region
    rows.append(row_at("chr1", at))
    regions.append((0, at, at + 1))
    return Case(rows, ["chr1", "chr2"], recs, regions, "one 10M record per region list, weights 0..5")


def class_B() -> Case:
    """The three good records; b_probes() adds the probe and the tail."""
    rows = [row_at("chr1", p) for p in range(100, 140)]
    recs = [record(0, 100, [("M", 6)]), record(0, 110, [("S", 1), ("M", 3), ("I", 2), ("M", 4)]),
            record(0, 120, [("M", 2), ("D", 1)] * 34 + [("M", 2)])]
    return Case(rows, ["chr1"], recs, None, "three good records, a probe and the 64 bytes of a skipped record")


B_TAIL = 64


def b_probes():
    """[(what, recs, data, accepted, records of the statement)].  The probe is
    the fourth of five descriptors, `6M` at 130; behind its bytes lie 64
    bytes that belong to a flag-0x4 record, so everything the probe could
    claim up to one word too many starts inside data."""
    case = class_B()
    probe = record(0, 130, [("M", 6)])
    tail = (0, 130, 0x4, [], 2 * B_TAIL, bytes([0x11]) * B_TAIL)
    base_recs, data = pack(case.recs + [probe, tail])
    off, n = int(base_recs[3]["off"]), data.size
    assert int(base_recs[4]["off"]) == off + 8 and n == off + 8 + B_TAIL and n % 4 == 0
    avail = n - off
    out = []

    def add(what, accepted, counted, **fields):
        recs = base_recs.copy()
        for k, v in fields.items():
            recs[3][k] = v
        out.append((what, recs, data, accepted, case.recs + counted if accepted else None))

    exact = 2 * (avail - 4)             # need = 4 + (l_seq + 1) / 2 = avail
    add("need == data_bytes - off", True, [probe[:4] + (exact,) + probe[5:]], l_seq=exact)
    add("need == data_bytes - off, odd l_seq", True, [probe[:4] + (exact - 1,) + probe[5:]], l_seq=exact - 1)
    add("off == data_bytes, empty", True, [], off=n, n_cigar=0, l_seq=0)
    add("l_seq one byte over", False, None, l_seq=exact + 1)
    add("n_cigar one word over", False, None, n_cigar=avail // 4 + 1, l_seq=0)
    add("off == data_bytes + 4, empty", False, None, off=n + 4, n_cigar=0, l_seq=0)
    add("off % 4 == 1", False, None, off=off + 1)
    add("off % 4 == 3", False, None, off=off + 3)
    return out


def b_need(rec) -> int:
    return 4 * int(rec["n_cigar"]) + ((int(rec["l_seq"]) + 1) >> 1)


CLASSES = {"S": class_S, "Q": class_Q, "Z": class_Z, "P": class_P, "T": class_T, "W": class_W}
SPLIT = "SPT"                 # also counted as two batches cut at an odd index
_cases = {}


def case_of(name: str, n_cu: int = 256) -> Case:
    key = (name, n_cu if name == "S" else 0)
    if key not in _cases:
        _cases[key] = CLASSES[name](n_cu) if name == "S" else CLASSES[name]()
    return _cases[key]


def thresholds_of(name: str):
    """S is about the long kernel's loop: threshold 0, and 64 as a control."""
    return (0, 64) if name == "S" else THRESHOLDS


def batches_of(name: str, case: Case, n_cu: int = 256):
    """The record counts of the prefixes of the class that are counted."""
    return s_batches(n_cu) if name == "S" else (len(case.recs),)


def row_tids(case: Case):
    tid_of = {nm: i for i, nm in enumerate(case.ref_names)}
    return [tid_of.get(r[0], -1) for r in case.rows]


# ---------------------------------------------------------------------------
# the statement, record by record
# ---------------------------------------------------------------------------

class Statement:
    """count_records of tests/bam_statement.py for every record of a case on
    its own: (count index, amount) lists whose sums over any batch are the
    counts of that batch.  count_records tests every row and every region
    against every record; here it is handed the rows inside [pos, end) and the
    regions that can reach the record, both found by bisection, and applies
    its own rules to them."""

    def __init__(self, case: Case):
        self.case = case
        self.row_tid = row_tids(case)
        self.by_tid = {}
        for i, (t, r) in enumerate(zip(self.row_tid, case.rows)):
            if t >= 0:
                self.by_tid.setdefault(t, []).append((r[1], i))
        for v in self.by_tid.values():
            v.sort()
        self.regs = {}
        for t, s, e in case.regions or ():
            self.regs.setdefault(t, []).append((s, e))
        self.reach = {t: max(e - s for s, e in v) for t, v in self.regs.items()}
        for v in self.regs.values():
            v.sort()
        self._parts = {}

    def _one(self, rec, weighted):
        tid, pos = rec[0], rec[1]
        end = rec_end(rec)
        at = self.by_tid.get(tid, [])
        idx = [i for _p, i in at[bisect.bisect_left(at, (pos, -1)):bisect.bisect_left(at, (end, -1))]]
        if not idx:
            return []
        regions = None
        if weighted:
            rs = self.regs.get(tid, [])
            lo = bisect.bisect_left(rs, (pos - self.reach.get(tid, 0), -POS_END))
            hi = bisect.bisect_left(rs, (end, -POS_END))
            regions = [(tid, s, e) for s, e in rs[lo:hi]]
        c = count_records([self.case.rows[i] for i in idx], [tid] * len(idx), [rec], regions)
        return [(2 * idx[k // 2] + k % 2, int(c[k])) for k in np.nonzero(c)[0]]

    def parts(self, weighted: bool):
        if weighted not in self._parts:
            self._parts[weighted] = [self._one(rec, weighted) for rec in self.case.recs]
        return self._parts[weighted]

    def counts(self, n: int, weighted: bool) -> np.ndarray:
        """The counts of the first n records."""
        out = np.zeros(2 * len(self.case.rows), np.uint64)
        for part in self.parts(weighted)[:n]:
            for k, v in part:
                out[k] += v
        return (out & 0xFFFFFFFF).astype(np.uint32)


_statements = {}


def statement(name: str, n_cu: int = 256) -> Statement:
    case = case_of(name, n_cu)
    if id(case) not in _statements:
        _statements[id(case)] = Statement(case)
    return _statements[id(case)]


# ---------------------------------------------------------------------------
# the long kernel's walk with named faults
# ---------------------------------------------------------------------------

FAULTS = ("no_l_seq_guard", "pos_32_bits", "key_shift_32", "weight_e_ge_pos", "weight_s_le_end", "zero_covers",
          "stride_dropped", "stale_rp", "stale_cur")


def _wrap32(v: int) -> int:
    return ((v + POS_END) & 0xFFFFFFFF) - POS_END


def model_counts(case: Case, n: int, weighted: bool, fault=None, n_cu: int = 256) -> np.ndarray:
    """What bam_long_kernel counts for the first n records when every record
    with a CIGAR is long (threshold 0), in the kernel's own terms: sorted
    (tid, pos) keys, lower bounds, the clamps at 2^31.  fault None: the shipped
    kernel.  The list of long records is taken in batch order."""
    assert fault is None or fault in FAULTS
    shift = 32 if fault == "key_shift_32" else 33
    wrap = _wrap32 if fault == "pos_32_bits" else (lambda v: v)

    def key(t, x):
        return (t << shift) + (x + POS_END)

    def key_pos(k):
        return (k & ((1 << 33) - 1)) - POS_END

    order = sorted((key(t, r[1]), i) for i, (t, r) in enumerate(zip(row_tids(case), case.rows)) if t >= 0)
    row_key = [k for k, _i in order]
    regions = case.regions if weighted else None
    reg_s = sorted(key(t, s) for t, s, _e in regions or ())
    reg_e = sorted(key(t, e) for t, _s, e in regions or ())
    counts = np.zeros(2 * len(case.rows), np.uint64)
    waves = 8 * n_cu
    listed = [r for r in case.recs[:n] if not (r[2] & SKIP) and r[0] >= 0 and r[3]]
    if fault == "stride_dropped":
        listed = listed[:waves]
    left = {}                 # wave -> (cur, rp) its last record ended with
    for e, (tid, pos, _flag, words, l_seq, seq) in enumerate(listed):
        w = 1
        if regions:
            rlen = sum(c >> 4 for c in words if (c & 15) in REF_OPS)
            end = min(wrap(pos + (rlen or 1)), POS_END)
            starts_below = bisect.bisect_left(reg_s, key(tid, end) + (fault == "weight_s_le_end"))
            ends_upto = bisect.bisect_left(reg_e, key(tid, pos) + (fault != "weight_e_ge_pos"))
            w = (starts_below - ends_upto) & 0xFFFFFFFF
            if w == 0:
                continue
        cur, rp = pos, 0
        if e % waves in left:
            if fault == "stale_rp":
                rp = left[e % waves][1]
            if fault == "stale_cur":
                cur = left[e % waves][0]
        for c in words:
            op, ln = c & 15, c >> 4
            if op in MATCH_OPS and (ln > 0 or fault == "zero_covers") and cur < POS_END:
                hi = min(wrap(cur + (max(ln, 1) if fault == "zero_covers" else ln)), POS_END)
                for j in range(bisect.bisect_left(row_key, key(tid, cur)), len(row_key)):
                    if row_key[j] >= key(tid, hi):
                        break
                    q = rp + key_pos(row_key[j]) - cur
                    if q >= l_seq and (fault != "no_l_seq_guard" or (q >> 1) >= len(seq)):
                        continue
                    base = F.NT16[seq[q >> 1] & 15 if q & 1 else seq[q >> 1] >> 4]
                    i = order[j][1]
                    if base == case.rows[i][2]:
                        counts[2 * i] += w
                    elif base == case.rows[i][3]:
                        counts[2 * i + 1] += w
            if op in REF_OPS:
                cur = wrap(cur + ln)
            if op in QUERY_OPS:
                rp += ln
        left[e % waves] = (cur, rp)
    return (counts & 0xFFFFFFFF).astype(np.uint32)


# ---------------------------------------------------------------------------
# a second, plainer restatement: the CIGAR expanded base by base
# ---------------------------------------------------------------------------

EXPAND_LIMIT = 1 << 20        # reference bases; the gigabase walks of P are left to model_counts


def expanded_counts(case: Case, n: int, weighted: bool):
    """(counts, records left out).  Every record becomes a dict {reference
    position: query index, or None inside D / N}; a row counts if its position
    is in the dict with an index below l_seq."""
    row_at_ = {}
    for i, (t, r) in enumerate(zip(row_tids(case), case.rows)):
        if t >= 0:
            row_at_.setdefault((t, r[1]), []).append(i)
    counts = np.zeros(2 * len(case.rows), np.uint64)
    left_out = []
    for ri, (tid, pos, flag, words, l_seq, seq) in enumerate(case.recs[:n]):
        if flag & SKIP or tid < 0:
            continue
        if sum(c >> 4 for c in words) > EXPAND_LIMIT:
            left_out.append(ri)
            continue
        where, cur, rp = {}, pos, 0
        for c in words:
            op, ln = c & 15, c >> 4
            for _ in range(ln):
                if op in MATCH_OPS:
                    where[cur] = rp
                elif op in (2, 3):
                    where[cur] = None
                cur += op in REF_OPS
                rp += op in QUERY_OPS
        end = max(cur, pos + 1)
        w = 1
        if weighted:
            w = len([1 for t, s, e in case.regions if t == tid and max(s, pos) < min(e, end)])
        for p, q in where.items():
            if q is None or q >= l_seq:
                continue
            base = F.NT16[seq[q >> 1] & 15 if q & 1 else seq[q >> 1] >> 4]
            for i in row_at_.get((tid, p), ()):
                if base == case.rows[i][2]:
                    counts[2 * i] += w
                elif base == case.rows[i][3]:
                    counts[2 * i + 1] += w
    return (counts & 0xFFFFFFFF).astype(np.uint32), left_out


def first_difference(case: Case, got, want):
    """None, or the text that names the first row whose counts differ."""
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    i = int(bad[0]) // 2
    return "%d of %d counts differ, first row %d %r: counted (ref %d, alt %d), statement (ref %d, alt %d)" % (
        bad.size, got.size, i, tuple(case.rows[i]), int(got[2 * i]), int(got[2 * i + 1]), int(want[2 * i]),
        int(want[2 * i + 1]))

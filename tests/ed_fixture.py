"""Deterministic inputs for the approximate-search kernel (csrc/vafc_ed.hip):
the statement of the hit count, a model of how wave 0 lays reads out in its
4,096-byte chunks, query sets that reach every kernel shape, and one class of
reads per layout event, each with the counts the statement gives.  Pure
Python and numpy, no GPU; tests/test_ed_fixture.py checks the fixture on the
CPU, tests/test_ed_edges.py runs it against the kernel.

Queries.  Three lengths of the 32-bit width and two of each other width
(WIDTH_LENGTHS).  A width has N_BASE = 13 distinct base queries that cycle
through its lengths; query i of a width is base[i % 13].  13 is coprime to 64,
so no power-of-two shift of a lane or a wave maps a query onto an equal one.
The statement scans the 13 distinct queries only: the expected count of query
i is that of base i % 13.  The second base of each width is a slice of the
128-bit width's 127-byte base around its middle, and the first a slice of its
65-byte base, so one planted copy straddles a chunk edge for all widths.

Alphabets.  `small` is ACGT (5 classes: every shape keeps its masks in LDS).
`wide256` uses all 256 byte values (class = byte), `wide255` all but one
(n_class = 256, class 0 = the other byte); the first three 128-bit bases of
a wide alphabet hold every symbol, and a wide handle always has at least
these three, so every shape reads its masks from HBM.  alphabet("t<k>") has k
symbols, all of them in the queries of each single width (the mask placement
threshold).

Read classes (one EdClass per ordered list of reads; a list runs as one read
range):

  P  prefixes of one 8,300-byte text with copies planted around bytes 4,096
     and 8,192, cut at 4,092..4,101 and 8,188..8,197 bytes, each followed by a
     30-byte marker read: takes of 4,092 and 4,096 (rounded up); the CHUNK + 4 branch; a
     tail of exactly one chunk; tails of 1..5 bytes that share a chunk with
     the marker
  X  four reads whose takes add up to exactly 4,096 (the fit test's <=), and
     the same with the last read 4 bytes longer (it moves to the next chunk)
  G  63, 64, 65, 128, 129 empty reads and 64 reads of 1..4 bytes, then a
     marker (the 64-read cut: a 65th read that would fit by bytes); empty
     reads behind a tail of exactly 4,096 bytes (beg == end == 4096).  An
     empty read counts 1 for every query, so the counts say how many reads
     were walked
  T  a read of 4,096 + k bytes (k = 1, 4, 5, 100) with a copy across byte
     4,096, then short reads with copies: the tail shares a chunk with them,
     its state must survive; one list fills the tail's chunk to exactly 4,096
  L  short reads, then a read longer than a chunk (the piece path starts with
     done == 0 after a chunk of segments); short reads, then a read of at most
     4,096 bytes that does not fit what is left
  S  X + Q, 63 empty reads, X + Q[:-1] of a length that is no multiple of 4:
     the second read opens the next chunk at the same LDS offset, and the
     class of Q[-1] still lies behind it, where only the nj clamp keeps the
     walk from completing the match; per length residue 1, 2, 3 and a query
     of each width
  R  the T and L lists in one: cut into read ranges at several max_ranges
"""
import collections
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# the statement (include/vafc.h, vc_ed_create)
# ---------------------------------------------------------------------------

def pad_w(m):
    return 64 * ((m + 63) // 64) - m


def dp_hits(P: bytes, T: bytes, e: int) -> int:
    """The hit count of (T, P), straight from the table."""
    m, n = len(P), len(T)
    if n == 0:
        return 1
    kp = min(m if e < 0 else e, m)
    col = list(range(m + 1))
    cand = []
    for ch in T:
        nc = [0] * (m + 1)
        for i in range(1, m + 1):
            nc[i] = min(col[i] + 1, nc[i - 1] + 1, col[i - 1] + (P[i - 1] != ch))
        col = nc
        cand.append(col[m])
    if kp == m and n < pad_w(m):
        cand.append(m)
    b = min(cand)
    return cand.count(b) if b <= kp else 0


def scan_read(Q: np.ndarray, T: bytes):
    """Q: uint8 [nq, m], queries of one length.  (best, cnt): the minimum of the
    last row over the columns of T and how often it occurs, per query."""
    nq, m = Q.shape
    idx = np.arange(m + 1, dtype=np.int32)
    col = np.tile(idx, (nq, 1))
    best = np.full(nq, m + 1, np.int32)
    cnt = np.zeros(nq, np.int64)
    neq = {}
    full = np.zeros((nq, m + 1), np.int32)
    for ch in T:
        d = neq.get(ch)
        if d is None:
            d = neq[ch] = (Q != ch).astype(np.int32)
        np.minimum(col[:, 1:] + 1, col[:, :-1] + d, out=full[:, 1:])
        # nc[i] = min(full[i], nc[i - 1] + 1): a running minimum of full[i] - i
        col = np.minimum.accumulate(full - idx, axis=1) + idx
        s = col[:, m]
        lt = s < best
        cnt = np.where(lt, 1, cnt + (s == best))
        best = np.minimum(best, s)
    return best, cnt


def scan_read_at(Q: np.ndarray, T: bytes, marks):
    """scan_read with checkpoints: one pass over T; {n: (best, cnt)} of the
    prefix T[:n] for every n in marks (1..len(T))."""
    marks = set(int(n) for n in marks)
    assert marks and min(marks) >= 1 and max(marks) <= len(T)
    nq, m = Q.shape
    idx = np.arange(m + 1, dtype=np.int32)
    col = np.tile(idx, (nq, 1))
    best = np.full(nq, m + 1, np.int32)
    cnt = np.zeros(nq, np.int64)
    neq = {}
    full = np.zeros((nq, m + 1), np.int32)
    out = {}
    for j, ch in enumerate(T[:max(marks)]):
        d = neq.get(ch)
        if d is None:
            d = neq[ch] = (Q != ch).astype(np.int32)
        np.minimum(col[:, 1:] + 1, col[:, :-1] + d, out=full[:, 1:])
        col = np.minimum.accumulate(full - idx, axis=1) + idx
        s = col[:, m]
        lt = s < best
        cnt = np.where(lt, 1, cnt + (s == best))
        best = np.minimum(best, s)
        if j + 1 in marks:
            out[j + 1] = (best.copy(), cnt.copy())
    return out


def rule(best, cnt, n, m, e):
    if n == 0:
        return np.ones(len(best), np.int64)
    kp = min(m if e < 0 else e, m)
    c = cnt + ((best == m) if (kp == m and n < pad_w(m)) else 0)
    return np.where(best <= kp, c, 0)


class Statement:
    """Per read and query length the (best, cnt) vectors, so that one scan
    serves every -e."""

    def __init__(self, queries, reads):
        self.queries = [bytes(q) for q in queries]
        self.by_len = {}
        for i, q in enumerate(self.queries):
            self.by_len.setdefault(len(q), []).append(i)
        self.reads = [bytes(r) for r in reads]
        self.scans = []
        mats = {m: np.array([list(self.queries[i]) for i in ids], np.uint8).reshape(len(ids), m)
                for m, ids in self.by_len.items()}
        for T in self.reads:
            self.scans.append({m: scan_read(mats[m], T) for m in mats} if T else None)

    def per_read(self, e: int) -> np.ndarray:
        """int64 [reads, queries]: the hit count of every (read, query)."""
        out = np.zeros((len(self.reads), len(self.queries)), np.int64)
        for r, (T, sc) in enumerate(zip(self.reads, self.scans)):
            for m, ids in self.by_len.items():
                out[r, ids] = 1 if sc is None else rule(sc[m][0], sc[m][1], len(T), m, e)
        return out

    def counts(self, e: int, times=None) -> np.ndarray:
        """The counters after all reads (read r taken times[r] times)."""
        pr = self.per_read(e)
        out = pr.sum(axis=0) if times is None else (pr * np.asarray(times, np.int64)[:, None]).sum(axis=0)
        return (out & 0xFFFFFFFF).astype(np.uint32)


# ---------------------------------------------------------------------------
# the kernel's constants and the host's shape rule (csrc/vafc_ed.h, ed_fill)
# ---------------------------------------------------------------------------

def _define(name):
    with open(os.path.join(ROOT, "kmer-cnt_amd", "csrc", "vafc_ed.h")) as f:
        return int(re.search(r"#define %s (\d+)\b" % name, f.read()).group(1))


CHUNK = _define("VC_ED_CHUNK")
SEGS = _define("VC_ED_SEGS")
MAX_WAVES = _define("VC_ED_MAX_WAVES")
LDS_MASKS = _define("VC_ED_LDS_MASKS")

W32, W64, W128 = 0, 1, 2
WIDTHS = (W32, W64, W128)
WIDTH_NAMES = ("W32", "W64", "W128")
WIDTH_WORDS = (1, 1, 2)
WIDTH_WORDBYTES = (4, 8, 8)
WIDTH_LENGTHS = ((21, 32, 1), (33, 64), (65, 127))     # the order in which the bases cycle through them
N_BASE = 13
E_VALUES = (0, 2, -1)
N_QUERIES = (1, 64, 65, 129, 192, 193, 256, 257)      # per width: 1, 1, 2, 3, 3, 4, 4 and 5 groups


def width_of(m):
    return W32 if m <= 32 else (W64 if m <= 64 else W128)


def n_class_of(queries):
    """ed_fill's classes: one per byte value in a query and class 0 for the
    others; class = byte when all 256 occur."""
    used = len(set(b"".join(queries)))
    return 256 if used == 256 else used + 1


def expected_shape(n_class, width, n_queries):
    """(n_groups, waves, lds_masks) as ed_fill decides them."""
    if n_queries == 0:
        return 0, 1, True
    groups = (n_queries + 63) // 64
    waves = min(groups, MAX_WAVES)
    return groups, waves, n_class * WIDTH_WORDS[width] * waves * 64 * WIDTH_WORDBYTES[width] <= LDS_MASKS


# ---------------------------------------------------------------------------
# wave 0's loop, restated
# ---------------------------------------------------------------------------

Seg = collections.namedtuple("Seg", "read beg end starts ends")
Piece = collections.namedtuple("Piece", "read done starts")     # CHUNK bytes of `read` from byte `done` on
Chunk = collections.namedtuple("Chunk", "segs piece")           # one of the two is None


def layout(lens):
    """The chunks one block makes of a read range with these lengths: per chunk
    either its segments (read, beg, end, starts, ends: bytes [beg, end) of
    s_codes, whether the read starts / ends here) or one piece."""
    chunks, r, done, n = [], 0, 0, len(lens)
    while r < n:
        segs, end = [], 0
        for lane in range(min(SEGS, n - r)):
            rem = lens[r + lane] - (done if lane == 0 else 0)
            take = CHUNK + 4 if rem > CHUNK else (rem + 3) & ~3
            end += take                                   # the inclusive scan
            if end > CHUNK:                               # fit: the fitting reads are a prefix
                break
            segs.append(Seg(r + lane, end - take, end - take + rem, lane > 0 or done == 0, True))
        if not segs:
            chunks.append(Chunk(None, Piece(r, done, done == 0)))
            done += CHUNK
        else:
            chunks.append(Chunk(segs, None))
            r += len(segs)
            done = 0
    return chunks


def range_cuts(n_reads, max_ranges):
    """The read ranges of a launch with vc_ed_set_max_ranges(max_ranges > 0) on
    a device with more blocks to fill than that (vafc_ed.cpp, launch)."""
    gy = max(1, min(max_ranges, n_reads))
    per = (n_reads + gy - 1) // gy
    return [(a, min(a + per, n_reads)) for a in range(0, n_reads, per)]


def tail_done(chunks, read):
    """Bytes of `read` that pieces consumed before its last segment."""
    return CHUNK * sum(1 for c in chunks if c.piece and c.piece.read == read)


def stale_behind(reads, other):
    """Per read of the range, the bytes that lie in s_codes between its end and
    the next dword boundary when it is walked: what earlier chunks left there
    (`other`, a byte of class 0, where nothing was written yet).  A piece ends
    on a dword: nothing behind it."""
    lds = bytearray(other * CHUNK)
    out = [b""] * len(reads)
    for c in layout([len(r) for r in reads]):
        if c.piece:
            p = c.piece
            lds[:] = reads[p.read][p.done:p.done + CHUNK]
            continue
        for s in c.segs:
            src = len(reads[s.read]) - (s.end - s.beg)     # a segment always ends its read
            lds[s.beg:s.end] = reads[s.read][src:]
        for s in c.segs:
            out[s.read] = bytes(lds[s.end:(s.end + 3) & ~3])
    return out


# ---------------------------------------------------------------------------
# alphabets and queries
# ---------------------------------------------------------------------------

class Alphabet:
    """symbols: the bytes of the queries; other: one byte of class 0 (for
    wide256, where class = byte, the byte 0 that the kernel's cleared LDS
    holds); bases[width]: the 13 base queries."""

    def __init__(self, name, symbols, other, seed):
        self.name, self.symbols, self.other, self.seed = name, bytes(symbols), bytes(other), seed
        sym = np.frombuffer(self.symbols, np.uint8)
        rng = np.random.default_rng(seed)

        def rnd(n):
            return bytearray(sym[rng.integers(0, sym.size, n)].tobytes())

        # the 128-bit bases first: the leading three hold every symbol (as far as 257 bytes go)
        big = [rnd(WIDTH_LENGTHS[W128][i % 2]) for i in range(N_BASE)]
        perm = sym[rng.permutation(sym.size)].tobytes()[:65 + 127 + 65]
        for i, at in ((0, 0), (1, 65), (2, 192)):
            part = perm[at:at + len(big[i])]
            big[i][:len(part)] = part
        k65, k127 = bytes(big[0]), bytes(big[1])
        self.bases = {W128: [bytes(q) for q in big]}
        for w, nested in ((W32, (k65[22:43], k127[47:79])), (W64, (k65[16:49], k127[31:95]))):
            lens = WIDTH_LENGTHS[w]
            qs = [bytearray(nested[i]) if i < 2 else rnd(lens[i % len(lens)]) for i in range(N_BASE)]
            ones = [q for q in qs if len(q) == 1]
            for j, q in enumerate(ones):                  # the one-byte queries: distinct symbols
                q[0] = self.symbols[j]
            # as many of the symbols as fit: a missing one replaces, from the
            # back, a byte that occurs elsewhere in the width's queries
            have = collections.Counter(b"".join(bytes(q) for q in qs))
            missing = [s for s in self.symbols if not have[s]]
            slots = [(i, j) for i in range(3, N_BASE) if len(qs[i]) > 1 for j in range(len(qs[i]))]
            for i, j in slots[::-1]:
                if missing and have[qs[i][j]] > 1:
                    have[qs[i][j]] -= 1
                    qs[i][j] = missing.pop()
            self.bases[w] = [bytes(q) for q in qs]
        for w in WIDTHS:
            assert len(set(self.bases[w])) == N_BASE, (name, w)
            assert [len(q) for q in self.bases[w]] == [WIDTH_LENGTHS[w][i % len(WIDTH_LENGTHS[w])]
                                                       for i in range(N_BASE)]
        self.wide = len(self.symbols) >= 200

    def text(self, rng, n):
        """n random symbols, one in 64 replaced by the other byte."""
        sym = np.frombuffer(self.symbols, np.uint8)
        t = bytearray(sym[rng.integers(0, sym.size, n)].tobytes())
        if self.other[0] not in self.symbols:
            for at in np.nonzero(rng.integers(0, 64, n) == 0)[0]:
                t[at] = self.other[0]
        return t

    def edited(self, q):
        """q with its middle byte replaced by another symbol."""
        q = bytearray(q)
        at = len(q) // 2
        q[at] = next(s for s in self.symbols if s != q[at])
        return bytes(q)

    def queries(self, width, n):
        return [self.bases[width][i % N_BASE] for i in range(n)]


@functools.lru_cache(maxsize=None)
def alphabet(name):
    if name == "small":
        return Alphabet(name, b"ACGT", b"N", 4101)
    if name == "wide256":
        return Alphabet(name, bytes(range(256)), b"\x00", 4102)
    if name == "wide255":
        return Alphabet(name, bytes(b for b in range(256) if b != 0x4E), b"\x4e", 4103)
    m = re.fullmatch(r"t(\d+)", name)
    assert m, name
    return Alphabet(name, bytes(range(0x30, 0x30 + int(m.group(1)))), b"\xff", 4200 + int(m.group(1)))


ALPHABETS = ("small", "wide256", "wide255")


def handle_queries(alpha, n_per_width):
    """The queries of one handle that holds the three widths at once, widths
    interleaved (query 3 i + w is query i of width w, as far as the width
    goes), and per width the positions of its queries in the handle.
    n_per_width: one number for all widths or one per width.  A wide handle
    has at least the three 128-bit queries that hold every symbol."""
    ns = [n_per_width] * 3 if isinstance(n_per_width, int) else list(n_per_width)
    if alpha.wide:
        ns[W128] = max(ns[W128], 3)
    per = [alpha.queries(w, ns[w]) for w in WIDTHS]
    queries, where = [], [[], [], []]
    for i in range(max(ns)):
        for w in WIDTHS:
            if i < ns[w]:
                where[w].append(len(queries))
                queries.append(per[w][i])
    return queries, [np.array(x, np.int64) for x in where]


# ---------------------------------------------------------------------------
# read classes
# ---------------------------------------------------------------------------

EdClass = collections.namedtuple("EdClass", "name tag reads")

P_CUTS = tuple(range(4092, 4102)) + tuple(range(8188, 8198))
P_LEN = 8300
T_TAILS = (1, 4, 5, 100)
G_EMPTY = (63, 64, 65, 128, 129)
S_QUERIES = ((W32, 0), (W64, 1), (W128, 0))      # (width, base): 21, 64 and 65 bytes


def _plant(t, at, q):
    assert 0 <= at and at + len(q) <= len(t)
    t[at:at + len(q)] = q


class Reads:
    """The texts and read lists of one alphabet."""

    def __init__(self, alpha):
        self.alpha = a = alpha
        rng = np.random.default_rng(alpha.seed + 1)

        def text(n):
            return alpha.text(rng, n)

        b32, b64, b128 = a.bases[W32], a.bases[W64], a.bases[W128]
        k65, k127 = b128[0], b128[1]
        # P: the 127-byte base (and the slices of it that are bases of the other
        # widths) around 4,096 and 8,192, at other offsets in every alphabet
        t = text(P_LEN)
        if a.name == "small":
            _plant(t, CHUNK - 63, k127)                       # the middle byte on the edge
            _plant(t, 2 * CHUNK - 65, k65)                    # offset -m: ends with the chunk
            _plant(t, 2 * CHUNK + 1, a.edited(k65))           # offset +1
        elif a.name == "wide256":
            _plant(t, CHUNK - 1, k65)                         # offset -1: one byte before the edge
            _plant(t, 2 * CHUNK - 126, k127)                  # offset -(m - 1): one byte behind it
        else:
            _plant(t, CHUNK, k127)                            # offset 0
            _plant(t, 2 * CHUNK - 32, a.edited(k65))          # the middle, one edit
        _plant(t, 300, k65)                                   # the first chunk holds a copy of every
        _plant(t, 1000, k127)                                 # planted base: losing it changes a count
        _plant(t, 700, b32[3])
        _plant(t, 5000, b64[2])
        self.p_text = bytes(t)
        self.marker = bytes(text(4)) + b32[0] + bytes(text(5))
        assert len(self.marker) == 30
        self.shorts = [bytes(text(7)) + b32[0] + bytes(text(9)),
                       bytes(text(5)) + a.edited(b64[0]) + bytes(text(6)),
                       bytes(text(3)) + b128[0] + bytes(text(2)),
                       bytes(text(11)) + a.edited(b32[1])]
        # X: three reads of 1,024 bytes and the prefixes of a fourth text
        xs = [text(1024) for _ in range(3)] + [text(1028)]
        for i, (t, q) in enumerate(zip(xs, (b32[4], a.edited(b64[3]), b128[2], b32[6]))):
            _plant(t, 100 + 200 * i, q)
        _plant(xs[3], 1021 - 21, b32[0])                     # ends with the shortest cut
        self.x_reads, self.x_text = [bytes(t) for t in xs[:3]], bytes(xs[3])
        # T: prefixes of one text, a copy across byte 4,096
        t = text(CHUNK + 100)
        _plant(t, CHUNK - 40, k127)
        _plant(t, 1500, a.edited(b64[1]))
        self.t_text = bytes(t)
        self.tiny = [bytes(text(1 + i % 4)) for i in range(64)]

    def classes(self, names="PXGTLSR"):
        a, mk = self.alpha, self.marker
        rng = np.random.default_rng(a.seed + 2)
        out = []
        if "P" in names:
            out += [EdClass("P", {"cut": n}, [self.p_text[:n], mk]) for n in P_CUTS]
        if "X" in names:
            for n in (1021, 1022, 1023, 1024):
                out.append(EdClass("X", {"last": n, "sum": "4096"}, self.x_reads + [self.x_text[:n], mk]))
                out.append(EdClass("X", {"last": n + 4, "sum": "4096 + 4"}, self.x_reads + [self.x_text[:n + 4], mk]))
        if "G" in names:
            out += [EdClass("G", {"empty": n}, [b""] * n + [mk]) for n in G_EMPTY]
            out.append(EdClass("G", {"tiny": 64}, self.tiny + [mk]))
            out.append(EdClass("G", {"behind_full_tail": 3}, [self.p_text[:2 * CHUNK]] + [b""] * 3 + [mk]))
        t_lists = [[self.t_text[:CHUNK + k]] + self.shorts for k in T_TAILS]
        # a tail of 100 bytes, 3 x 1,024 and 924 bytes: the takes add up to 4,096
        t_fill = [self.t_text[:CHUNK + 100]] + self.x_reads + [self.x_text[:924], mk]
        l_lists = [self.shorts + [self.p_text[:5000], mk], self.shorts + [self.p_text[:4050], mk]]
        if "T" in names:
            out += [EdClass("T", {"tail": k}, r) for k, r in zip(T_TAILS, t_lists)]
            out.append(EdClass("T", {"tail": 100, "fills": "to 4096"}, t_fill))
        if "L" in names:
            out.append(EdClass("L", {"long": 5000}, l_lists[0]))
            out.append(EdClass("L", {"unfit": 4050}, l_lists[1]))
        if "S" in names:
            for w, i in S_QUERIES:
                q = a.bases[w][i]
                for res in (1, 2, 3):
                    pre = (res + 1 - len(q)) % 4 + 4      # len(pre + q[:-1]) % 4 == res
                    x = bytes(s for s in a.text(rng, 16 * pre) if s != q[-1] and s != q[0])[:pre]
                    assert len(x) == pre and (len(x) + len(q) - 1) % 4 == res
                    out.append(EdClass("S", {"width": WIDTH_NAMES[w], "m": len(q), "residue": res},
                                       [x + q] + [b""] * 63 + [x + q[:-1]]))
        if "R" in names:
            out.append(EdClass("R", {"lists": "T + L"}, [r for lst in t_lists + [t_fill] + l_lists for r in lst]))
        return out


# ---------------------------------------------------------------------------
# the statement over a fixture: every distinct read scanned once, a read that
# is a prefix of another from the longer one's checkpoints
# ---------------------------------------------------------------------------

class Scores:
    def __init__(self, alpha):
        self.alpha = alpha
        self.mats = {}
        for w in WIDTHS:
            for m in WIDTH_LENGTHS[w]:
                ids = [i for i, q in enumerate(alpha.bases[w]) if len(q) == m]
                self.mats[m] = (ids, np.array([list(alpha.bases[w][i]) for i in ids], np.uint8).reshape(len(ids), m))
        self.cache = {}       # (m, text) -> (best, cnt)

    def prepare(self, reads, widths=WIDTHS):
        """Scan the distinct reads for the lengths of `widths`."""
        for m in [m for w in widths for m in WIDTH_LENGTHS[w]]:
            todo = sorted({bytes(r) for r in reads if r and (m, bytes(r)) not in self.cache}, key=len, reverse=True)
            left = set(todo)
            for t in todo:
                if t not in left:
                    continue
                fam = [u for u in left if t.startswith(u)]
                left.difference_update(fam)
                for n, sc in scan_read_at(self.mats[m][1], t, [len(u) for u in fam]).items():
                    self.cache[(m, t[:n])] = sc

    def counts(self, text, width, e, n=None):
        """int64 [13]: the hit counts of the width's base queries on `text`,
        the rule applied with read length n (the text's own by default)."""
        text = bytes(text)
        n = len(text) if n is None else n
        out = np.zeros(N_BASE, np.int64)
        for m in WIDTH_LENGTHS[width]:
            ids, mat = self.mats[m]
            if not text:
                assert n == 0
                out[ids] = 1
                continue
            if (m, text) not in self.cache:
                self.cache[(m, text)] = scan_read(mat, text)
            best, cnt = self.cache[(m, text)]
            out[ids] = rule(best, cnt, n, m, e)
        return out

    def expected(self, reads, width, e):
        """uint32 [13]: the counters of the width's base queries after `reads`."""
        tot = np.zeros(N_BASE, np.int64)
        for r in reads:
            tot += self.counts(r, width, e)
        return (tot & 0xFFFFFFFF).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _texts_and_scores(name):
    return Reads(alphabet(name)), Scores(alphabet(name))


@functools.lru_cache(maxsize=None)
def fixture(name, names=None):
    """(alphabet, classes, scores) of one alphabet; the texts and the scans are
    shared by every selection of classes.  names: the classes' letters; by
    default all for `small`, P, G and S else."""
    reads, scores = _texts_and_scores(name)
    return alphabet(name), reads.classes(names or ("PXGTLSR" if name == "small" else "PGS")), scores


def prepared(name, names=None, widths=WIDTHS):
    """fixture() with the statement built for the lengths of `widths`."""
    alpha, classes, scores = fixture(name, names)
    scores.prepare([r for c in classes for r in c.reads], widths)
    return alpha, classes, scores


# ---------------------------------------------------------------------------
# three faulty kernels, as plain Python over the layout model
# ---------------------------------------------------------------------------

def faulty_counts(fault, scores, reads, width, e):
    """What a kernel with one of these faults would count on a read range:
    1  the state is reset at the start of a tail (the first segment of a chunk
       that continues a read): only T[done:] is scored, with n = len(T)
    2  the state is reset at every piece: only the bytes from the last piece
       on are scored
    3  the nj clamp is ignored: the up to three stale bytes behind a read are
       walked as well"""
    lens = [len(r) for r in reads]
    chunks = layout(lens)
    stale = stale_behind(reads, scores.alpha.other) if fault == 3 else None
    tot = np.zeros(N_BASE, np.int64)
    for i, r in enumerate(reads):
        done = tail_done(chunks, i)
        if fault == 1 and done:
            tot += scores.counts(r[done:], width, e, n=len(r))
        elif fault == 2 and done > CHUNK:
            tot += scores.counts(r[done - CHUNK:], width, e, n=len(r))
        elif fault == 3 and r:
            assert done == 0
            tot += scores.counts(r + stale[i], width, e, n=len(r))
        else:
            tot += scores.counts(r, width, e)
    return (tot & 0xFFFFFFFF).astype(np.uint32)

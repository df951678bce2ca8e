"""Deterministic inputs for the k-mer scan kernels (csrc/vafc_scan.h), one class
of reads per path the scan can take, and what the oracle counts on them.

A wave of the counting kernel is 64 consecutive reads, and every branch of
scan_span_quad is chosen by a wave-uniform condition (the wave's longest read,
its longest tail, whether any lane has an invalid base ...).  So the classes
below are laid out in whole waves: every class starts on a 64-read boundary
and is padded to a multiple of 64 with reads of length 0, and the whole set
goes to the counter in one call.  Read starts take all four byte alignments
(class_index % 4 filler bytes 'N' before each class).

Every read is cut from one genome G of 3,000 random ACGT bases:

  A      uniform waves: for every L in 1..208, 64 substrings of length L
         (every nit = ceil(L / 16) in 1..13, every len & 15, the chunk-1 skip
         taken and not, the half last chunk taken and not)
  Bdiag  L in (40, 96, 150) x bad byte in ('N', 0x00, 0x80, 'S'): read p is one
         fixed substring with that byte at position p, consecutive lanes
  Bwave  the same reads, each one 64 times: a whole wave with the defect at
         the same position (the wave-uniform side of every ballot shortcut)
  Tdiag  L = 48 + t for every tail length t in 1..15 x byte in ('S', 0x00,
         0x01, 0x02, 'u'): read p has the byte at tail position p; one wave of
         equal tail lengths, so the tail ladder (dec_tail_chunk) stops at the
         dword that t asks for.  The head decode and seq_nt4_table disagree on
         all of 'S' (C / invalid), 0x00 (invalid / A), 0x01 (A / C), 0x02
         (invalid / G)
  Tmix   the same reads for all t in consecutive lanes (mixed tail lengths)
  C      G tiled to 16384 (the longest whole read), 16385, 16399, 16400, 16401,
         16640, 16641 and 20000 bases (the segmented long-read kernel), each
         once clean; 16385 and 16641 also once per defect position in
         b - k .. b + 1 around the segment borders b = 256, 16384 and the last
         multiple of 256 below the length, with 'N' and 0x00

Keys are every distinct canonical k-mer of all the reads (oracle.read_kmers);
key i has value i, its expected count is its multiplicity, and the expected
tally is the number of valid windows.  The "large" variant appends 70,000
absent keys, which takes the table past VC_L2F_MIN_KEYS (65,536).
"""
import collections
import functools

import numpy as np

WAVE = 64
SEED = 20261
GENOME_LEN = 3000
A_LENGTHS = tuple(range(1, 209))
B_LENGTHS = (40, 96, 150)
B_BYTES = (0x4E, 0x00, 0x80, 0x53)
T_BASE = 48
T_BYTES = (0x53, 0x00, 0x01, 0x02, 0x75)
C_LENGTHS = (16384, 16385, 16399, 16400, 16401, 16640, 16641, 20000)
C_DEFECT_LENGTHS = (16385, 16641)
C_BYTES = (0x4E, 0x00)
LONG_SEG = 256           # VC_LONG_SEG
LONG_READ = 16384        # VC_LONG_READ
N_ABSENT = 70_000
L2F_MIN_KEYS = 65_536    # VC_L2F_MIN_KEYS

ScanClass = collections.namedtuple("ScanClass", "name tag reads")


def genome():
    rng = np.random.default_rng(SEED)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, GENOME_LEN)]


def _with_byte(base, p, byte):
    r = base.copy()
    r[p] = byte
    return r.tobytes()


def classes_a(lengths=A_LENGTHS):
    G = genome()
    rng = np.random.default_rng(SEED + 1)
    out = []
    for L in lengths:
        starts = rng.integers(0, GENOME_LEN - L + 1, WAVE)
        out.append(ScanClass("A", {"L": L}, [G[s:s + L].tobytes() for s in starts]))
    return out


def _b_base(L):
    G = genome()
    s = 101 * L % (GENOME_LEN - L)
    return G[s:s + L]


def classes_bdiag(lengths=B_LENGTHS, bad=B_BYTES):
    return [ScanClass("Bdiag", {"L": L, "byte": b, "pos": "lane"}, [_with_byte(_b_base(L), p, b) for p in range(L)])
            for L in lengths for b in bad]


def classes_bwave(lengths=B_LENGTHS, bad=B_BYTES):
    return [ScanClass("Bwave", {"L": L, "byte": b, "pos": p}, [_with_byte(_b_base(L), p, b)] * WAVE)
            for L in lengths for b in bad for p in range(L)]


def classes_t(bad=T_BYTES):
    out = []
    for b in bad:
        mix = []
        for t in range(1, 16):
            L = T_BASE + t
            reads = [_with_byte(_b_base(L), T_BASE + p, b) for p in range(t)]
            out.append(ScanClass("Tdiag", {"L": L, "byte": b, "pos": "48 + lane"}, reads))
            mix += reads
        out.append(ScanClass("Tmix", {"L": "49..63", "byte": b, "pos": "every tail position"}, mix))
    return out


def c_borders(L):
    return sorted({LONG_SEG, LONG_READ, (L - 1) // LONG_SEG * LONG_SEG})


def classes_c(k):
    G = genome()
    tiled = np.tile(G, max(C_LENGTHS) // GENOME_LEN + 1)
    out = [ScanClass("C", {"L": L, "byte": None, "pos": None}, [tiled[:L].tobytes()]) for L in C_LENGTHS]
    for L in C_DEFECT_LENGTHS:
        for b in c_borders(L):
            pos = [p for p in range(b - k, b + 2) if 0 <= p < L]
            for byte in C_BYTES:
                out.append(ScanClass("C", {"L": L, "byte": byte, "pos": "%d + lane" % pos[0], "border": b},
                                     [_with_byte(tiled[:L], p, byte) for p in pos]))
    return out


def all_classes(k, long_reads=True):
    out = classes_a() + classes_bdiag() + classes_bwave() + classes_t()
    return out + classes_c(k) if long_reads else out


def layout(classes):
    """(seq, offs, lens, spans): the classes' reads in one buffer with explicit
    offsets; spans[i] = (first read, end read) of class i, both multiples of
    64.  Class i is preceded by i % 4 filler bytes and padded with reads of
    length 0 (which start where the class's bytes end)."""
    parts, offs, lens, spans, pos = [], [], [], [], 0
    for ci, c in enumerate(classes):
        fill = ci % 4
        parts.append(b"N" * fill)
        pos += fill
        first = len(offs)
        for r in c.reads:
            offs.append(pos)
            lens.append(len(r))
            parts.append(r)
            pos += len(r)
        pad = -len(c.reads) % WAVE
        offs += [pos] * pad
        lens += [0] * pad
        spans.append((first, len(offs)))
    seq = np.frombuffer(b"".join(parts), np.uint8).copy()
    return seq, np.array(offs, np.uint64), np.array(lens, np.uint32), spans


def revcomp(x, k):
    """Reverse complement of right-aligned k-mers (uint64 array)."""
    x = np.asarray(x, np.uint64)
    r = np.zeros_like(x)
    for _ in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x = x >> np.uint64(2)
    return r


def head_kmers(k, reads):
    """(keys, mult, tally): the distinct canonical k-mers of the reads as the
    oracle extracts them (oracle.read_kmers: vaf-counter's decode, the last
    len % 16 bytes of a read through seq_nt4_table), their multiplicities and
    the number of valid windows.  Equal reads are extracted once."""
    import oracle as O
    uniq = collections.Counter(reads)
    ks, ws = [np.zeros(0, np.uint64)], [np.zeros(0, np.int64)]
    for r, m in uniq.items():
        a = O.read_kmers(k, r)
        ks.append(a)
        ws.append(np.full(a.size, m, np.int64))
    return _tabulate(np.concatenate(ks), np.concatenate(ws))


def _tabulate(allk, w):
    keys, inv = np.unique(allk, return_inverse=True)
    mult = np.zeros(keys.size, np.int64)
    np.add.at(mult, inv.reshape(-1), w)
    return keys, mult, int(w.sum())


def absent_keys(k, keys, n=N_ABSENT):
    """n distinct canonical k-mers that are not in `keys`."""
    rng = np.random.default_rng(SEED + 100 + k)
    x = rng.integers(0, 1 << (2 * k), 2 * n, dtype=np.uint64)
    x = np.setdiff1d(np.unique(np.minimum(x, revcomp(x, k))), keys)
    assert x.size >= n
    return x[rng.permutation(x.size)[:n]]


ScanSet = collections.namedtuple("ScanSet", "k classes seq offs lens spans keys vals n_pat want tally n_present")


def _scan_set(k, classes):
    seq, offs, lens, spans = layout(classes)
    keys, mult, tally = head_kmers(k, [r for c in classes for r in c.reads])
    vals = np.arange(keys.size, dtype=np.uint32)
    n_pat = (keys.size + 1) // 2
    want = np.zeros(2 * n_pat, np.uint32)
    want[:keys.size] = mult
    assert int(mult.max(initial=0)) < 1 << 32
    return ScanSet(k, classes, seq, offs, lens, spans, keys, vals, n_pat, want, tally, keys.size)


@functools.lru_cache(maxsize=2)
def _whole_set(k, long_reads):
    return _scan_set(k, all_classes(k, long_reads))


def scan_set(k, large=False, long_reads=True):
    """The whole fixture for one k (cached: the kinds of one k share it); large:
    with N_ABSENT absent keys behind the present ones."""
    s = _whole_set(k, long_reads)
    if not large:
        return s
    keys = np.concatenate([s.keys, absent_keys(k, s.keys)])
    n_pat = (keys.size + 1) // 2
    want = np.zeros(2 * n_pat, np.uint32)
    want[:s.n_present] = s.want[:s.n_present]
    return s._replace(keys=keys, vals=np.arange(keys.size, dtype=np.uint32), n_pat=n_pat, want=want)


@functools.lru_cache(maxsize=2)
def scan_set_a(k):
    """Class A alone, longest reads last: the buffer ends with the last read's
    last byte."""
    s = _scan_set(k, classes_a())
    assert int(s.offs[-1]) + int(s.lens[-1]) == s.seq.size and int(s.lens[-1]) == max(A_LENGTHS)
    return s


def class_slice(s, i):
    """Class i of a ScanSet on its own: (seq, offs, lens) with the same byte
    alignment of every read (the buffer is cut at a multiple of 4)."""
    a, b = s.spans[i]
    base = int(s.offs[a]) & ~3
    end = int(s.offs[b - 1]) + int(s.lens[b - 1])
    return s.seq[base:max(end, base + 1)], s.offs[a:b] - np.uint64(base), s.lens[a:b]


# ---------------------------------------------------------------------------
# seq_nt4 mode (snp-pattern-gen's count_candidate_kmers): every byte through
# seq_nt4_table
# ---------------------------------------------------------------------------

def nt4_table():
    """seq_nt4_table: ACGT / acgt -> 0..3, U / u -> 3, bytes 0..3 -> themselves,
    everything else 4."""
    t = np.full(256, 4, np.uint8)
    for i, ch in enumerate(b"ACGT"):
        t[ch] = t[ch + 32] = i
        t[i] = i
    t[ord("U")] = t[ord("u")] = 3
    return t


def nt4_kmers(k, reads):
    """(keys, mult, tally) as head_kmers, every byte decoded with seq_nt4_table:
    a rolling k-mer that restarts at an invalid base, restated on arrays.  The
    distinct reads are joined with an invalid byte between them; window i is
    valid iff none of its k codes is 4."""
    uniq = collections.Counter(reads)
    rs = [r for r in uniq if len(r) >= k]
    if not rs:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64), 0
    codes = nt4_table()[np.frombuffer(b"\xff".join(rs) + b"\xff", np.uint8)]
    wpos = np.repeat(np.array([uniq[r] for r in rs], np.int64), [len(r) + 1 for r in rs])
    n = codes.size - k + 1
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    valid = (bad[k:] - bad[:-k]) == 0
    c = (codes & 3).astype(np.uint64)
    f = np.zeros(n, np.uint64)
    r = np.zeros(n, np.uint64)
    for j in range(k):
        cj = c[j:j + n]
        f = (f << np.uint64(2)) | cj
        r |= (np.uint64(3) - cj) << np.uint64(2 * j)
    return _tabulate(np.minimum(f, r)[valid], wpos[:n][valid])


def nt4_classes():
    """The classes that go through seq_nt4 mode: short equal reads per wave."""
    return (classes_a(tuple(range(1, 121))) + classes_bdiag((40,)) + classes_bwave((40,)) + classes_t())


def padded_reads(classes):
    """The classes' reads in order, each class padded to whole waves with
    empty reads (for interfaces that take a list of sequences)."""
    out = []
    for c in classes:
        out += list(c.reads) + [b""] * (-len(c.reads) % WAVE)
    return out

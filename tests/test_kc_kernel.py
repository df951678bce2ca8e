"""vafc_kc.hip key by key: the counting, histogram and Bloom-replay kernels
against a plain statement of the operation, at their edges.

The statement (Python integers, dicts and sets, written from the contract in
vafc_kc.hip / vafc_kc.h / include/vafc.h):
  kmer_stream()   every canonical k-mer of the reads in stream order as
                  (read index, end position, hash64 on 2k bits); a byte other
                  than 0..3, A/C/G/T/U or a/c/g/t/u restarts the k-mer;
  statement()     {hash: count}, the k-mers seen, {hash: first (read, pos)};
  slice_of()      a key's partition slice ((h & 1023) * n_parts) >> 10;
  yak_pass1()     yak-count's pass 1, literally: one blocked filter of
                  2^(bf_shift - pre) bits per sub-table h & (2^pre - 1), the
                  n_hash bits of a k-mer visited and set in turn, the k-mer
                  inserted iff all were set when visited (a set of bit ids);
  yak_expected()  pass 2 over the kept keys.

CPU tests pin the statement to oracle/kc_oracle.c (kco_hist_reads) and to the
yak-count-oracle CLI on the very inputs the GPU tests use, and assert that
those inputs reach the edges they are built for.  GPU tests drive
vafc.KmerHistogram with small tables and compare whole runs, every partition
slice and the kept set of the Bloom replay with the statement."""
import contextlib
import functools

import numpy as np
import pytest

from test_kc import oracle_reads
from test_yak import YAK_ORACLE, run_yak

KC_LONG, KC_SEG = 4096, 1024      # vafc_kc.h: reads longer than KC_LONG are cut into KC_SEG-base segments
L5 = KC_LONG + KC_SEG + 1         # five segments, the last of one base

# --- the statement ------------------------------------------------------------

CODE = [4] * 256
for _b in range(4):
    CODE[_b] = _b
for _ch, _c in zip(b"ACGTU", (0, 1, 2, 3, 3)):
    CODE[_ch] = CODE[_ch | 0x20] = _c     # upper and lower case


def hash64(key, mask):
    key = (~key + (key << 21)) & mask
    key ^= key >> 24
    key = (key + (key << 3) + (key << 8)) & mask
    key ^= key >> 14
    key = (key + (key << 2) + (key << 4)) & mask
    key ^= key >> 28
    key = (key + (key << 31)) & mask
    return key


def kmer_stream(k, reads):
    """(read index, end position, hash64(min(forward, reverse complement)))
    of every window of k valid bases, reads in order, positions in order."""
    mask = (1 << 2 * k) - 1
    top = 2 * (k - 1)
    memo = {}
    for r, s in enumerate(reads):
        fw = rc = run = 0
        for j, byte in enumerate(s):
            c = CODE[byte]
            if c == 4:
                run = 0
                continue
            fw = (fw << 2 | c) & mask
            rc = rc >> 2 | (3 - c) << top
            run += 1
            if run >= k:
                y = fw if fw < rc else rc
                h = memo.get(y)
                if h is None:
                    h = memo[y] = hash64(y, mask)
                yield r, j, h


def statement(k, reads):
    counts, first, n = {}, {}, 0
    for r, j, h in kmer_stream(k, reads):
        n += 1
        if h in counts:
            counts[h] += 1
        else:
            counts[h] = 1
            first[h] = (r, j)
    return counts, n, first


def slice_of(h, n_parts):
    return ((h & 1023) * n_parts) >> 10


def hist_of(counts, n_bins=256, min_count=1):
    """(hist[min(c, n_bins - 1)] over the counts >= min_count, how many)"""
    hist = np.zeros(n_bins, np.uint64)
    n = 0
    for c in counts:
        if c >= min_count:
            hist[min(c, n_bins - 1)] += 1
            n += 1
    return hist, n


def yak_filter_on(pre, bf_shift, n_hash):
    return n_hash > 0 and bf_shift > pre and 9 <= bf_shift - pre <= 55


def yak_pass1(hashes, pre, bf_shift, n_hash):
    """The keys pass 1 of yak-count -b puts into the table, hashes in stream order."""
    if not yak_filter_on(pre, bf_shift, n_hash):
        return set(hashes)
    ns = bf_shift - pre               # log2 bits per sub-table filter
    nb = ns - 9                       # log2 512-bit blocks per filter
    bits, kept = set(), set()
    for h in hashes:
        sub, x = h & ((1 << pre) - 1), h >> pre
        block = x & ((1 << nb) - 1)
        h1, h2 = (x >> nb) & 511, (x >> ns) & 511
        if h2 % 32 == 0:
            h2 = (h2 + 1) & 511
        base = (sub << nb | block) << 9
        were_set, z = 0, h1
        for _ in range(n_hash):
            if base | z in bits:
                were_set += 1
            else:
                bits.add(base | z)
            z = (z + h2) & 511
        if were_set == n_hash:
            kept.add(h)
    return kept


def yak_expected(k, row, reads1, reads2):
    """(hist of min(c2, 1023) over the kept keys, bin 0 included; kept keys)"""
    _, pre, bf_shift, n_hash = row
    kept = yak_pass1([h for _, _, h in kmer_stream(k, reads1)], pre, bf_shift, n_hash)
    c2 = dict.fromkeys(kept, 0)
    for _, _, h in kmer_stream(k, reads2):
        if h in c2:
            c2[h] += 1
    return hist_of(c2.values(), 1024, 0)[0], kept


# --- inputs -------------------------------------------------------------------

ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGTacgtNn", b"TGCAtgcaNn")
INVALID = [ord("N"), ord("n"), 4, 255, ord("-"), ord("R"), ord(" "), ord("@")]


def revcomp(s):
    return s.translate(_COMP)[::-1]


def bases(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def pack(reads):
    """(seq, offs, lens) of a list of byte strings (one pad byte, so seq is never empty)"""
    lens = np.array([len(r) for r in reads], np.uint32)
    offs = np.zeros(len(reads), np.uint64)
    if len(reads):
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    seq = np.frombuffer(b"".join(reads) + b"N", np.uint8)
    return seq, offs, lens


@functools.lru_cache(maxsize=None)
def byte_set(k):
    """256 reads: a valid flank, byte value b, a valid flank (both flanks >= 31 bases)"""
    rng = np.random.default_rng(1000 + k)
    return [bases(rng, 33 + b % 5) + bytes([b]) + bases(rng, 31 + b % 3) for b in range(256)]


BORDER_OFFSETS = lambda k: [-k, -k + 1, -1, 0, 1, k - 2, k - 1]   # noqa: E731


@functools.lru_cache(maxsize=None)
def border_set(k):
    """(reads, planted): reads of the edge lengths drawn from a periodic genome,
    then reads of L5 bases with single invalid bases around every segment
    border and runs of invalid bases across them.  planted[i] lists read i's
    (position, border, offset) triples."""
    rng = np.random.default_rng(2000 + k)
    period = 1500
    tile = bases(rng, period) * 6
    lengths = [0, 1, k - 1, k, k + 1, KC_LONG - 1, KC_LONG, KC_LONG + 1, KC_LONG + KC_SEG, L5,
               KC_LONG + KC_SEG + max(k // 2, 1)]          # the last: a final segment shorter than k (k > 1)
    reads, planted = [], {}
    for i, n in enumerate(lengths):
        st = (i * 131) % period
        reads.append(tile[st:st + n])
    borders = range(KC_SEG, L5, KC_SEG)                     # 1024 .. 5120
    for i, d in enumerate(BORDER_OFFSETS(k)):
        st = (977 + i * 263) % period
        r = bytearray(tile[st:st + L5])
        where = []
        for s0 in borders:
            p = s0 + d
            if 0 <= p < L5:
                r[p] = INVALID[(i + s0 // KC_SEG) % len(INVALID)]
                where.append((p, s0, d))
        planted[len(reads)] = where
        reads.append(bytes(r))
    for width in (2, k):                                    # runs [s0 - width, s0 + width) over each border
        r = bytearray(tile[419:419 + L5])
        for s0 in borders:
            for p in range(s0 - width, min(s0 + width, L5)):
                r[p] = ord("N")
        reads.append(bytes(r))
    return reads, planted


@functools.lru_cache(maxsize=None)
def mult_set(lo, hi, k=21, seed=3):
    """(reads, {hash: m}): key i as m_i = lo..hi own k-base reads on a random strand, shuffled"""
    rng = np.random.default_rng(seed)
    keys, claim = [], {}
    while len(keys) < hi - lo + 1:
        s = bases(rng, k)
        h = next(kmer_stream(k, [s]))[2]
        if h not in claim:
            claim[h] = lo + len(keys)
            keys.append(s)
    reads = [s if rng.random() < 0.5 else revcomp(s) for s in keys for _ in range(claim[next(kmer_stream(k, [s]))[2]])]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order], claim


@functools.lru_cache(maxsize=None)
def distinct_keys(n, k=21, seed=4):
    """n one-k-mer reads with n distinct canonical k-mers"""
    rng = np.random.default_rng(seed)
    seen, reads = set(), []
    while len(reads) < n:
        s = bases(rng, k)
        h = next(kmer_stream(k, [s]))[2]
        if h not in seen:
            seen.add(h)
            reads.append(s)
    return reads


@functools.lru_cache(maxsize=None)
def st_of(name, *args):
    fn = {"byte": byte_set, "border": lambda k: border_set(k)[0]}[name]
    return statement(args[0], fn(*args))


# yak: (k, pre, bf_shift, n_hash)
YAK_ROWS = [(21, 10, 19, 4), (21, 10, 20, 1), (21, 10, 19, 32), (21, 10, 19, 40), (21, 12, 21, 2),
            (31, 11, 20, 4), (5, 10, 19, 4), (21, 10, 18, 4), (21, 10, 20, 0)]
ROW_IDS = ["k%d_p%d_b%d_H%d" % r for r in YAK_ROWS]
# reads of file 1 by k: enough for 20 false positives at k = 31 (longer k-mers, fewer per read), few
# enough at k = 5 (512 canonical 5-mers) that some k-mers occur once
N_READS1 = {21: 600, 31: 1200, 5: 8}
YAK_SLOTS = {21: 1 << 16, 31: 1 << 17, 5: 1024}        # the smallest tables that hold file 1 under the load rule


@functools.lru_cache(maxsize=None)
def yak_genome():
    return bases(np.random.default_rng(11), 200_000)


def _sample(rng, genome, n, length=120, p_n=0.01):
    out = []
    for st in rng.integers(0, len(genome) - length + 1, n):
        r = bytearray(genome[st:st + length])
        for p in np.flatnonzero(rng.random(length) < p_n):
            r[p] = ord("N")
        out.append(bytes(r) if rng.random() < 0.5 else revcomp(bytes(r)))
    return out


@functools.lru_cache(maxsize=None)
def yak_file1(k=21):
    return _sample(np.random.default_rng(12), yak_genome(), N_READS1[k])


@functools.lru_cache(maxsize=None)
def yak_file2(kind="short", k=21):
    """File 2: two thirds of file 1's reads twice (either strand) and 300 fresh reads"""
    rng = np.random.default_rng(13)
    f1 = yak_file1(k)
    pick = [f1[i] for i in rng.choice(len(f1), len(f1) * 2 // 3, replace=False)]
    reads = pick + [revcomp(r) for r in pick] + _sample(rng, yak_genome(), 300)
    reads = [reads[i] for i in rng.permutation(len(reads))]
    if kind == "short":
        return reads
    if kind == "long":
        return as_long(reads, 9)
    if kind == "absent":       # mostly another genome: keys file 1 never had
        return _sample(rng, bases(rng, 50_000), 300) + reads[:200]
    assert kind == "empty"
    return []


def as_long(reads, n_long, seed=14):
    """The same bases as n_long reads, all longer than KC_LONG: the reads in
    order, an N between two, cut at read boundaries."""
    rng = np.random.default_rng(seed)
    total = sum(len(r) + 1 for r in reads)
    per = total / n_long
    assert per > KC_LONG + 300
    out, cur, target = [], [], per + rng.integers(-200, 200)
    for r in reads:
        cur.append(r)
        if sum(len(x) + 1 for x in cur) >= target and len(out) < n_long - 1:
            out.append(b"N".join(cur))
            cur, target = [], per + rng.integers(-200, 200)
    if cur:
        out.append(b"N".join(cur))
    assert all(len(r) > KC_LONG for r in out)
    return out


@functools.lru_cache(maxsize=None)
def yak_shape(shape, k=21):
    """File 1 in shape a (short reads), b (long reads), c (both, interleaved)"""
    f1 = yak_file1(k)
    if shape == "a":
        return f1
    assert k == 21
    if shape == "b":
        return as_long(f1, 10)
    assert shape == "c"
    longs = as_long(f1[300:], 5, seed=15)
    out = []
    for i, r in enumerate(f1[:300]):
        out.append(r)
        if i % 60 == 30:
            out.append(longs[i // 60])
    return out


@functools.lru_cache(maxsize=None)
def yak_want(row, shape="a", kind="short"):
    return yak_expected(row[0], row, yak_shape(shape, row[0]), yak_file2(kind, row[0]))


@functools.lru_cache(maxsize=None)
def yak_st1(k, shape="a"):
    return statement(k, yak_shape(shape, k))


# --- CPU: the statement against the oracles, and what the inputs reach ---------

def _against_kc_oracle(k, reads):
    counts, n, _ = statement(k, reads)
    hist, d, km = oracle_reads(k, *pack(reads))
    want, wd = hist_of(counts.values())
    assert km == n and d == wd == len(counts)
    assert np.array_equal(hist, want)


@pytest.mark.parametrize("k", [1, 4, 21, 31])
def test_statement_matches_kc_oracle_on_every_byte(k):
    _against_kc_oracle(k, byte_set(k))


@pytest.mark.parametrize("k", [1, 2, 16, 31])
def test_statement_matches_kc_oracle_on_borders(k):
    _against_kc_oracle(k, border_set(k)[0])


def test_statement_matches_kc_oracle_on_multiplicities():
    _against_kc_oracle(21, mult_set(1, 300)[0])
    _against_kc_oracle(21, yak_shape("c"))


def test_every_byte_set_decodes_as_stated():
    valid = set(range(4)) | set(b"ACGTUacgtu")
    for k in (1, 4, 21, 31):
        for b, r in enumerate(byte_set(k)):
            n = sum(1 for _ in kmer_stream(k, [r]))
            whole = len(r) - k + 1
            assert n == (whole if b in valid else whole - k), (k, b)
    assert any(s == revcomp(s) for s in (r[i:i + 4] for r in byte_set(4) for i in range(30)))   # palindromes at even k


@pytest.mark.parametrize("k", [1, 2, 16, 31])
def test_border_set_reaches_its_edges(k):
    reads, planted = border_set(k)
    lens = [len(r) for r in reads]
    for n in (0, 1, k - 1, k, k + 1, KC_LONG - 1, KC_LONG, KC_LONG + 1, KC_LONG + KC_SEG, L5):
        assert n in lens
    assert L5 % KC_SEG == 1
    if k > 1:
        assert any(n > KC_LONG and 0 < n % KC_SEG < k for n in lens)
    offsets = set()
    for i, where in planted.items():
        assert len(reads[i]) == L5 > KC_LONG and where
        for p, s0, d in where:
            assert s0 % KC_SEG == 0 and 0 < s0 < L5 and p - s0 == d and CODE[reads[i][p]] == 4
            offsets.add(d)
        # a single invalid base: its neighbours are valid
        assert all(CODE[reads[i][q]] < 4 for p, _, _ in where for q in (p - 1, p + 1) if 0 <= q < L5)
    assert offsets == set(BORDER_OFFSETS(k))
    for r in reads[-2:]:                                   # the runs cover both sides of every border
        assert all(CODE[r[s0 - 1]] == 4 and CODE[r[min(s0, L5 - 1)]] == 4 for s0 in range(KC_SEG, L5, KC_SEG))
    counts, _, _ = st_of("border", k)
    if k >= 16:   # keys recur across segments and reads, below the histogram's clamp
        assert 2 < min(counts.values()) and max(counts.values()) < 255
        assert len(set(counts.values())) >= 4


def test_multiplicity_sets_have_the_counts_they_claim():
    for lo, hi in ((1, 300), (1021, 1026)):
        reads, claim = mult_set(lo, hi)
        counts, n, _ = statement(21, reads)
        assert counts == claim and n == len(reads) == sum(range(lo, hi + 1))
        assert sorted(claim.values()) == list(range(lo, hi + 1))
        assert any(r != s for r, s in zip(reads, map(revcomp, reads))) and len(set(reads)) > len(claim)
    assert len(statement(21, distinct_keys(851))[0]) == 851


def _yak_oracle_text(hist, tmp_path, k, pre, bf_shift, n_hash, f1, f2):
    got = run_yak(YAK_ORACLE, ["-k", str(k), "-p", str(pre), "-b", str(bf_shift), "-H", str(n_hash), f1, f2],
                  cwd=tmp_path)
    assert got[0] == 0, got[2]
    shrunk = [0, 0] + [int(c) for c in hist[2:]]            # yak drops keys outside [2, 1023] before printing
    assert got[1].decode() == "".join("%d\t%d\n" % (i, shrunk[i]) for i in range(1, 1024))
    assert got[3] == "[M::main] %d distinct k-mers after shrinking" % sum(shrunk)


def _write(path, reads, fastq):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) if fastq else b">r%d\n%s\n" % (i, r))


@pytest.fixture(scope="module")
def yak_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("yakk")
    for shape in "abc":
        _write(d / ("1%s.fq" % shape), yak_shape(shape), True)
        _write(d / ("1%s.fa" % shape), yak_shape(shape), False)
    for kind in ("short", "long", "absent", "empty"):
        _write(d / ("2%s.fq" % kind), yak_file2(kind), True)
        _write(d / ("2%s.fa" % kind), yak_file2(kind), False)
    for k in (5, 31):
        for fastq, ext in ((True, "fq"), (False, "fa")):
            _write(d / ("1a_k%d.%s" % (k, ext)), yak_shape("a", k), fastq)
            _write(d / ("2short_k%d.%s" % (k, ext)), yak_file2("short", k), fastq)
    return d


@pytest.mark.parametrize("row", YAK_ROWS, ids=ROW_IDS)
def test_statement_matches_yak_oracle(row, yak_files):
    hist, _ = yak_want(row)
    tag = "" if row[0] == 21 else "_k%d" % row[0]
    _yak_oracle_text(hist, yak_files, *row, "1a%s.fq" % tag, "2short%s.fq" % tag)
    _yak_oracle_text(hist, yak_files, *row, "1a%s.fa" % tag, "2short%s.fa" % tag)
    assert hist[2:].sum() > 100                            # file 2 sees kept keys twice and more


@pytest.mark.parametrize("row", YAK_ROWS[:3], ids=ROW_IDS[:3])
@pytest.mark.parametrize("shape,kind", [("b", "short"), ("c", "short"), ("a", "long"), ("a", "absent"),
                                        ("a", "empty")])
def test_statement_matches_yak_oracle_on_shapes(row, shape, kind, yak_files):
    hist, _ = yak_want(row, shape, kind)
    _yak_oracle_text(hist, yak_files, *row, "1%s.fa" % shape, "2%s.fq" % kind)


@pytest.mark.parametrize("row", YAK_ROWS, ids=ROW_IDS)
def test_yak_sets_exercise_the_filter(row):
    k, pre, bf_shift, n_hash = row
    for shape in "abc" if row in YAK_ROWS[:3] else "a":
        counts, _, _ = yak_st1(k, shape)
        _, kept = yak_want(row, shape)
        singles = {h for h, c in counts.items() if c == 1}
        assert {h for h, c in counts.items() if c > 1} <= kept <= set(counts)
        if not yak_filter_on(pre, bf_shift, n_hash):
            assert kept == set(counts)
        elif k == 5:
            # hash64 on 10 bits: h >> pre is 0, every key is alone in its sub-table's filter
            assert len(singles) >= 20 and not singles & kept and len(kept) >= 20
        else:
            assert len(singles & kept) >= 20 and len(singles - kept) >= 20
            back = yak_pass1([h for _, _, h in kmer_stream(k, yak_shape(shape, k)[::-1])], pre, bf_shift, n_hash)
            assert back != kept                             # the order of the stream decides: stamps matter
    if n_hash > 32:   # some key visits one of its own bits twice
        assert any(((h >> bf_shift) & 511) % 32 == 16 for h in counts)   # h2 = 16 (mod 32): period 32


def test_yak_shapes_are_what_they_claim():
    assert all(len(r) == 120 for r in yak_shape("a"))
    assert len(yak_shape("b")) == 10 and all(len(r) > KC_LONG + KC_SEG for r in yak_shape("b"))
    lens = [len(r) for r in yak_shape("c")]
    assert sum(n > KC_LONG for n in lens) == 5 and sum(n == 120 for n in lens) == 300
    assert lens[0] == 120 and lens[-1] == 120               # long reads lie between short ones
    gone = set(statement(21, yak_file2("absent"))[0]) - set(yak_st1(21)[0])
    assert len(gone) > 10_000
    assert all(len(r) > KC_LONG for r in yak_file2("long"))
    for k in (5, 21, 31):                                   # file 1 fits its table, and no smaller one
        assert YAK_SLOTS[k] // 2 // 100 * 85 < len(yak_st1(k)[0]) <= YAK_SLOTS[k] // 100 * 85


# --- GPU: counting and histogram kernels ---------------------------------------

@contextlib.contextmanager
def counter(k, slots):
    import vafc
    h = vafc.KmerHistogram(k, slots)
    try:
        yield h
    finally:
        h.close()


def count(h, reads):
    h.count_block(*pack(reads))
    return h.finish()[1]


def check_whole(h, st, n_bins=256, min_count=1):
    counts, n, _ = st
    hist, d, km = h.histogram(n_bins, min_count)
    want, wd = hist_of(counts.values(), n_bins, min_count)
    assert (km, d) == (n, wd)
    assert np.array_equal(hist, want)


def check_exact_counts(h, st):
    """Few keys, counts beyond every clamp: keys with count >= c, for every c around the stated counts."""
    counts = st[0]
    for c in sorted({x + e for x in counts.values() for e in (0, 1)}):
        assert h.histogram(2, c)[1] == sum(1 for x in counts.values() if x >= c), c


def check_slices(h, reads, st, n_parts):
    counts, n, _ = st
    packed = pack(reads)
    by = [[] for _ in range(n_parts)]
    for key, c in counts.items():
        by[slice_of(key, n_parts)].append(c)
    for part in range(n_parts):
        h.set_partition(n_parts, part)
        h.count_block(*packed)
        assert h.finish()[1] == n
        hist, d, _ = h.histogram()
        want, wd = hist_of(by[part])
        assert d == wd and np.array_equal(hist, want), (n_parts, part)
    h.set_partition(1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 4, 21, 31])
def test_every_byte_value(k):
    reads, st = byte_set(k), st_of("byte", k)
    with counter(k, 1 << 14) as h:
        assert count(h, reads) == st[1]
        check_whole(h, st)
        if k <= 4:
            check_whole(h, st, 1024)
        for n_parts in (3, 7, 64):
            check_slices(h, reads, st, n_parts)
        if k == 31:                                         # the smallest set: every slice of 1024
            check_slices(h, reads, st, 1024)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 16, 31])
def test_lengths_and_segment_borders(k):
    reads, st = border_set(k)[0], st_of("border", k)
    with counter(k, 1 << 13) as h:
        assert count(h, reads) == st[1]
        check_whole(h, st)
        if k <= 2:
            check_exact_counts(h, st)
        for n_parts in (3, 7, 64):
            check_slices(h, reads, st, n_parts)
        # every read on its own: no error of one read hidden by another
        for r in reads[5:]:
            h.reset()
            count(h, [r])
            check_whole(h, statement(k, [r]))


@pytest.mark.gpu
def test_multiplicity_coded_keys():
    import vafc
    reads, claim = mult_set(1, 300)
    st = statement(21, reads)
    with counter(21, 1024) as h:
        assert count(h, reads) == st[1]
        hist, d, _ = h.histogram()
        assert d == 300 and hist[0] == 0 and np.all(hist[1:255] == 1) and hist[255] == 46
        for n_bins, min_count in [(256, 0), (256, 2), (256, 255), (256, 256), (1024, 1), (2, 1), (2, 2), (2, 0),
                                  (3, 1)]:
            check_whole(h, st, n_bins, min_count)
        assert h.histogram(2)[0].tolist() == [0, 300] and h.histogram(256, 256)[1] == 45
        for n_bins in (1, 1025, 0):
            with pytest.raises(vafc.VafcError) as e:
                h.histogram(n_bins)
            assert e.value.code == vafc.VC_EINVAL
        reads, claim = mult_set(1021, 1026)
        h.reset()
        count(h, reads)
        hist, d, _ = h.histogram(1024)
        assert d == 6 and hist[1021] == 1 and hist[1022] == 1 and hist[1023] == 4 and hist.sum() == 6
        check_whole(h, statement(21, reads), 256)
        check_exact_counts(h, (claim,))


@pytest.mark.gpu
def test_contention_on_one_read():
    read = bases(np.random.default_rng(5), 40)
    st = statement(21, [read] * 1000)
    assert sorted(st[0].values()) == [1000] * 20
    with counter(21, 1024) as h:
        assert count(h, [read] * 1000) == 20_000
        hist, d, _ = h.histogram(1024)
        assert hist[1000] == 20 and hist.sum() == 20 and d == 20


@pytest.mark.gpu
def test_accumulation_over_calls():
    k = 16
    edge = border_set(k)[0]
    shorts = [edge[2][:k - 1], b"", b"ACGTN" * 2, edge[3][:k - 1]]
    parts = [edge[:9], [], shorts, edge[9:14], edge[14:]]
    whole = [r for p in parts for r in p]
    st = statement(k, whole)
    assert statement(k, shorts)[1] == 0 and st[1] == st_of("border", k)[1]
    with counter(k, 1 << 14) as h:
        results = []
        for cuts in ([whole], [whole[:7], whole[7:]], parts):
            h.reset()
            for p in cuts:
                h.count_block(*pack(p))
            assert h.finish()[1] == st[1]
            check_whole(h, st)
            results.append(h.histogram(1024)[0])
        assert all(np.array_equal(results[0], r) for r in results[1:])
        h.reset()
        other = byte_set(k)
        count(h, other)
        check_whole(h, statement(k, other))


@pytest.mark.gpu
def test_device_path_unaligned_and_overlapping():
    import torch
    rng = np.random.default_rng(6)
    buf = bytearray(bases(rng, 3001))
    for p in rng.integers(0, len(buf), 25):
        buf[p] = ord("N")
    offs = np.array([(i * 7) % 2900 for i in range(700)], np.uint64)
    lens = np.array([1 + (i * 13) % 100 for i in range(700)], np.uint32)
    reads = [bytes(buf[int(o):int(o) + int(n)]) for o, n in zip(offs, lens)]
    st = statement(21, reads)
    dev = torch.device("cuda:0")
    d_buf = torch.from_numpy(np.frombuffer(b"\0" + bytes(buf), np.uint8).copy()).to(dev)
    d_seq = d_buf[1:]
    assert d_seq.data_ptr() % 4 == 1
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
    with counter(21, 1 << 13) as h:
        h.count_device(d_seq.data_ptr(), len(buf), d_offs.data_ptr(), d_lens.data_ptr(), len(reads),
                       torch.cuda.current_stream().cuda_stream)
        assert h.finish()[1] == st[1]
        check_whole(h, st)


@pytest.mark.gpu
def test_load_rule_at_its_edge():
    import vafc
    with counter(21, 1024) as h:
        assert h.slots == 1024
        reads = distinct_keys(851)
        count(h, reads[:850])                               # slots / 100 * 85
        check_whole(h, statement(21, reads[:850]))
        h.reset()
        count(h, reads)
        with pytest.raises(vafc.VafcError) as e:
            h.histogram()
        assert e.value.code == vafc.VC_EFULL
        h.reset()
        count(h, reads[1:])
        check_whole(h, statement(21, reads[1:]))


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["block", "device"])
def test_long_list_overflow_is_reported(path):
    """Three reads of KC_LONG + 1 bases on the same KC_LONG + 1 bytes: the
    long-read list, sized seq_bytes / (KC_LONG + 1) + 1 = 2, cannot hold them.
    The main counter's rule (test_gpu_parity.py::test_long_read_list_overflow_is_reported):
    finish() fails with VC_EINVAL until reset(), never VC_EFULL (which the
    CLIs answer by counting again in more partitions)."""
    import torch
    import vafc
    read = bases(np.random.default_rng(7), KC_LONG + 1)
    seq = np.frombuffer(read, np.uint8)
    offs, lens = np.zeros(3, np.uint64), np.full(3, KC_LONG + 1, np.uint32)
    st1 = statement(21, [read])
    with counter(21, 1 << 13) as h:
        if path == "block":
            h.count_block(seq, offs, lens)
        else:
            dev = torch.device("cuda:0")
            d = [torch.from_numpy(a.copy()).to(dev) for a in (seq, offs.view(np.int64), lens.view(np.int32))]
            h.count_device(d[0].data_ptr(), seq.size, d[1].data_ptr(), d[2].data_ptr(), 3)
        for _ in range(2):                                  # sticky
            with pytest.raises(vafc.VafcError) as e:
                h.finish()
            assert e.value.code == vafc.VC_EINVAL
        with pytest.raises(vafc.VafcError) as e:
            h.histogram()
        assert e.value.code == vafc.VC_EINVAL
        h.reset()
        h.count_block(seq, offs[:1], lens[:1])
        assert h.finish()[1] == st1[1]
        check_whole(h, st1)


# --- GPU: the Bloom replay at library level ------------------------------------

def yak_gpu(h, row, calls1, reads2, n_parts=1):
    """track_first, file 1 (one count_block per entry of calls1), select, file 2, histogram"""
    k, pre, bf_shift, n_hash = row
    total, kept = np.zeros(1024, np.uint64), 0
    for part in range(n_parts):
        if n_parts > 1:
            h.set_partition(n_parts, part)
        h.track_first(True)
        for reads in calls1:
            h.count_block(*pack(reads))
        h.finish()
        h.yak_bloom_select(pre, bf_shift, n_hash)
        h.count_block(*pack(reads2))
        h.finish()
        hist, d, _ = h.histogram(1024, 0)
        assert d == hist.sum()
        total += hist
        kept += d
    return total, kept


def probe_of(k, reads, first, keys):
    """One k-base read per key: the bases of its first occurrence"""
    return [reads[r][j - k + 1:j + 1] for r, j in (first[h] for h in keys)]


def check_yak(h, row, shape="a", kind="short", cuts=None, n_parts=1):
    f1 = yak_shape(shape, row[0])
    calls = [f1] if cuts is None else [f1[a:b] for a, b in zip(cuts, cuts[1:])]
    want, kept = yak_want(row, shape, kind)
    hist, d = yak_gpu(h, row, calls, yak_file2(kind, row[0]), n_parts)
    assert d == len(kept)
    assert np.array_equal(hist, want)


def check_yak_identity(h, row, shape="a"):
    k = row[0]
    f1 = yak_shape(shape, k)
    counts, _, first = yak_st1(k, shape)
    _, kept = yak_want(row, shape)
    # every key of file 1 once: all kept keys are keys of file 1
    hist, d = yak_gpu(h, row, [f1], probe_of(k, f1, first, list(counts)))
    assert d == len(kept) and hist[1] == len(kept) and hist[0] == 0 and hist[2:].sum() == 0
    # the stated kept keys once, the others not at all: the kept keys are those
    hist, d = yak_gpu(h, row, [f1], probe_of(k, f1, first, sorted(kept)))
    assert d == len(kept) and hist[1] == len(kept) and hist[0] == 0 and hist[2:].sum() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("row", YAK_ROWS, ids=ROW_IDS)
def test_yak_replay_rows(row):
    with counter(row[0], YAK_SLOTS[row[0]]) as h:
        check_yak(h, row)
        check_yak_identity(h, row)


@pytest.mark.gpu
@pytest.mark.parametrize("row", YAK_ROWS[:3], ids=ROW_IDS[:3])
def test_yak_replay_shapes_of_file_1(row):
    with counter(row[0], YAK_SLOTS[row[0]]) as h:
        check_yak(h, row, "b")                              # every stamp from the long-read kernel
        check_yak_identity(h, row, "b")
        check_yak(h, row, "c")                              # short and long reads in one block
        check_yak_identity(h, row, "c")
        for cuts in ([0, 600], [0, 217, 600], [0, 1, 100, 101, 350, 600]):
            check_yak(h, row, "a", cuts=cuts)               # read_base carries the stream order over calls
        check_yak(h, row, "c", cuts=[0, 31, 32, 200, len(yak_shape("c"))])
        check_yak(h, row, "a", n_parts=3)
        h.set_partition(1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["long", "absent", "empty"])
def test_yak_replay_file_2(kind):
    row = YAK_ROWS[0]
    with counter(row[0], YAK_SLOTS[row[0]]) as h:
        check_yak(h, row, "a", kind)
        check_yak(h, row, "b", kind)

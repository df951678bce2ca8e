"""The scan fixture (tests/scan_fixture.py) against the oracle alone, no GPU:
the classes hold the shapes they claim, the expected counts are what the
oracle counts, and the seq_nt4 restatement agrees with test_spg's."""
import numpy as np
import pytest

import scan_fixture as F

KS = (1, 5, 9, 15) + tuple(range(16, 32))


def _windows(k, read):
    import oracle as O
    return int(O.read_kmers(k, read).size)


def test_layout_is_whole_waves_at_every_alignment():
    s = F.scan_set(21)
    assert len(s.spans) == len(s.classes) and s.offs.size == s.lens.size == s.spans[-1][1]
    align = set()
    for i, (c, (a, b)) in enumerate(zip(s.classes, s.spans)):
        assert a % F.WAVE == 0 and b % F.WAVE == 0 and b - a >= len(c.reads) > 0
        assert a == (s.spans[i - 1][1] if i else 0)
        for j, r in enumerate(c.reads):
            o = int(s.offs[a + j])
            assert int(s.lens[a + j]) == len(r) and s.seq[o:o + len(r)].tobytes() == r
        assert not s.lens[a + len(c.reads):b].any()
        align.add(int(s.offs[a]) & 3)
    assert align == {0, 1, 2, 3}
    assert np.all(s.offs + s.lens <= s.seq.size)
    # the same seed gives the same bytes
    again = F.layout(F.all_classes(21))
    assert np.array_equal(again[0], s.seq) and np.array_equal(again[1], s.offs)


def test_class_a_holds_every_trip_count_and_tail_length():
    """nit = ceil(L / 16) in 1..13 and every len & 15; for K >= 18 the chunk-1
    skip needs nit >= 6, and the half last chunk is taken iff the last chunk
    holds at most 8 bases of every lane."""
    cls = F.classes_a()
    assert all(len(c.reads) == F.WAVE and {len(r) for r in c.reads} == {c.tag["L"]} for c in cls)
    Ls = [c.tag["L"] for c in cls]
    nit = {(L + 15) >> 4 for L in Ls}
    assert nit == set(range(1, 14))
    for n in nit:    # every tail length, and both sides of the half-chunk test, at every trip count
        last = {L - 16 * (n - 1) for L in Ls if (L + 15) >> 4 == n}
        assert last == set(range(1, 17))
    assert {(n - 1) % 4 or 4 for n in nit if n > 1} == {1, 2, 3, 4}     # chunks left after the peel and the trips
    s = F.scan_set_a(21)
    assert s.seq.size == sum(64 * L for L in Ls) + sum(i % 4 for i in range(len(Ls)))


@pytest.mark.parametrize("k", KS)
def test_keys_all_occur_and_stay_below_the_second_level_threshold(k):
    s = F.scan_set(k)
    assert s.keys.size == s.n_present == np.unique(s.keys).size
    assert 0 < s.keys.size < F.L2F_MIN_KEYS
    assert int(s.want[:s.n_present].min()) >= 1 and not s.want[s.n_present:].any()
    assert int(s.want.astype(np.int64).sum()) == s.tally > 0
    assert np.array_equal(np.minimum(s.keys, F.revcomp(s.keys, k)), s.keys)


@pytest.mark.parametrize("k", (9, 16, 21, 31))
def test_expected_counts_are_the_oracles_whole_set_pass(k):
    """The per-read extraction added up (the fixture's expectation) equals
    the oracle's table pass over the whole buffer, for the small and the large
    key set."""
    import oracle as O
    for large in (False, True) if k >= 16 else (False,):
        s = F.scan_set(k, large)
        want, km = O.Oracle(k, keys=s.keys, vals=s.vals).count_reads(s.seq, s.offs, s.lens, n_patterns=s.n_pat)
        assert km == s.tally
        assert np.array_equal(want, s.want)
        if large:
            assert s.keys.size == s.n_present + F.N_ABSENT > F.L2F_MIN_KEYS
            assert np.unique(s.keys).size == s.keys.size


@pytest.mark.parametrize("k", (5, 16, 21, 31))
def test_bdiag_window_counts(k):
    """One bad byte at p leaves max(0, p - k + 1) + max(0, L - p - k) windows.
    'N' and 0x80 are invalid everywhere.  'S' is C to the head decode (the
    first 16 (L // 16) bytes) and invalid to seq_nt4_table (the tail); 0x00 is
    the reverse: invalid in the head, A in the tail (seq_nt4_table maps bytes
    0..3 to themselves)."""
    for c in F.classes_bdiag():
        L, byte = c.tag["L"], c.tag["byte"]
        head = 16 * (L // 16)
        for p, r in enumerate(c.reads):
            cut = max(0, p - k + 1) + max(0, L - p - k)
            whole = max(0, L - k + 1)
            if byte == 0x53:
                want = whole if p < head else cut
            elif byte == 0x00:
                want = cut if p < head else whole
            else:
                want = cut
            assert _windows(k, r) == want, (L, byte, p)


@pytest.mark.parametrize("k", (16, 21))
def test_tail_classes_separate_the_two_decodes(k):
    """Every byte of the T classes sits in the tail; the head decode would
    count differently (validity for 'S', 0x00 and 0x02, the code for 0x01)."""
    import oracle as O
    seen = set()
    for c in F.classes_t():
        if c.name != "Tdiag":
            continue
        L, byte = c.tag["L"], c.tag["byte"]
        assert len(c.reads) == L - F.T_BASE == L & 15
        seen.add((L & 15, byte))
        for p, r in enumerate(c.reads):
            assert r[F.T_BASE + p] == byte
            cut = max(0, F.T_BASE + p - k + 1) + max(0, L - (F.T_BASE + p) - k)
            valid = F.nt4_table()[byte] < 4
            assert _windows(k, r) == (L - k + 1 if valid else cut)
            # as a head byte (the same read, 16 bases longer) it decodes differently
            longer = r + b"ACGTACGTACGTACGT"
            if byte == 0x75:
                continue     # 'u' is T to both decodes
            as_head = O.read_kmers(k, longer)
            as_tail = F.nt4_kmers(k, [longer])
            assert as_head.size != as_tail[2] or not np.array_equal(np.unique(as_head), as_tail[0])
    assert seen == {(t, b) for t in range(1, 16) for b in F.T_BYTES}


def test_long_read_classes_put_defects_at_every_segment_border():
    k = 21
    cls = F.classes_c(k)
    clean = [c for c in cls if c.tag["byte"] is None]
    assert [c.tag["L"] for c in clean] == list(F.C_LENGTHS)
    assert F.c_borders(16385) == [256, 16384] and F.c_borders(16641) == [256, 16384, 16640]
    for c in cls:
        if c.tag["byte"] is None:
            continue
        L, b = c.tag["L"], c.tag["border"]
        pos = [int(np.flatnonzero(np.frombuffer(r, np.uint8) == c.tag["byte"])[0]) if c.tag["byte"] else None
               for r in c.reads]
        want = [p for p in range(b - k, b + 2) if p < L]
        assert len(c.reads) == len(want) and all(len(r) == L for r in c.reads)
        if c.tag["byte"]:
            assert pos == want


def test_nt4_restatement_matches_test_spg():
    """nt4_kmers against test_spg._oracle_counts (the rolling loop of
    count_candidate_kmers) on a few hundred of the reads it is used on."""
    from test_spg import _oracle_counts
    rng = np.random.default_rng(5)
    reads = F.padded_reads(F.nt4_classes())
    reads = [reads[i] for i in rng.permutation(len(reads))[:300]] + [c.reads[-1] for c in F.classes_t()]
    for k in (17, 21):
        keys, mult, tally = F.nt4_kmers(k, reads)
        assert keys.size > 100 and tally == int(mult.sum())
        extra = F.absent_keys(k, keys, 50)
        allk = np.concatenate([keys, extra])
        want = _oracle_counts(k, reads, allk)
        assert np.array_equal(want[:keys.size], mult) and not want[keys.size:].any()

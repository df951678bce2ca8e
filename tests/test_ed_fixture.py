"""The ed fixture (tests/ed_fixture.py) on the CPU alone: every class produces
the layout event it is named for under the layout model, the statement's
counts differ from what three faulty kernels would count, the fast form of
the statement equals the plain table, and the query sets reach all 24 kernel
shapes."""
import time

import numpy as np
import pytest

import ed_fixture as F

_STATE = {}


def _sets():
    """{alphabet: (alphabet, classes, scores)}: the whole fixture's statement,
    built once per module and timed."""
    if not _STATE:
        t0 = time.perf_counter()
        _STATE["sets"] = {name: F.prepared(name) for name in F.ALPHABETS}
        _STATE["seconds"] = time.perf_counter() - t0
    return _STATE["sets"]


def _classes(alphabet, name):
    out = [c for c in _sets()[alphabet][1] if c.name == name]
    assert out, (alphabet, name)
    return out


def _layout(c):
    return F.layout([len(r) for r in c.reads])


# ---------------------------------------------------------------------------
# the layout model and the intended layouts
# ---------------------------------------------------------------------------

def test_constants_are_the_headers():
    assert (F.CHUNK, F.SEGS, F.MAX_WAVES, F.LDS_MASKS) == (4096, 64, 4, 32768)


def test_layout_model_on_plain_cases():
    assert F.layout([]) == []
    assert F.layout([0]) == [F.Chunk([F.Seg(0, 0, 0, True, True)], None)]
    assert F.layout([5, 3]) == [F.Chunk([F.Seg(0, 0, 5, True, True), F.Seg(1, 8, 11, True, True)], None)]
    assert F.layout([4097]) == [F.Chunk(None, F.Piece(0, 0, True)), F.Chunk([F.Seg(0, 0, 1, False, True)], None)]
    ch = F.layout([12289, 7])
    assert [c.piece for c in ch[:3]] == [F.Piece(0, 0, True), F.Piece(0, 4096, False), F.Piece(0, 8192, False)]
    assert ch[3].segs == [F.Seg(0, 0, 1, False, True), F.Seg(1, 4, 11, True, True)]
    # every read ends in exactly one segment, in order, whatever the lengths
    rng = np.random.default_rng(1)
    for _ in range(50):
        lens = [int(x) for x in rng.choice([0, 1, 3, 4, 30, 1000, 4092, 4093, 4096, 4097, 9000], 90)]
        segs = [s for c in F.layout(lens) if c.segs for s in c.segs]
        assert [s.read for s in segs] == list(range(len(lens)))
        for c in F.layout(lens):
            if c.segs:
                assert len(c.segs) <= F.SEGS and c.segs[-1].end <= F.CHUNK
                assert all(s.beg % 4 == 0 and s.beg <= s.end for s in c.segs)
                assert all(a.end <= b.beg for a, b in zip(c.segs, c.segs[1:]))
        for i, n in enumerate(lens):
            assert F.tail_done(F.layout(lens), i) + (segs[i].end - segs[i].beg) == n


def test_range_cuts():
    assert F.range_cuts(7, 1) == [(0, 7)]
    assert F.range_cuts(7, 2) == [(0, 4), (4, 7)]
    assert F.range_cuts(7, 3) == [(0, 3), (3, 6), (6, 7)]
    assert F.range_cuts(7, 100) == [(i, i + 1) for i in range(7)]


def test_class_p_covers_the_take_edges():
    for alphabet in F.ALPHABETS:
        cls = _classes(alphabet, "P")
        assert [c.tag["cut"] for c in cls] == list(F.P_CUTS)
        takes, tails = set(), set()
        text = cls[-1].reads[0]
        for c in cls:
            ch, n = _layout(c), c.tag["cut"]
            assert len(c.reads[1]) == 30 and c.reads[0] == text[:n]
            pieces = [x.piece for x in ch if x.piece]
            assert len(pieces) == (n - 1) // F.CHUNK and [p.starts for p in pieces] == [True, False][:len(pieces)]
            first = next(x.segs[0] for x in ch if x.segs)
            assert first.read == 0 and first.starts == (not pieces)
            tails.add(first.end - first.beg)
            for rem in range(n, 0, -F.CHUNK):             # lane 0's take in every chunk of the read
                takes.add(F.CHUNK + 4 if rem > F.CHUNK else (rem + 3) & ~3)
            if n % F.CHUNK in (1, 2, 3, 4, 5):          # the marker shares the tail's chunk
                assert [s.read for s in ch[-1].segs] == [0, 1]
        assert takes == {4, 8, 4092, 4096, 4100} and {1, 2, 3, 4, 5, 4092, 4093, 4096} <= tails
    # rem of 4,093..4,096 rounds to a take of 4,096; 4,097 and more take the CHUNK + 4 branch
    assert [len(F.layout([n])) for n in (4092, 4093, 4096, 4097, 4100, 4101)] == [1, 1, 1, 2, 2, 2]


def test_class_x_fills_a_chunk_exactly():
    cls = _classes("small", "X")
    assert len(cls) == 8
    for c in cls:
        ch = _layout(c)
        if c.tag["sum"] == "4096":
            assert len(ch[0].segs) == 4 and ch[0].segs[-1].end == c.tag["last"] + 3072
            assert (ch[0].segs[-1].end + 3) & ~3 == F.CHUNK
            assert [s.read for s in ch[1].segs] == [4]
        else:       # four bytes more: the fourth read moves to the next chunk
            assert [s.read for s in ch[0].segs] == [0, 1, 2] and [s.read for s in ch[1].segs] == [3, 4]
    assert any(_layout(c)[0].segs[-1].end == F.CHUNK for c in cls)


def test_class_g_cuts_at_64_reads():
    for alphabet in F.ALPHABETS:
        cls = _classes(alphabet, "G")
        by = {next(iter(c.tag)): c for c in cls if "empty" not in c.tag}
        for c in cls:
            if "empty" in c.tag:
                n = c.tag["empty"]
                sizes = [len(x.segs) for x in _layout(c)]
                assert sizes == [64] * ((n + 1) // 64) + ([(n + 1) % 64] if (n + 1) % 64 else [])
        c64 = next(c for c in cls if c.tag.get("empty") == 64)
        ch = _layout(c64)      # the 65th read would fit by bytes: it goes to the next chunk
        assert len(ch[0].segs) == 64 and ch[0].segs[-1].end == 0 and [s.read for s in ch[1].segs] == [64]
        ch = _layout(by["tiny"])
        assert len(ch[0].segs) == 64 and ch[0].segs[-1].end <= 256 and [s.read for s in ch[1].segs] == [64]
        assert {len(r) for r in by["tiny"].reads[:64]} == {1, 2, 3, 4}
        ch = _layout(by["behind_full_tail"])
        assert ch[0].piece and [(s.beg, s.end, s.starts) for s in ch[1].segs] == [
            (0, 4096, False), (4096, 4096, True), (4096, 4096, True), (4096, 4096, True)]


def test_class_t_shares_the_tails_chunk():
    cls = _classes("small", "T")
    assert [c.tag["tail"] for c in cls] == [1, 4, 5, 100, 100]
    for c in cls:
        ch = _layout(c)
        assert ch[0].piece == F.Piece(0, 0, True)
        first = ch[1].segs[0]
        assert (first.read, first.starts, first.end - first.beg) == (0, False, c.tag["tail"])
        assert len(ch[1].segs) > 1 and all(s.starts for s in ch[1].segs[1:])
        if "fills" in c.tag:
            assert ch[1].segs[-1].end == F.CHUNK and [s.read for s in ch[2].segs] == [5]


def test_class_l_long_after_short():
    long, unfit = _classes("small", "L")
    ch = _layout(long)
    assert [s.read for s in ch[0].segs] == [0, 1, 2, 3] and ch[1].piece == F.Piece(4, 0, True)
    assert ch[2].segs[0] == F.Seg(4, 0, 5000 - F.CHUNK, False, True)
    ch = _layout(unfit)
    assert [s.read for s in ch[0].segs] == [0, 1, 2, 3] and not any(c.piece for c in ch)
    assert len(unfit.reads[4]) <= F.CHUNK and ch[1].segs[0] == F.Seg(4, 0, 4050, True, True)


def test_class_s_puts_the_second_read_where_the_first_was():
    for alphabet in F.ALPHABETS:
        alpha = _sets()[alphabet][0]
        cls = _classes(alphabet, "S")
        assert {(c.tag["width"], c.tag["residue"]) for c in cls} == {(w, r) for w in F.WIDTH_NAMES for r in (1, 2, 3)}
        for c in cls:
            ch = _layout(c)
            assert len(ch) == 2 and len(ch[0].segs) == 64 and len(ch[1].segs) == 1
            a, b = ch[0].segs[0], ch[1].segs[0]
            assert a.beg == b.beg == 0 and b.end == a.end - 1 and b.end % 4 == c.tag["residue"]
            q = c.reads[0][-c.tag["m"]:]
            assert q in alpha.bases[F.WIDTH_NAMES.index(c.tag["width"])] and c.reads[-1] == c.reads[0][:-1]
            stale = F.stale_behind(c.reads, alpha.other)
            assert stale[64][:1] == q[-1:] and len(stale[64]) == 4 - c.tag["residue"]
            assert set(stale[0]) <= set(alpha.other)


def test_class_r_is_cut_differently_by_every_max_ranges():
    (c,) = _classes("small", "R")
    lens = [len(r) for r in c.reads]
    seen = set()
    for mr in (1, 2, 3, len(lens)):
        cuts = F.range_cuts(len(lens), mr)
        assert cuts[0][0] == 0 and cuts[-1][1] == len(lens)
        seen.add(tuple(len(F.layout(lens[a:b])) for a, b in cuts))
    assert len(seen) == 4


# ---------------------------------------------------------------------------
# the fixture tells faulty kernels from the right one
# ---------------------------------------------------------------------------

def _differs(fault, alphabet, name, width, keep=lambda c: True, queries=slice(None)):
    """(tag, e) of the lists on which the faulty counts of `queries` (of the
    width's 13 bases) differ from the statement's."""
    _, _, scores = _sets()[alphabet]
    found = []
    for c in _classes(alphabet, name):
        if not keep(c):
            continue
        for e in F.E_VALUES:
            want = scores.expected(c.reads, width, e)[queries]
            if not np.array_equal(want, F.faulty_counts(fault, scores, c.reads, width, e)[queries]):
                found.append((c.tag, e))
    return found


@pytest.mark.parametrize("width", F.WIDTHS)
def test_fault_1_a_tail_that_resets_the_state(width):
    for alphabet in F.ALPHABETS:
        found = _differs(1, alphabet, "P", width, queries=slice(0, 1))
        assert {t["cut"] for t, _ in found} == {n for n in F.P_CUTS if n > F.CHUNK}, alphabet
    # every T list shows it
    assert len({str(t) for t, _ in _differs(1, "small", "T", width)}) == len(_classes("small", "T"))


@pytest.mark.parametrize("width", F.WIDTHS)
def test_fault_2_a_piece_that_resets_the_state(width):
    for alphabet in F.ALPHABETS:
        assert not _differs(2, alphabet, "P", width, lambda c: c.tag["cut"] <= 2 * F.CHUNK)
        found = _differs(2, alphabet, "P", width, lambda c: c.tag["cut"] > 2 * F.CHUNK)
        assert {t["cut"] for t, _ in found} == set(range(8193, 8198)), alphabet
        # the first base alone shows it: a handle with one query per width has no other
        found = _differs(2, alphabet, "P", width, lambda c: c.tag["cut"] > 2 * F.CHUNK, slice(0, 1))
        assert {t["cut"] for t, _ in found} == set(range(8193, 8198)), alphabet


@pytest.mark.parametrize("width", F.WIDTHS)
def test_fault_3_a_walk_that_ignores_the_clamp(width):
    for alphabet in F.ALPHABETS:
        found = _differs(3, alphabet, "S", width, lambda c: c.tag["width"] == F.WIDTH_NAMES[width])
        # every residue, at the exact search: the stale byte completes the copy
        assert {t["residue"] for t, e in found if e == 0} == {1, 2, 3}, (alphabet, found)


# ---------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------

def test_checkpoints_equal_separate_scans():
    alpha, _, scores = _sets()["small"]
    rng = np.random.default_rng(2)
    t = bytes(alpha.text(rng, 400))
    for m, (ids, mat) in scores.mats.items():
        marks = [1, 2, m, 399, 400]
        at = F.scan_read_at(mat, t, marks)
        assert sorted(at) == sorted(set(marks))
        for n in marks:
            best, cnt = F.scan_read(mat, t[:n])
            assert np.array_equal(at[n][0], best) and np.array_equal(at[n][1], cnt)


def test_fast_form_equals_dp_on_the_fixture():
    """Every read of at most 300 bytes and three windows of the long text,
    every base query, every e."""
    for alphabet in F.ALPHABETS:
        alpha, classes, scores = _sets()[alphabet]
        p_text = next(c for c in classes if c.name == "P" and c.tag["cut"] == 8197).reads[0]
        reads = {r for c in classes for r in c.reads if len(r) <= 300}
        reads |= {p_text[at:at + 140] for at in (F.CHUNK - 70, 2 * F.CHUNK - 100, 660)}
        assert len(reads) > 20
        for t in sorted(reads):
            for w in F.WIDTHS:
                for e in F.E_VALUES:
                    want = [F.dp_hits(q, t, e) for q in alpha.bases[w]]
                    assert scores.counts(t, w, e).tolist() == want, (alphabet, w, e, t)


def test_every_class_counts_something_for_every_e():
    for alphabet in F.ALPHABETS:
        _, classes, scores = _sets()[alphabet]
        for c in classes:
            for e in F.E_VALUES:
                total = sum(int(scores.expected(c.reads, w, e).sum()) for w in F.WIDTHS)
                assert total > 0, (alphabet, c.name, c.tag, e)
    # an empty read counts 1 for every query: the G lists count their reads
    _, classes, scores = _sets()["small"]
    marker = classes[0].reads[1]
    for c in _classes("small", "G"):
        if "empty" in c.tag:
            for w in F.WIDTHS:
                assert np.array_equal(scores.expected(c.reads, w, 0),
                                      c.tag["empty"] + scores.expected([marker], w, 0))


# ---------------------------------------------------------------------------
# queries and shapes
# ---------------------------------------------------------------------------

def test_query_sets():
    for alphabet in F.ALPHABETS + ("t31", "t32", "t63", "t64"):
        alpha = F.alphabet(alphabet)
        for w in F.WIDTHS:
            assert len(set(alpha.bases[w])) == F.N_BASE
            assert {len(q) for q in alpha.bases[w]} == set(F.WIDTH_LENGTHS[w])
            assert all(F.width_of(len(q)) == w for q in alpha.bases[w])
            qs = alpha.queries(w, 257)
            assert all(qs[i] == alpha.bases[w][i % 13] for i in range(257))
            # no shift by a power of two maps a query onto an equal one
            assert all(qs[i] != qs[i + d] for d in (1, 2, 4, 8, 16, 32, 64, 128) for i in range(257 - d))
        if alphabet.startswith("t"):     # a single width's queries hold every symbol
            for w in F.WIDTHS:
                assert F.n_class_of(alpha.queries(w, 64)) == len(alpha.symbols) + 1
    assert F.n_class_of(F.handle_queries(F.alphabet("small"), 1)[0]) == 5
    for alphabet, n_used in (("wide256", 256), ("wide255", 255)):
        alpha = F.alphabet(alphabet)
        assert len(set(b"".join(alpha.bases[F.W128][:3]))) == n_used >= 200
        for n in F.N_QUERIES:
            queries, where = F.handle_queries(alpha, n)
            assert F.n_class_of(queries) == 256
            assert [len(x) for x in where] == [n, n, max(n, 3)]
            for w in F.WIDTHS:
                assert [queries[j] for j in where[w]] == alpha.queries(w, len(where[w]))
    assert alpha.other[0] not in alpha.symbols and F.alphabet("wide256").other == b"\0"


def test_model_covers_every_shape():
    shapes, groups, sizes = set(), {}, set()
    for alphabet in F.ALPHABETS:
        alpha = F.alphabet(alphabet)
        for n in F.N_QUERIES:
            queries, where = F.handle_queries(alpha, n)
            nc = F.n_class_of(queries)
            for w in F.WIDTHS:
                g, waves, lds = F.expected_shape(nc, w, len(where[w]))
                assert lds == (alphabet == "small")
                shapes.add((w, waves, lds))
                groups.setdefault((w, waves, lds), set()).add(g)
                sizes.add((w, len(where[w]) - 64 * (g - 1)))
    assert shapes == {(w, waves, lds) for w in F.WIDTHS for waves in (1, 2, 3, 4) for lds in (True, False)}
    for w in F.WIDTHS:
        for lds in (True, False):
            assert 5 in groups[(w, 4, lds)]      # a second block with three idle waves
        assert {(w, 64), (w, 1)} <= sizes        # a full last group, and one query with 63 idle lanes
    assert F.expected_shape(5, F.W32, 0) == (0, 1, True)
    # at the limit and one class above it
    for w, n, nc in ((F.W32, 193, 32), (F.W64, 64, 64), (F.W128, 64, 32)):
        assert F.expected_shape(nc, w, n)[2] and not F.expected_shape(nc + 1, w, n)[2]


def test_statement_is_cheap_enough():
    _sets()
    print("ed fixture statement: %.1f s" % _STATE["seconds"])
    assert _STATE["seconds"] < 20

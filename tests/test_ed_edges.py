"""The approximate-search kernel (csrc/vafc_ed.hip) in every launch shape, at
every chunk-layout edge (needs an MI355X): the query sets and read classes of
tests/ed_fixture.py -- three word widths x 1..4 waves per block x match masks
in LDS or in HBM; reads whose takes land on a chunk's last byte, the 64-read
cut, tails that share a chunk, pieces after segments, a stale class byte
behind a read -- each class counted alone as one read range and compared
exactly with the statement.  A failure names the alphabet, the width, its
waves and mask placement, -e, the class and the first wrong query.

The shapes are read back from the handle (vc_ed_shape) and compared with the
fixture's restatement of the host rule, and the last test checks that all 24
were launched: a change of the rule cannot quietly shrink the matrix."""
import numpy as np
import pytest

import ed_fixture as F

pytestmark = pytest.mark.gpu

SHAPES_SEEN = set()       # (width, waves, lds_masks) of every handle test_every_shape_walks_every_class made
MATRIX = [(a, n) for a in F.ALPHABETS for n in F.N_QUERIES]
_matrix_cases_run = []
_expected = {}


def pack(reads):
    lens = np.array([len(r) for r in reads], np.uint32)
    offs = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    blob = np.frombuffer(b"".join(reads), np.uint8) if lens.sum() else np.zeros(0, np.uint8)
    return blob, offs, lens


def _want(alphabet, scores, ci, c, w, e):
    key = (alphabet, c.name, str(c.tag), ci, w, e)
    if key not in _expected:
        _expected[key] = scores.expected(c.reads, w, e)
    return _expected[key]


def _count(ed, reads, max_ranges=1):
    ed.set_max_ranges(max_ranges)
    ed.count_block(*pack(reads))
    got = ed.finish().copy()
    ed.reset()
    return got


def _compare(got, want13, where, queries, what):
    """got: the handle's counts; the queries of one width lie at `where`, the
    i-th of them expecting want13[i % 13]."""
    want = want13[np.arange(where.size) % F.N_BASE]
    mine = got[where]
    if np.array_equal(mine, want):
        return
    i = int(np.nonzero(mine != want)[0][0])
    pytest.fail("%s: %d of %d queries differ, first query %d of the width (length %d): counted %d, statement %d"
                % (what, int((mine != want).sum()), where.size, i, len(queries[where[i]]), int(mine[i]),
                   int(want[i])))


def _what(alphabet, w, shape, e, c):
    return "alphabet %s, %s x %d waves (%d groups), masks in %s, -e %d, class %s %r" % (
        alphabet, F.WIDTH_NAMES[w], shape[1], shape[0], "LDS" if shape[2] else "HBM", e, c.name, c.tag)


def _check_classes(ed, alphabet, classes, scores, queries, where, widths, e, max_ranges=1):
    shapes = {w: ed.shape(w) for w in widths}
    for ci, c in enumerate(classes):
        got = _count(ed, c.reads, max_ranges)
        for w in widths:
            _compare(got, _want(alphabet, scores, ci, c, w, e), where[w], queries, _what(alphabet, w, shapes[w], e, c))


@pytest.mark.parametrize("alphabet,n_queries", MATRIX)
def test_every_shape_walks_every_class(alphabet, n_queries):
    """One handle with n_queries of every width (1, 1, 2, 3, 3, 4, 4 and 5
    groups: every number of waves, a full and a one-query last group, a second
    block with three idle waves), per -e; every class but R as one read range."""
    import vafc
    _matrix_cases_run.append((alphabet, n_queries))
    alpha, classes, scores = F.prepared(alphabet)
    classes = [c for c in classes if c.name != "R"]
    queries, where = F.handle_queries(alpha, n_queries)
    n_class = F.n_class_of(queries)
    for e in F.E_VALUES:
        ed = vafc.EdCounter(queries=queries, max_edit=e)
        try:
            for w in F.WIDTHS:
                shape = ed.shape(w)
                assert shape == F.expected_shape(n_class, w, where[w].size), (alphabet, F.WIDTH_NAMES[w], n_queries)
                assert shape[2] == (alphabet == "small")
                SHAPES_SEEN.add((w, shape[1], shape[2]))
            _check_classes(ed, alphabet, classes, scores, queries, where, F.WIDTHS, e)
        finally:
            ed.close()


@pytest.mark.parametrize("width,n_queries,at_limit,above", [(F.W32, 193, "t31", "t32"), (F.W64, 64, "t63", "t64"),
                                                            (F.W128, 64, "t31", "t32")],
                         ids=["W32x4_waves", "W64x1_wave", "W128x1_wave"])
def test_mask_placement_threshold(width, n_queries, at_limit, above):
    """Masks of exactly VC_ED_LDS_MASKS bytes stay in LDS, one class more sends
    them to HBM; both count classes S and G like the statement."""
    import vafc
    waves = min((n_queries + 63) // 64, F.MAX_WAVES)
    for name, lds in ((at_limit, True), (above, False)):
        alpha, classes, scores = F.prepared(name, "SG", (width,))
        queries = alpha.queries(width, n_queries)
        where = {width: np.arange(n_queries)}
        n_class = F.n_class_of(queries)
        assert n_class == len(alpha.symbols) + 1
        per_class = F.WIDTH_WORDS[width] * waves * 64 * F.WIDTH_WORDBYTES[width]
        assert n_class * per_class == F.LDS_MASKS + (0 if lds else per_class)
        for e in F.E_VALUES:
            ed = vafc.EdCounter(queries=queries, max_edit=e)
            try:
                assert ed.shape(width) == ((n_queries + 63) // 64, waves, lds), (name, e)
                for other in set(F.WIDTHS) - {width}:
                    assert ed.shape(other)[0] == 0
                _check_classes(ed, name, classes, scores, queries, where, (width,), e)
            finally:
                ed.close()


@pytest.mark.parametrize("alphabet,n_queries,waves", [("small", 257, 4), ("wide256", 65, 2)])
def test_range_cuts(alphabet, n_queries, waves):
    """Class R (the T and L lists in one) cut into 1, 2, 3 read ranges and one
    per read: a tail's followers, a long read and the reads before it fall
    into different blocks; the sums do not depend on the cut."""
    import vafc
    alpha, classes, scores = F.prepared(alphabet, "R")
    (c,) = classes
    queries, where = F.handle_queries(alpha, n_queries)
    for e in F.E_VALUES:
        ed = vafc.EdCounter(queries=queries, max_edit=e)
        try:
            assert [ed.shape(w)[1] for w in F.WIDTHS] == [waves] * 3
            for max_ranges in (1, 2, 3, len(c.reads)):
                tagged = [c._replace(tag=dict(c.tag, max_ranges=max_ranges))]
                _check_classes(ed, alphabet, tagged, scores, queries, where, F.WIDTHS, e, max_ranges)
        finally:
            ed.close()


def test_shape_of_a_width_without_queries_and_bad_arguments():
    import ctypes as C
    import vafc
    ed = vafc.EdCounter(queries=[b"ACGT"])
    try:
        assert ed.shape(F.W32) == (1, 1, True) and ed.shape(F.W64)[0] == 0 and ed.shape(F.W128)[0] == 0
        for width in (-1, 3):
            with pytest.raises(vafc.VafcError) as ei:
                ed.shape(width)
            assert ei.value.code == vafc.VC_EINVAL
        assert vafc.lib().vc_ed_shape(ed._h, 0, None, None, None) == vafc.VC_OK
        g = C.c_uint32(7)
        assert vafc.lib().vc_ed_shape(None, 0, C.byref(g), None, None) == vafc.VC_EINVAL and g.value == 7
    finally:
        ed.close()


def test_all_24_shapes_ran():
    """Last in the file: the matrix above launched every (width, waves, mask
    placement).  Skipped when the matrix was deselected or cut."""
    if sorted(_matrix_cases_run) != sorted(MATRIX):
        pytest.skip("test_every_shape_walks_every_class did not run in full")
    want = {(w, waves, lds) for w in F.WIDTHS for waves in range(1, F.MAX_WAVES + 1) for lds in (True, False)}
    assert len(want) == 24 and SHAPES_SEEN == want, sorted(want - SHAPES_SEEN)

"""The BAI reader and the seek plan (vc_bam_index_plan, include/vafc.h item 9 of
the bam contract) without a GPU: the library's spans against the plain
statement of tests/bam_seek_fixture.py on the goldens' htslib-made indexes, on
the fixture's own indexes for the same files and on a synthetic sorted file;
the coverage property (every record that overlaps a merged region starts
inside exactly one span); what makes an index not usable for seeking; the
piece classes of the fixture; and the parser, the planner and the piece walk
under AddressSanitizer and UBSan (tools/bam_index_asan.sh)."""
import os
import struct
import subprocess

import pytest

import bam_seek_fixture as S
from conftest import GOLDEN, ROOT

BAM = os.path.join(GOLDEN, "bam")
REAL = [("a.bam", "a.index"), ("b.bam", "b.bam.bai"), ("long.bam", "long.index")]


def read(name):
    with open(os.path.join(BAM, name), "rb") as f:
        return f.read()


_decoded = {}


def decoded(name):
    if name not in _decoded:
        _decoded[name] = S.decode(read(name))
    return _decoded[name]


def panel_regions(refs):
    """The merged regions of p.txt as the file pass builds them: build_regions,
    tids from this file's header, absent chromosomes skipped."""
    import vafc
    db = vafc.load_patterns(os.path.join(BAM, "p.txt"))
    tid_of = {nm: i for i, nm in enumerate(refs)}
    return [(tid_of[c], s, e) for c, s, e in vafc.build_regions(db) if c in tid_of]


def lib_plan(tmp_path, index: bytes, n_ref, regions, name="x.bai"):
    import vafc
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(index)
    return vafc.bam_index_plan(None, n_ref, regions, index_fn=path)


@pytest.mark.parametrize("bam,index", REAL)
def test_plan_on_the_real_indexes(bam, index, tmp_path):
    d = decoded(bam)
    regions = panel_regions(d.refs)
    assert regions and S.wanted(d, regions)
    raw = read(index)
    want = S.py_plan(raw, len(d.refs), regions)
    got = lib_plan(tmp_path, raw, len(d.refs), regions)
    assert want and got == want
    assert S.covered(d, regions, got) is None


@pytest.mark.parametrize("bam,index", REAL)
@pytest.mark.parametrize("meta,no_coor", [(True, True), (False, False)])
def test_the_fixtures_index_passes_the_same_property(bam, index, meta, no_coor, tmp_path):
    d = decoded(bam)
    regions = panel_regions(d.refs)
    mine = S.write_bai(d, meta, no_coor)
    assert S.parse_bai(mine, len(d.refs)) is not None
    want = S.py_plan(mine, len(d.refs), regions)
    assert want and S.covered(d, regions, want) is None
    assert lib_plan(tmp_path, mine, len(d.refs), regions) == want
    # the same bins hold the same records' starts as in the real index
    real, own = S.parse_bai(read(index), len(d.refs)), S.parse_bai(mine, len(d.refs))
    for (rb, _rl), (ob, _ol) in zip(real, own):
        assert set(rb) == set(ob)
        for b in rb:
            assert [c[0] for c in rb[b]] == [c[0] for c in ob[b]], b


def test_index_found_beside_the_file(tmp_path):
    """index_path NULL: item 6's search order; a CSI found first is no seeking."""
    import vafc
    d = decoded("a.bam")
    regions = panel_regions(d.refs)
    path = str(tmp_path / "f.bam")
    with open(path, "wb") as f:
        f.write(read("a.bam"))
    assert vafc.bam_index_plan(path, len(d.refs), regions) is None          # no index
    with open(path + ".bai", "wb") as f:
        f.write(read("a.index"))
    assert vafc.bam_index_plan(path, len(d.refs), regions) == S.py_plan(read("a.index"), len(d.refs), regions)
    import bam_fixture as F
    with open(str(tmp_path / "f.csi"), "wb") as f:
        f.write(F.bgzf(b"CSI\1" + b"\0" * 40))
    assert vafc.bam_index_usable(path) == (True, str(tmp_path / "f.csi"))
    assert vafc.bam_index_plan(path, len(d.refs), regions) is None


@pytest.fixture(scope="module")
def sorted_file():
    raw = S.sorted_bam()
    d = S.decode(raw)
    return raw, d, S.write_bai(d)


def test_synthetic_sorted_file(sorted_file, tmp_path):
    raw, d, index = sorted_file
    assert len(d.recs) == 3000 and all(400 <= m.isize <= 1024 for m in d.members[:-1])
    assert [(r.tid, r.pos) for r in d.recs] == sorted((r.tid, r.pos) for r in d.recs)
    regions = S.SORTED_REGIONS
    want = S.py_plan(index, 2, regions)
    got = lib_plan(tmp_path, index, 2, regions)
    assert got == want and len(want) >= 3
    assert S.covered(d, regions, got) is None
    assert len(S.wanted(d, regions)) > 300
    read_members = S.span_members(d, got)
    assert read_members < set(range(len(d.members)))                      # a strict subset of the file's
    # regions in any order and one region twice: the same spans
    assert lib_plan(tmp_path, index, 2, regions[::-1] + regions[:1]) == want
    assert lib_plan(tmp_path, index, 2, []) == []


def test_many_regions_many_spans(tmp_path):
    """More than 64 spans: clusters far apart on both references."""
    clusters = [(t, 1_000_000 * (k + 1), 1_000_000 * (k + 1) + 200) for t in (0, 1) for k in range(70)]
    raw = S.sorted_bam(S.sorted_records(seed=11, n=6000, clusters=clusters))
    d = S.decode(raw)
    index = S.write_bai(d)
    want = S.py_plan(index, 2, clusters)
    assert len(want) > 64 and lib_plan(tmp_path, index, 2, clusters) == want
    assert S.covered(d, clusters, want) is None


def flip_chunk(index: bytes) -> bytes:
    """The first chunk of the first bin of the first reference that has one,
    with its two offsets exchanged."""
    at = 8
    n_bin, = struct.unpack_from("<I", index, at)
    assert n_bin
    b, n_chunk = struct.unpack_from("<II", index, at + 4)
    assert b != S.META_BIN and n_chunk
    beg, end = struct.unpack_from("<QQ", index, at + 12)
    assert beg < end
    return index[:at + 12] + struct.pack("<QQ", end, beg) + index[at + 28:]


def n_intv_at(index: bytes) -> int:
    """Where the first reference's n_intv stands: behind all of its bins."""
    n_bin, = struct.unpack_from("<I", index, 8)
    at = 12
    for _ in range(n_bin):
        n_chunk, = struct.unpack_from("<I", index, at + 4)
        at += 8 + 16 * n_chunk
    n_intv, = struct.unpack_from("<I", index, at)
    assert n_bin and 0 < n_intv and at + 4 + 8 * n_intv <= len(index)
    return at


def test_indexes_that_are_not_usable_for_seeking(tmp_path):
    d = decoded("a.bam")
    n_ref, regions = len(d.refs), panel_regions(d.refs)
    raw = read("a.index")
    assert lib_plan(tmp_path, raw, n_ref, regions)
    # every prefix: truncated.  One prefix is a whole BAI by the specification, the one that lacks
    # nothing but the optional n_no_coor; it plans as the whole file does.
    whole = S.py_plan(raw, n_ref, regions)
    for n in range(len(raw)):
        got = lib_plan(tmp_path, raw[:n], n_ref, regions)
        assert got == S.py_plan(raw[:n], n_ref, regions), n
        assert got is None or (n == len(raw) - 8 and got == whole), n
    assert S.py_plan(raw[:len(raw) - 8], n_ref, regions) == whole           # a.index carries n_no_coor
    for bad_n_ref in (n_ref - 1, n_ref + 1):
        assert lib_plan(tmp_path, raw, bad_n_ref, [r for r in regions if r[0] < bad_n_ref]) is None
    assert lib_plan(tmp_path, flip_chunk(raw), n_ref, regions) is None
    # counts that exceed the file: n_ref, n_bin, n_chunk, n_intv
    huge = struct.pack("<I", 0x7FFFFFF0)
    assert lib_plan(tmp_path, raw[:4] + huge + raw[8:], 0x7FFFFFF0, regions) is None
    assert lib_plan(tmp_path, raw[:8] + huge + raw[12:], n_ref, regions) is None
    assert lib_plan(tmp_path, raw[:16] + huge + raw[20:], n_ref, regions) is None
    at = n_intv_at(raw)                                                    # the first reference's n_intv, behind its bins
    assert lib_plan(tmp_path, raw[:at] + huge + raw[at + 4:], n_ref, regions) is None
    assert lib_plan(tmp_path, b"CSI\1" + raw[4:], n_ref, regions) is None
    assert lib_plan(tmp_path, raw + b"\0", n_ref, regions) is None          # bytes behind n_no_coor
    assert lib_plan(tmp_path, raw, n_ref, [(0, 5, S.MAX_POS + 1)]) is None    # past what a BAI's bins reach


def test_bad_arguments(tmp_path):
    import vafc
    raw = read("a.index")
    n_ref = len(decoded("a.bam").refs)
    for regions in ([(n_ref, 1, 2)], [(-1, 1, 2)], [(0, 5, 5)], [(0, -1, 5)]):
        with pytest.raises(vafc.VafcError) as ei:
            lib_plan(tmp_path, raw, n_ref, regions)
        assert ei.value.code == vafc.VC_EINVAL


@pytest.mark.parametrize("name", list(S.CLASSES))
def test_piece_classes_hold_what_they_are_named_for(name):
    """The fixture against itself: it passes without the piece walk and covers
    nothing of it; tests/test_bam_pieces.py and the sanitizer run below do."""
    case, want = S.case_of(name), S.want_of(name)
    assert len(case.text) < 100_000 and len(want.per_piece) == len(case.pieces)
    st = [p[0] for p in want.per_piece]
    if name == "stop":
        a, b = want.per_piece
        assert b[1] == a[1] + [case.pieces[0][1]] and a[0] == b[0] == S.OK
    elif name == "straddle":
        assert want.per_piece[1][1] == want.per_piece[0][1][:3] and len(want.per_piece[0][1]) == 5
    elif name == "cut":
        assert st == [S.OK] + [S.CUT] * 6 + [S.OK]
        assert [p[2] > 0 for p in want.per_piece] == [False, False, False, True, True, True, True, False]
        assert want.per_piece[-2][2] == 1
    elif name == "empty":
        assert [len(p[1]) for p in want.per_piece] == [0, 0, 0, 0, 0, 2] and set(st) == {S.OK}
    elif name == "adjacent":
        assert len(want.emitted) == len(set(want.emitted)) == 38
    elif name == "bad_entry":
        assert S.SHORT in st and want.irregular and len(want.irregular) == 2
    elif name == "mod4":
        assert {o % 4 for o in want.emitted} == {0, 1, 2, 3}
    elif name == "long":
        assert sum(1 for r in want.recs if len(r[3]) > 64) == 2
    elif name.startswith("n_"):
        n = int(name[2:])
        assert len(case.pieces) == n and sum(1 for p in want.per_piece if not p[1]) == n // 3 + (n % 3 == 2)
    if name not in ("empty", "cut"):
        assert want.plain.any()
    assert (want.plain != want.weighted).any() or not want.plain.any()


def test_index_and_pieces_under_the_sanitizers(tmp_path):
    """The parser and the planner over every golden index, every prefix of
    each and seeded byte flips, and the piece walk with a one-lane wave over
    the piece classes, compared with the statement."""
    n = S.write_cases(str(tmp_path))
    p = subprocess.run([os.path.join(ROOT, "tools", "bam_index_asan.sh"), str(tmp_path)], capture_output=True, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    assert out.count(" ok ") == n + len(REAL) and "bam_index_asan: all clean" in out

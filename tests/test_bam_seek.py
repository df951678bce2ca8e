"""bam-vaf-counter reading by its index ($VAFC_BAM_INDEX=seek; needs an
MI355X): every golden case that reads a file beside an index through the CLI,
against the reference's .vaf, stderr and exit code (the reference wrote them
reading through the same indexes); a synthetic sorted file in process against
the whole-file pass, per batch size and with more than 64 spans; every way the
pass gives a file up, byte for byte against a run without the variable and
with vc_bam_seek_info naming the reason; and a record longer than its span's
members, which the second reading completes.

tests/test_bam_seek_plan.py has the plan itself, without a GPU;
tests/test_bam_pieces.py the piece walk."""
import os
import re
import subprocess

import numpy as np
import pytest

import bam_fixture as F
import bam_seek_fixture as S
from bam_statement import make_counter
from test_bam import BAM_DIR, CLI, MANIFEST, assert_vaf_equals, golden_vaf, own_lines

pytestmark = pytest.mark.gpu

INDEXED = sorted(n for n, e in MANIFEST.items() if "Using indexed access" in e["stderr"])
PHASE = re.compile(r"^\[P::main\] (\S+): inflate host (\d+) device (\d+) members, (\d+) records, (\d+) bases, \S+ s"
                   r"(?:, seek state (\d+) spans (\d+) members (\d+) rereads (\d+))?$")
FALLBACK_FROM = 4                  # VC_BAM_SEEK_OFFSET


def run_cli(argv, cwd, seek=True, **env):
    e = dict(os.environ, VAFC_PHASES="1", **env)
    e.pop("VAFC_BAM_INDEX", None)
    e.pop("VAFC_BGZF", None)
    if seek:
        e["VAFC_BAM_INDEX"] = "seek"
    p = subprocess.run([CLI] + list(argv), cwd=str(cwd), capture_output=True, timeout=120, env=e)
    lines = p.stderr.decode().splitlines()
    phases = {}
    for m in filter(None, map(PHASE.match, lines)):
        phases[m.group(1)] = tuple(int(x) if x is not None else None for x in m.groups()[1:])
    stderr = own_lines("".join(ln + "\n" for ln in lines if not ln.startswith("[P::")))
    out = os.path.join(str(cwd), "o", "out.vaf")
    vaf = None
    if os.path.exists(out):
        with open(out, "rb") as f:
            vaf = f.read()
        os.unlink(out)
    return p.returncode, stderr, vaf, phases


def read(path):
    with open(path, "rb") as f:
        return f.read()


def link_goldens(tmp_path):
    for fn in os.listdir(BAM_DIR):
        os.symlink(os.path.join(BAM_DIR, fn), str(tmp_path / fn))
    os.mkdir(str(tmp_path / "o"))


def test_the_indexed_cases_are_there():
    """The manifest against this file's selection: it passes without the
    feature and covers nothing of it."""
    assert {"idx_bai", "idx_bam_bai", "long_idx", "two_headers_idx", "two_headers_swapped", "missing_second"} <= set(INDEXED)


@pytest.mark.parametrize("name", INDEXED)
def test_indexed_goldens_by_seeking(name, tmp_path):
    entry = MANIFEST[name]
    link_goldens(tmp_path)
    rc, stderr, vaf, phases = run_cli(entry["argv"], tmp_path)
    assert rc == entry["rc"] and stderr == entry["stderr"]
    out = str(tmp_path / "got.vaf")
    with open(out, "wb") as f:
        f.write(vaf)
    assert_vaf_equals(out, golden_vaf(name))
    sought = 0
    for fn, (host, device, _recs, _bases, state, spans, members, rereads) in phases.items():
        if os.path.exists(os.path.join(BAM_DIR, fn + ".bai")) or os.path.exists(os.path.join(BAM_DIR, fn[:-4] + ".bai")):
            assert (state, rereads) == (1, 0) and spans > 0 and device == members > 0, (fn, state, spans, members)
            sought += 1
        else:
            assert state == 2, (fn, state)                   # no index: not tried
    assert sought >= 1
    # and without the variable the line is the one it was
    plain = run_cli(entry["argv"], tmp_path, seek=False)
    assert plain[:3] == (rc, stderr, vaf) and all(p[4] is None for p in plain[3].values())


def write_sorted(tmp_path, records=None, regions=None, name="s.bam"):
    raw = S.sorted_bam(records)
    d = S.decode(raw)
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(raw)
    with open(path + ".bai", "wb") as f:
        f.write(S.write_bai(d))
    rows = S.sorted_rows(regions)
    return path, d, rows


def full_then_seek(bc, path, monkeypatch, batches=(None,)):
    monkeypatch.delenv("VAFC_BAM_INDEX", raising=False)
    monkeypatch.delenv("VAFC_BATCH_BYTES", raising=False)
    monkeypatch.delenv("VAFC_BGZF", raising=False)
    bc.reset()
    full_st = bc.count_file(path)
    want = bc.finish()
    full_members = sum(bc.inflate_info())
    assert bc.seek_info().name == "off" and want.any()
    out = []
    monkeypatch.setenv("VAFC_BAM_INDEX", "seek")
    for batch in batches:
        if batch:
            monkeypatch.setenv("VAFC_BATCH_BYTES", str(batch))
        bc.reset()
        st = bc.count_file(path)
        got = bc.finish()
        assert np.array_equal(got, want), (batch, np.nonzero(got != want)[0][:8])
        out.append((st, bc.seek_info(), bc.inflate_info()))
    return full_st, full_members, out


def test_sorted_file_in_process(tmp_path, monkeypatch):
    path, d, rows = write_sorted(tmp_path)
    spans = S.py_plan(S.write_bai(d), 2, S.SORTED_REGIONS)
    n_read = len(S.span_members(d, spans))
    bc = make_counter(rows, [r[0] for r in S.SORTED_REFS], tmp_path)
    try:
        full_st, full_members, runs = full_then_seek(bc, path, monkeypatch, (None, 3000, 70000))
        assert full_members >= len(d.members)
        for (st, sk, (host, device)), batch in zip(runs, (None, 3000, 70000)):
            assert (sk.name, sk.spans, sk.members, sk.rereads) == ("done", len(spans), n_read, 0), batch
            assert device == n_read < len(d.members) and host >= 1
            assert 0 < st.seqs < full_st.seqs and st.seqs >= len(S.wanted(d, S.SORTED_REGIONS))
        assert runs[0][0].blocks == 1 and runs[1][0].blocks >= 3
        assert (runs[0][0].seqs, runs[0][0].bases) == (runs[1][0].seqs, runs[1][0].bases) == (runs[2][0].seqs, runs[2][0].bases)
    finally:
        bc.close()


def test_more_than_64_spans(tmp_path, monkeypatch):
    clusters = [(t, 1_000_000 * (k + 1), 1_000_000 * (k + 1) + 200) for t in (0, 1) for k in range(70)]
    path, d, rows = write_sorted(tmp_path, S.sorted_records(seed=11, n=6000, clusters=clusters), clusters)
    spans = S.py_plan(S.write_bai(d), 2, clusters)
    assert len(spans) > 64
    bc = make_counter(rows, [r[0] for r in S.SORTED_REFS], tmp_path)
    try:
        _full, _members, runs = full_then_seek(bc, path, monkeypatch, (None, 3000))
        for _st, sk, (_host, device) in runs:
            assert (sk.name, sk.spans) == ("done", len(spans)) and device == len(S.span_members(d, spans)) < len(d.members)
    finally:
        bc.close()


def member_in_a_span(raw, index):
    """(offset, size) of the last member that a span of the file's plan reads;
    the header lies in a member before it."""
    d = S.decode(raw)
    import vafc
    db = vafc.load_patterns(os.path.join(BAM_DIR, "p.txt"))
    tid_of = {nm: i for i, nm in enumerate(d.refs)}
    regions = [(tid_of[c], s, e) for c, s, e in vafc.build_regions(db) if c in tid_of]
    spans = S.py_plan(index, len(d.refs), regions)
    k = sorted(S.span_members(d, spans))[-1]
    m = d.members[k]
    assert k > 2 and d.body <= d.members[0].isize
    return m.coff, m.size


def fallback_case(kind, tmp_path):
    """The files of one way to be given up, in tmp_path: (argv, state wanted)."""
    a = os.path.join(BAM_DIR, "a_i.bam")
    if kind == "stale":
        # the same text in members of 1,024 bytes: the index's offsets are another file's
        (tmp_path / "x.bam").write_bytes(F.bgzf(S.decode(read(a)).text, 1024))
        (tmp_path / "x.bam.bai").write_bytes(read(a + ".bai"))
        return ["x.bam"], "offset"
    if kind in ("flip", "cut"):
        # a.bam's text in members of 4,096 bytes, with the index the fixture writes for that file
        raw = F.bgzf(S.decode(read(a)).text, 4096)
        index = S.write_bai(S.decode(raw))
        off, size = member_in_a_span(raw, index)
        if kind == "flip":
            b = bytearray(raw)
            b[off + 18 + (size - 26) // 2] ^= 0x10
            raw = bytes(b)
        else:
            raw = raw[:off + size // 2]
        (tmp_path / "x.bam").write_bytes(raw)
        (tmp_path / "x.bam.bai").write_bytes(index)
        return ["x.bam"], "inflate" if kind == "flip" else "offset"
    if kind == "wrong_magic":
        return ["a_k.bam"], "no_index"
    if kind == "no_index":
        return ["a.bam"], "no_index"
    if kind == "csi":
        (tmp_path / "x.bam").write_bytes(read(a))
        (tmp_path / "x.bam.csi").write_bytes(F.bgzf(b"CSI\1" + b"\0" * 40))
        (tmp_path / "x.bam.bai").write_bytes(read(a + ".bai"))
        return ["x.bam"], "no_index"
    if kind == "second_file":
        fallback_case("flip", tmp_path)
        return ["a_i.bam", "x.bam", "b.bam"], None
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["stale", "flip", "cut", "wrong_magic", "no_index", "csi", "second_file"])
def test_files_given_up_are_read_as_without_the_variable(kind, tmp_path):
    import vafc
    link_goldens(tmp_path)
    files, state = fallback_case(kind, tmp_path)
    argv = ["-p", "p.txt", "-o", "o/out.vaf"] + files
    plain = run_cli(argv, tmp_path, seek=False)
    seek = run_cli(argv, tmp_path)
    assert seek[:3] == plain[:3] and plain[0] == 0 and plain[2] is not None
    names = vafc.BAM_SEEK_STATES
    if kind == "second_file":
        got = [names[seek[3][fn][4]] for fn in files]
        assert got == ["done", "inflate", "done"], got
        assert seek[3]["x.bam"][:4] == plain[3]["x.bam"][:4]                    # members, records, bases of the pass it fell back to
        alone = run_cli(argv[:-2], tmp_path)
        assert alone[2] != seek[2]                                              # the first file's counts are in the sum
    else:
        fn = files[0]
        assert names[seek[3][fn][4]] == state, seek[3][fn]
        assert seek[3][fn][:4] == plain[3][fn][:4]
        assert (seek[3][fn][4] >= FALLBACK_FROM) == (kind in ("stale", "flip", "cut"))


def test_fallback_restores_counts_in_process(tmp_path, monkeypatch):
    import vafc
    from test_bam import load_rows
    link_goldens(tmp_path)
    fallback_case("flip", tmp_path)
    db, _rows = load_rows(os.path.join(BAM_DIR, "p.txt"))
    a, bad = os.path.join(BAM_DIR, "a_i.bam"), str(tmp_path / "x.bam")
    bc = vafc.create_snp_map(db, a)
    try:
        monkeypatch.delenv("VAFC_BAM_INDEX", raising=False)
        for fn in (a, bad, a):
            bc.count_file(fn)
        want = bc.finish()
        bc.reset()
        monkeypatch.setenv("VAFC_BAM_INDEX", "seek")
        seen = []
        for fn in (a, bad, a):
            bc.count_file(fn)
            seen.append(bc.seek_info().name)
        assert seen == ["done", "inflate", "done"]
        assert np.array_equal(bc.finish(), want) and want.any()
        monkeypatch.setenv("VAFC_BAM_INDEX", "ignore")
        bc.count_file(a)
        assert bc.seek_info().name == "off"
    finally:
        bc.close()


def test_a_record_longer_than_its_spans_members(tmp_path, monkeypatch):
    """A single read of 200,000 bases, the last of its reference, whose chunk
    in the index ends one byte behind its start: the span holds the member it
    starts in, the piece ends cut, and the second reading brings the rest."""
    rng = np.random.default_rng(5)
    pos = 3_000_000
    recs = [F.record(0, pos - 500 + 7 * i, 0, [("M", 50)], "".join("ACGT"[j] for j in rng.integers(0, 4, 50)), name=b"f%d" % i)
            for i in range(60)]
    long_seq = "".join("ACGT"[j] for j in rng.integers(0, 4, 200_000))
    recs.append(F.record(0, pos, 0, [("M", 200_000)], long_seq, name=b"long"))
    recs += [F.record(1, 1000 + 9 * i, 0, [("M", 50)], "ACGT" * 12 + "AC", name=b"g%d" % i) for i in range(60)]
    raw = F.bam(S.SORTED_REFS, recs)
    d = S.decode(raw)
    k = 60
    assert d.recs[k].end - d.recs[k].pos == 200_000
    first, last = d.recs[k].voff >> 16, d.recs[k].end_voff >> 16
    assert len([m for m in d.members if first <= m.coff <= last]) >= 4
    short = d._replace(recs=d.recs[:k] + [d.recs[k]._replace(end_voff=d.recs[k].voff + 1)] + d.recs[k + 1:])
    path = str(tmp_path / "l.bam")
    with open(path, "wb") as f:
        f.write(raw)
    with open(path + ".bai", "wb") as f:
        f.write(S.write_bai(short))
    rows = [("chr1", p, long_seq[p - pos], "ACGT"[(p + 1) % 4]) for p in range(pos, pos + 200_000, 50)]
    regions = [(0, r[1], r[1] + 1) for r in rows]
    spans = S.py_plan(S.write_bai(short), 2, regions)
    assert any(e == d.recs[k].voff + 1 for _b, e in spans)
    bc = make_counter(rows, [r[0] for r in S.SORTED_REFS], tmp_path)
    try:
        full_st, _members, runs = full_then_seek(bc, path, monkeypatch)
        st, sk, (_host, device) = runs[0]
        assert (sk.name, sk.rereads) == ("done", 1) and sk.members == device
        assert st.seqs <= full_st.seqs and st.blocks == 2
        got = bc.finish()
        assert int(got[0::2].sum()) >= len(rows)                                # the long read matches its own bases
    finally:
        bc.close()

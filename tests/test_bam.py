"""bam-vaf-counter (include/vafc.h, "bam-vaf-counter"): a Python statement of
the contract with its own BGZF / BAM reader over zlib, checked against the
goldens of the real reference binary (tests/golden/bam, written by
tests/golden/make_golden_bam.py) without a GPU; the C++ host reader against
the Python one; and, on the GPU, the CLI against the goldens and the kernels
against the statement."""
import atexit
import hashlib
import json
import os
import re
import shutil
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

import bam_fixture as F
from bam_statement import (MATCH_OPS, QUERY_OPS, REF_OPS, SKIP, count_records, make_counter, pack, py_build_regions,
                           rec_end)
from conftest import GOLDEN, PKG

CLI = os.path.join(PKG, "lib", "bam-vaf-counter")
with open(os.path.join(GOLDEN, "bam", "manifest.json")) as _f:
    MANIFEST = json.load(_f)
# the directory the golden cases ran in: the committed files and what bam_fixture.derive makes of them
BAM_DIR = tempfile.mkdtemp(prefix="vafc_bam_")
atexit.register(shutil.rmtree, BAM_DIR, True)
F.derive(os.path.join(GOLDEN, "bam"), BAM_DIR)


# ---------------------------------------------------------------------------
# the statement: files and records here, counting in tests/bam_statement.py
# ---------------------------------------------------------------------------

class NotBam(Exception):
    pass


def bgzf_text(raw: bytes) -> bytes:
    """The text of the blocks in front of the first one that is truncated, is
    no BGZF member, does not inflate or fails its CRC-32 / ISIZE (item 7)."""
    out, at = [], 0
    while at < len(raw):
        if len(raw) - at < 12 or raw[at:at + 3] != b"\x1f\x8b\x08" or not raw[at + 3] & 4:
            break
        xlen = struct.unpack_from("<H", raw, at + 10)[0]
        extra, bsize, i = raw[at + 12:at + 12 + xlen], None, 0
        if len(extra) < xlen:
            break
        while i + 4 <= xlen:
            slen = struct.unpack_from("<H", extra, i + 2)[0]
            if extra[i:i + 2] == b"BC" and slen == 2 and i + 6 <= xlen:
                bsize = struct.unpack_from("<H", extra, i + 4)[0]
                break
            i += 4 + slen
        if bsize is None or bsize + 1 < 12 + xlen + 8 or at + bsize + 1 > len(raw):
            break
        blk = raw[at:at + bsize + 1]
        crc, isize = struct.unpack_from("<II", blk, len(blk) - 8)
        try:
            d = zlib.decompressobj(-15)
            text = d.decompress(blk[12 + xlen:-8])
            if not d.eof or d.unused_data:
                break
        except zlib.error:
            break
        if len(text) != isize or zlib.crc32(text) != crc or isize > 65536:
            break
        out.append(text)
        at += bsize + 1
    return b"".join(out)


def find_cg(aux: bytes):
    """The words of a CG:B,I tag, None without one, False on malformed aux."""
    at = 0
    while at < len(aux):
        if len(aux) - at < 3:
            return False
        tag, typ = aux[at:at + 2], aux[at + 2:at + 3]
        at += 3
        if typ in b"AcC":
            size = 1
        elif typ in b"sS":
            size = 2
        elif typ in b"iIf":
            size = 4
        elif typ == b"d":
            size = 8
        elif typ in b"ZH":
            nul = aux.find(b"\0", at)
            if nul < 0:
                return False
            size = nul - at + 1
        elif typ == b"B":
            if len(aux) - at < 5:
                return False
            el = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}.get(aux[at:at + 1])
            if el is None:
                return False
            cnt = struct.unpack_from("<I", aux, at + 1)[0]
            if cnt * el > len(aux) - at - 5:
                return False
            if tag == b"CG":
                return list(struct.unpack_from("<%dI" % cnt, aux, at + 5)) if aux[at:at + 1] in b"Ii" else None
            size = 5 + cnt * el
        else:
            return False
        if size > len(aux) - at:
            return False
        if tag == b"CG":
            return None
        at += size
    return None


def read_bam_py(path):
    """(reference names, [(tid, pos, flag, CIGAR words, l_seq, packed bases)])
    under items 7 and 8.  OSError: cannot be opened; NotBam: not BGZF BAM, or
    the header cannot be read."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:2] != b"\x1f\x8b":
        raise NotBam("format")
    t = bgzf_text(raw)
    try:
        if t[:4] != b"BAM\1":
            raise NotBam("header")
        l_text, = struct.unpack_from("<i", t, 4)
        at = 8 + l_text
        n_ref, = struct.unpack_from("<i", t, at)
        at += 4
        names = []
        for _ in range(n_ref):
            l_name, = struct.unpack_from("<i", t, at)
            if l_name < 1 or at + 4 + l_name + 4 > len(t):
                raise NotBam("header")
            names.append(t[at + 4:at + 4 + l_name].split(b"\0")[0].decode("latin-1"))
            at += 4 + l_name + 4
    except struct.error:
        raise NotBam("header")
    recs, in_batch, empty = [], 0, 0

    def failed():       # the reference's batch of 1,000 closes; the second empty one ends the file
        nonlocal in_batch, empty
        empty += in_batch == 0
        in_batch = 0
        return empty == 2

    while True:
        if len(t) - at < 4:
            break
        bl, = struct.unpack_from("<i", t, at)
        at += 4
        if bl < 32:
            if failed():
                break
            continue
        if len(t) - at < 32:
            break
        tid, pos, l_qname, _mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", t, at)
        at += 32
        if l_seq < 0 or l_qname < 1 or 4 * n_cigar + l_qname + (l_seq + 1) // 2 + l_seq > bl - 32:
            if failed():
                break
            continue
        if len(t) - at < bl - 32:
            break
        body = t[at:at + bl - 32]
        at += bl - 32
        words = list(struct.unpack_from("<%dI" % n_cigar, body, l_qname))
        s0 = l_qname + 4 * n_cigar
        seq = body[s0:s0 + (l_seq + 1) // 2]
        if n_cigar and words[0] == (l_seq << 4 | 4) & 0xFFFFFFFF and tid >= 0 and pos >= 0:
            cg = find_cg(body[s0 + (l_seq + 1) // 2 + l_seq:])
            if cg is False:
                if failed():
                    break
                continue
            if cg is not None and n_cigar <= len(cg) < 1 << 29:
                words = cg
        qlen = sum(w >> 4 for w in words if (w & 15) in QUERY_OPS)
        if words and l_seq > 0 and not flag & 4 and qlen != l_seq:
            if failed():
                break
            continue
        recs.append((tid, pos, flag, words, l_seq, seq))
        in_batch = (in_batch + 1) % 1000
    return names, recs


def index_usable(fn):
    """Item 6: the first existing candidate decides."""
    stem = None
    for i in range(len(fn) - 1, 0, -1):
        if fn[i] == ".":
            stem = fn[:i]
            break
    cand = [fn + ".csi"] + ([stem + ".csi"] if stem else []) + [fn + ".bai"] + ([stem + ".bai"] if stem else [])
    for c in cand:
        if os.path.exists(c):
            with open(c, "rb") as f:
                raw = f.read()
            return raw[:4] == b"BAI\1" or (raw[:2] == b"\x1f\x8b" and bgzf_text(raw)[:4] == b"CSI\1")
    return False


def load_rows(path):
    """patterns.txt -> [(chr, pos, ref, alt)], ref / alt one character each."""
    import vafc
    db = vafc.load_patterns(path)
    rows = []
    for i in range(db.n):
        r = db.record(i)
        rows.append((r[0], r[1], r[3].decode("latin-1"), r[4].decode("latin-1")))
    return db, rows


def statement_main(argv, cwd):
    """main (bam-vaf-counter.c:472-578): (exit code, counts or None, db)."""
    import vafc
    opts, files = vafc.ketopt_scan(list(argv), "p:o:t:")
    opt = {"p": None, "o": None}
    for c, a in opts:
        if c in opt:
            opt[c] = a
    if not opt["p"] or not opt["o"] or not files:
        return 1, None, None
    try:
        db, rows = load_rows(os.path.join(cwd, opt["p"]))
    except vafc.VafcError:
        return 1, None, None
    try:
        names, _ = read_bam_py(os.path.join(cwd, files[0]))
    except (OSError, NotBam):
        return 1, None, None
    row_tid = [names.index(r[0]) if r[0] in names else -1 for r in rows]
    if not rows:
        return 1, None, None
    regions = py_build_regions(rows)
    counts = np.zeros(2 * len(rows), np.uint32)
    for fn in files:
        path = os.path.join(cwd, fn)
        try:
            fnames, recs = read_bam_py(path)
        except (OSError, NotBam):
            continue
        regs = None
        if index_usable(path):
            regs = [(fnames.index(c), s, e) for c, s, e in regions if c in fnames]
        count_records(rows, row_tid, recs, regs, counts)
    return 0, counts, db


# ---------------------------------------------------------------------------
# CPU: the statement against the goldens, the C++ reader against the statement
# ---------------------------------------------------------------------------

def golden_vaf(name):
    """The .vaf the reference wrote for a case, as the manifest keeps it: md5
    of its bytes, first line, "ref alt" counts of its rows; None without one."""
    e = MANIFEST[name].get("vaf")
    return golden_vaf(e[1:]) if isinstance(e, str) else e


def assert_vaf_equals(path, want):
    """Byte for byte through the md5; the counts first, to show what differs."""
    with open(path, "rb") as f:
        got = f.read()
    lines = got.decode().splitlines()
    counts = " ".join("%s %s" % tuple(ln.split("\t")[5:7]) for ln in lines[2:]).split()
    diff = [(i // 2, g, w) for i, (g, w) in enumerate(zip(counts, want["counts"].split())) if g != w]
    assert not diff and lines[0] == want["depth"], (diff[:8], lines[0], want["depth"])
    assert hashlib.md5(got).hexdigest() == want["md5"]


GOLDEN_BAMS = sorted(fn for fn in os.listdir(BAM_DIR) if fn.endswith(".bam"))
assert len(GOLDEN_BAMS) == 18


def test_manifest_covers_the_cases():
    need = {"noidx", "idx_bam_bai", "idx_bai", "idx_wrong_magic", "two_headers_noidx", "two_headers_idx",
            "missing_second", "missing_first", "opts_after_files", "empty_patterns", "long_noidx", "long_idx",
            "damage_noeof", "damage_midblock", "damage_border", "damage_flip", "damage_mismatch", "damage_bs8"}
    assert need <= set(MANIFEST)
    assert golden_vaf("noidx") != golden_vaf("idx_bam_bai")          # the indexed multiplicity is real
    assert golden_vaf("idx_wrong_magic") == golden_vaf("noidx")
    assert golden_vaf("damage_noeof") == golden_vaf("small")
    assert golden_vaf("damage_mismatch") == golden_vaf("small")      # dropped, and reading goes on
    assert len({golden_vaf("damage_" + d)["md5"] for d in ("midblock", "border", "flip", "bs8", "noeof",
                                                           "mismatch_thrice")}) >= 5
    assert golden_vaf("damage_mismatch_twice") == golden_vaf("small")    # one empty batch: reading goes on
    assert golden_vaf("damage_mismatch_batch") != golden_vaf("damage_mismatch_thrice") != golden_vaf("small")


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_statement_equals_reference(name, tmp_path):
    entry = MANIFEST[name]
    rc, counts, db = statement_main(entry["argv"], BAM_DIR)
    want = golden_vaf(name)
    if want is None:
        if name == "bad_outdir":          # everything is counted, then the output cannot be created
            assert rc == 0 and entry["rc"] == 1
        else:
            assert rc == entry["rc"] == 1
        return
    assert rc == entry["rc"] == 0
    out = str(tmp_path / "out.vaf")
    db.write_vaf(counts, out)
    assert_vaf_equals(out, want)


def test_goldens_reach_the_edges():
    """What the golden panel is meant to reach in a.bam, by the statement:
    bases right after I and S, rows inside D and N, at the first and the last
    base of a match block and at end - 1, and a 5,000-op record."""
    _db, rows = load_rows(os.path.join(BAM_DIR, "p.txt"))
    names, recs = read_bam_py(os.path.join(BAM_DIR, "a.bam"))
    row_tid = [names.index(r[0]) if r[0] in names else -1 for r in rows]
    tally = {}
    count_records(rows, row_tid, recs, None, None, tally)
    for key in ("hit1", "hit4", "gap2", "gap3", "hitNone", "base0", "base7", "base8"):
        assert tally.get(key, 0) > 0, (key, tally)
    pos_of = {(t, r[1]) for t, r in zip(row_tid, rows)}
    edges = {"first": 0, "last": 0, "end-1": 0}
    for rec in recs:
        if rec[2] & SKIP or rec[0] < 0:
            continue
        cur = rec[1]
        for w in rec[3]:
            op, n = w & 15, w >> 4
            if op in MATCH_OPS and n:
                edges["first"] += (rec[0], cur) in pos_of
                edges["last"] += (rec[0], cur + n - 1) in pos_of
            if op in REF_OPS:
                cur += n
        edges["end-1"] += (rec[0], rec_end(rec) - 1) in pos_of
    assert min(edges.values()) > 0, edges
    assert any(len(r[3]) == 0 and r[4] > 0 for r in recs) and any(len(r[3]) == 0 and r[4] == 0 for r in recs)
    assert any(r[4] % 2 == 1 for r in recs)
    assert {w & 15 for r in recs for w in r[3]} >= {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 13}
    assert max(len(r[3]) for r in read_bam_py(os.path.join(BAM_DIR, "long.bam"))[1]) == 5000
    assert len(read_bam_py(os.path.join(BAM_DIR, "cg.bam"))[1][0][3]) == 6      # the real CIGAR moved in


def test_build_regions_equals_statement():
    import vafc
    db, rows = load_rows(os.path.join(BAM_DIR, "p.txt"))
    want = py_build_regions(rows)
    assert vafc.build_regions(db) == want
    assert len(want) < len(rows) and any(e - s > 1 for _c, s, e in want)
    empty, _ = load_rows(os.path.join(BAM_DIR, "p_empty.txt"))
    assert vafc.build_regions(empty) == []


def test_index_rule():
    import vafc
    for fn, want in (("a.bam", False), ("a_i.bam", True), ("a_j.bam", True), ("a_k.bam", False), ("b.bam", True)):
        path = os.path.join(BAM_DIR, fn)
        assert index_usable(path) == want
        assert vafc.bam_index_usable(path)[0] == want
    assert vafc.bam_index_usable(os.path.join(BAM_DIR, "a_j.bam"))[1].endswith("a_j.bai")


def assert_reader_equal(path, n_thread):
    import vafc
    names, want = read_bam_py(path)
    got_names, recs, data = vafc.read_bam(path, n_thread)
    assert got_names == names
    assert len(recs) == len(want)
    for r, w in zip(recs, want):
        assert (int(r["tid"]), int(r["pos"]), int(r["flag"]), int(r["n_cigar"]), int(r["l_seq"])) == \
            (w[0], w[1], w[2], len(w[3]), w[4])
        off = int(r["off"])
        assert off % 4 == 0 and r["reserved"] == 0
        assert data[off:off + 4 * len(w[3])].tobytes() == struct.pack("<%dI" % len(w[3]), *w[3])
        assert data[off + 4 * len(w[3]):off + 4 * len(w[3]) + len(w[5])].tobytes() == w[5]


@pytest.mark.parametrize("fn", GOLDEN_BAMS)
def test_cpp_reader_equals_python_reader(fn):
    assert_reader_equal(os.path.join(BAM_DIR, fn), 1 if fn < "b" else 4)


def test_cpp_reader_across_every_block_border(tmp_path):
    """Records longer than the 1 KB blocks: every border cuts a record, and
    the header is cut as well; 300 blocks make two inflate groups."""
    import vafc
    rng = np.random.default_rng(5)
    refs = [("chr%d" % i, 100000) for i in range(1, 60)]
    recs = []
    for i in range(220):
        cigar = F.random_cigar(rng, 40 + i % 7, 60, "MMMM=XIDN")
        seq = "".join("ACGTN"[j] for j in rng.integers(0, 5, F.query_len(cigar)))
        recs.append(F.record(i % 3, 10 * i, 0, cigar, seq, name=b"read%d" % i))
    assert min(len(r) for r in recs) > 1024
    raw = F.bam(refs, recs, block=1024)
    assert len(F.bgzf_blocks(raw)) > 256
    path = str(tmp_path / "straddle.bam")
    with open(path, "wb") as f:
        f.write(raw)
    for t in (1, 3, 16):
        assert_reader_equal(path, t)
    assert vafc.bam_header_names(path) == [r[0] for r in refs]


def test_probe_and_formats(tmp_path):
    import gzip
    import vafc
    kinds = {"x.sam": b"@HD\tVN:1.6\n", "x.cram": b"CRAM\x03\x00", "x.ubam": b"BAM\1\0\0\0\0\0\0\0\0",
             "x.gz": gzip.compress(b"BAM\1"), "x.bgzf": F.bgzf(b"not a BAM file")}
    want = {"x.sam": "SAM", "x.cram": "CRAM", "x.ubam": "RAW", "x.gz": "GZIP", "x.bgzf": "BGZF_OTHER"}
    for fn, raw in kinds.items():
        p = str(tmp_path / fn)
        with open(p, "wb") as f:
            f.write(raw)
        assert vafc.bam_probe(p) == want[fn]
        with pytest.raises(vafc.VafcError) as ei:
            vafc.read_bam(p)
        assert ei.value.code == vafc.VC_EINVAL
    assert vafc.bam_probe(os.path.join(BAM_DIR, "a.bam")) == "BGZF"
    with pytest.raises(FileNotFoundError):
        vafc.read_bam(str(tmp_path / "nope.bam"))
    # a header that ends early: BGZF BAM by its first bytes, but unreadable
    p = str(tmp_path / "cut.bam")
    with open(p, "wb") as f:
        f.write(F.bgzf(F.header([("chr1", 100)])[:20]))
    assert vafc.bam_probe(p) == "BGZF"
    with pytest.raises(vafc.VafcError):
        vafc.read_bam(p)


# ---------------------------------------------------------------------------
# fuzz material (made once; the CPU test checks that it is not vacuous)
# ---------------------------------------------------------------------------

FUZZ_SEED = 11
_fuzz = {}


def fuzz_set():
    """2,000 random records x 200 rows on two references, the rows dense
    enough to be hit, the statement's counts with and without weights."""
    if _fuzz:
        return _fuzz
    rng = np.random.default_rng(FUZZ_SEED)
    rows, seen = [], set()
    while len(rows) < 200:
        chr_ = ("chr1", "chr2", "chrX")[int(rng.integers(0, 10)) // 5 if len(rows) % 50 else 2]
        pos = int(rng.integers(0, 400))
        if (chr_, pos) in seen and len(rows) % 9:
            continue
        seen.add((chr_, pos))
        ref = "ACGTNacgR="[int(rng.integers(0, 10))]
        alt = ref if len(rows) % 23 == 0 else "ACGTN"[int(rng.integers(0, 5))]
        rows.append((chr_, pos, ref, alt))
    names = ["chr1", "chr2"]
    recs = []
    for i in range(2000):
        n_ops = (0, 1, 2, 3, 5, 8, 13, 70, 130)[int(rng.integers(0, 9))] if i % 10 else 66
        cigar = F.random_cigar(rng, n_ops, 6 if n_ops < 60 else 3) if n_ops else []
        if i % 37 == 0 and cigar:
            cigar.insert(len(cigar) // 2, (int(rng.integers(9, 16)), 3))
        l_seq = F.query_len(cigar) if cigar else int(rng.integers(0, 20))
        nib = rng.integers(0, 16, l_seq + 1)
        if i % 3:
            nib = np.where(rng.random(l_seq + 1) < 0.9, np.array([1, 2, 4, 8])[rng.integers(0, 4, l_seq + 1)], nib)
        seq = bytes(int(nib[j]) << 4 | int(nib[j + 1]) if j + 1 < l_seq else int(nib[j]) << 4 for j in range(0, l_seq, 2))
        flag = (0, 16, 0x100, 0x800, 0, 0, 0x4, 0x200, 0x400, 1)[int(rng.integers(0, 10))]
        tid = int(rng.integers(-1, 2)) if i % 11 == 0 else int(rng.integers(0, 2))
        recs.append((tid, int(rng.integers(-5, 420)), flag, F.cigar_words(cigar), l_seq, seq))
    row_tid = [names.index(r[0]) if r[0] in names else -1 for r in rows]
    regions = [(names.index(c), s, e) for c, s, e in py_build_regions(rows) if c in names]
    tally = {}
    _fuzz.update(rows=rows, names=names, recs=recs, row_tid=row_tid, regions=regions, tally=tally,
                 plain=count_records(rows, row_tid, recs, None, None, tally),
                 weighted=count_records(rows, row_tid, recs, regions))
    return _fuzz


def test_fuzz_set_is_not_vacuous():
    z = fuzz_set()
    assert int(z["plain"].astype(np.uint64).sum()) >= 300
    assert not np.array_equal(z["plain"], z["weighted"])
    t = z["tally"]
    assert t.get("hit1", 0) >= 1 and t.get("hit4", 0) >= 1        # a count right after an I, after an S
    assert t.get("gap2", 0) >= 1 and t.get("gap3", 0) >= 1        # a row inside a D, inside an N
    assert sum(1 for r in z["recs"] if len(r[3]) > 64) > 100 and sum(1 for r in z["recs"] if 0 < len(r[3]) <= 64) > 100


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def own_lines(stderr: str) -> str:
    return "".join(ln + "\n" for ln in stderr.splitlines() if not re.match(r"\[[EWIDT]::", ln))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_cli_equals_reference(name, tmp_path):
    entry = MANIFEST[name]
    for fn in os.listdir(BAM_DIR):
        os.symlink(os.path.join(BAM_DIR, fn), str(tmp_path / fn))
    os.mkdir(str(tmp_path / "o"))
    p = subprocess.run([CLI] + entry["argv"], cwd=str(tmp_path), capture_output=True, timeout=120)
    assert p.returncode == entry["rc"], p.stderr.decode()
    assert own_lines(p.stderr.decode()) == entry["stderr"]
    out = str(tmp_path / "o" / "out.vaf")
    want = golden_vaf(name)
    if want is None:
        assert not os.path.exists(out)
    else:
        assert_vaf_equals(out, want)


@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0, 64, 0xFFFFFFFF], ids=["all_long", "64", "never_long"])
def test_fuzz_against_statement(threshold, tmp_path):
    z = fuzz_set()
    bc = make_counter(z["rows"], z["names"], tmp_path)
    try:
        bc.set_long_threshold(threshold)
        recs, data = pack(z["recs"])
        bc.count_block(recs, data)
        got = bc.finish()
        assert np.array_equal(got, z["plain"]), np.nonzero(got != z["plain"])[0][:8]
        bc.reset()
        t, s, e = zip(*z["regions"])
        bc.set_regions(t, s, e)
        bc.count_block(recs, data)
        got = bc.finish()
        assert np.array_equal(got, z["weighted"]), np.nonzero(got != z["weighted"])[0][:8]
        assert bc.kernel_ms() > 0
    finally:
        bc.close()


@pytest.mark.gpu
def test_wave_path_edges(tmp_path):
    """One record each of 63, 64, 65, 127, 128, 129 and 4,097 ops, with rows at
    the first and last base of the first and the last op of every 64-op group
    (the two ops either side of each group border)."""
    rng = np.random.default_rng(3)
    recs, rows = [], []
    for k, n_ops in enumerate((63, 64, 65, 127, 128, 129, 4097)):
        cigar = F.random_cigar(rng, n_ops, 3, "MM=XIDN")
        marks = sorted({i for g in range(0, n_ops, 64) for i in (g - 1, g, g + 1, g + 62, g + 63) if 0 <= i < n_ops}
                       | {n_ops - 1})
        if n_ops > 4000:
            marks = [i for i in marks if i < 200 or i > n_ops - 200 or i % 1024 < 2 or i % 1024 > 1021]
        for i in marks:
            cigar[i] = ("M=X"[i % 3], 3)
        pos, cur = 1000 * k + 7, 1000 * k + 7
        for i, w in enumerate(F.cigar_words(cigar)):
            op, n = w & 15, w >> 4
            if i in marks:
                rows += [("chr1", cur, "A", "C"), ("chr1", cur + n - 1, "G", "T")]
            if op in REF_OPS:
                cur += n
        l_seq = F.query_len(cigar)
        nib = np.array([1, 2, 4, 8])[rng.integers(0, 4, l_seq + 1)]
        seq = bytes(int(nib[j]) << 4 | (int(nib[j + 1]) if j + 1 < l_seq else 0) for j in range(0, l_seq, 2))
        recs.append((0, pos, 0, F.cigar_words(cigar), l_seq, seq))
    # rows inside the gaps and the other ops as well
    rows += [("chr1", p, "ACGT"[p % 4], "ACGT"[(p + 1) % 4]) for p in range(0, 16000, 13)]
    row_tid = [0] * len(rows)
    regions = [(0, s, e) for _c, s, e in py_build_regions(rows)]
    plain = count_records(rows, row_tid, recs)
    weighted = count_records(rows, row_tid, recs, regions)
    assert int(plain.sum()) > 150 and int(weighted.sum()) > int(plain.sum())
    bc = make_counter(rows, ["chr1"], tmp_path)
    try:
        packed = pack(recs)
        for thr in (64, 0, 0xFFFFFFFF, 100):
            bc.set_long_threshold(thr)
            bc.set_regions()
            bc.reset()
            bc.count_block(*packed)
            assert np.array_equal(bc.finish(), plain), thr
            t, s, e = zip(*regions)
            bc.set_regions(t, s, e)
            bc.reset()
            bc.count_block(*packed)
            assert np.array_equal(bc.finish(), weighted), thr
    finally:
        bc.close()


@pytest.mark.gpu
def test_skipped_only_and_empty_batches(tmp_path):
    import vafc
    rows = [("chr1", 10, "A", "C"), ("chr1", 11, "C", "A")]
    seq = bytes([0x12, 0x12])
    recs = [(0, 9, f, F.cigar_words([("M", 4)]), 4, seq) for f in (0x4, 0x200, 0x400, 0x604, 0x4 | 16)] + \
        [(-1, 9, 0, F.cigar_words([("M", 4)]), 4, seq)]
    bc = make_counter(rows, ["chr1"], tmp_path)
    try:
        for thr in (64, 0):
            bc.set_long_threshold(thr)
            bc.count_block(*pack(recs))
            bc.count_block(np.zeros(0, vafc.BAM_REC), np.zeros(0, np.uint8))
            assert not bc.finish().any()
        bc.count_block(*pack([(0, 9, 0x100, F.cigar_words([("M", 4)]), 4, seq)]))
        assert bc.finish().tolist() == [0, 1, 0, 1]      # bases C at 10 (alt), A at 11 (alt)
    finally:
        bc.close()


@pytest.mark.gpu
def test_accumulation_reset_wrap_and_bad_descriptor(tmp_path):
    import vafc
    z = fuzz_set()
    bc = make_counter(z["rows"], z["names"], tmp_path)
    try:
        a, b = z["recs"][:900], z["recs"][900:]
        bc.count_block(*pack(a))
        bc.count_block(*pack(b))
        assert np.array_equal(bc.finish(), z["plain"])
        bc.reset()
        assert not bc.finish().any()
        # the wrap at 2^32 with a weight of 3: one record over three regions
        rows = z["rows"]
        i = next(i for i, r in enumerate(rows) if r[0] == "chr1" and r[2] == "A" and r[3] != "A")
        p = rows[i][1]
        rec = (0, p - 4, 0, F.cigar_words([("M", 9)]), 9, bytes([0x11] * 5))
        bc.set_regions([0, 0, 0, 0], [p - 4, p, p + 3, p + 40], [p - 3, p + 1, p + 5, p + 41])
        start = np.zeros(2 * len(rows), np.uint32)
        start[2 * i] = 0xFFFFFFFE
        bc.set_counts(start)
        bc.count_block(*pack([rec]))
        got = bc.finish()
        want = count_records(rows, z["row_tid"], [rec], [(0, p - 4, p - 3), (0, p, p + 1), (0, p + 3, p + 5)],
                             start.copy())
        assert int(got[2 * i]) == 1 and np.array_equal(got, want)
        # a descriptor that points past the buffer is reported at finish, not followed
        bc.set_regions()
        for bad_off, thr in ((1 << 40, 64), (1 << 40, 0), (2, 64)):
            bc.reset()
            bc.set_long_threshold(thr)
            recs, data = pack(z["recs"][:50] + [rec])
            recs[-1]["off"] = bad_off
            bc.count_block(recs, data)
            with pytest.raises(vafc.VafcError) as ei:
                bc.finish()
            assert ei.value.code == vafc.VC_EINVAL
        recs, data = pack([rec])
        recs[0]["l_seq"] = 4000                       # bases that would reach past the data
        bc.reset()
        bc.count_block(recs, data)
        with pytest.raises(vafc.VafcError):
            bc.finish()
        bc.reset()
        bc.count_block(*pack(z["recs"]))
        assert np.array_equal(bc.finish(), z["plain"])
    finally:
        bc.close()


@pytest.mark.gpu
def test_count_device_side_stream_after_reset(tmp_path):
    """vc_bam_count_device on a torch side stream right after a vc_bam_reset on
    the handle's own stream, which is still busy with an earlier batch, and no
    host synchronisation in between: the reset comes first, and vc_bam_finish
    sees the launch."""
    import torch
    import vafc
    z = fuzz_set()
    recs, data = pack(z["recs"])
    dev = torch.device("cuda", 0)
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
    d_data = torch.from_numpy(data.copy()).to(dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    bc = make_counter(z["rows"], z["names"], tmp_path)
    try:
        for _ in range(3):
            bc.count_block(recs, data)
        bc.reset()
        bc.count_device(d_recs.data_ptr(), recs.size, d_data.data_ptr(), data.size, side.cuda_stream)
        assert np.array_equal(bc.finish(), z["plain"])
        bc.reset()
        bc.count_device(d_recs.data_ptr(), recs.size, d_data.data_ptr(), data.size, vafc.STREAM_CTX)
        bc.count_device(d_recs.data_ptr(), recs.size, d_data.data_ptr(), data.size)
        assert np.array_equal(bc.finish(), z["plain"] * np.uint32(2))
    finally:
        bc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_thread", [1, 3, 16])
def test_count_file_equals_count_block(n_thread, tmp_path, monkeypatch):
    import vafc
    monkeypatch.setenv("VAFC_BATCH_BYTES", "4096")        # several batches per file
    db, rows = load_rows(os.path.join(BAM_DIR, "p.txt"))
    first = vafc.bam_header_names(os.path.join(BAM_DIR, "a.bam"))
    row_tid = [first.index(r[0]) if r[0] in first else -1 for r in rows]
    regions = py_build_regions(rows)
    bc = vafc.create_snp_map(db, os.path.join(BAM_DIR, "a.bam"))
    ref = vafc.BamCounter(db, first)
    try:
        for fn in ("a.bam", "a_i.bam", "b.bam", "long_i.bam", "d_flip.bam"):
            path = os.path.join(BAM_DIR, fn)
            st = vafc.count_bam_variants(path, n_thread, bc)
            names, recs = read_bam_py(path)
            assert st.seqs == len(recs) and st.bases == sum(r[4] for r in recs)
            assert st.blocks > 1 or fn == "d_flip.bam"    # less than one batch of data
            regs = [(names.index(c), s, e) for c, s, e in regions if c in names] if index_usable(path) else []
            ref.set_regions(*(zip(*regs) if regs else ((), (), ())))
            ref.count_block(*pack(recs))
        with pytest.raises(FileNotFoundError):
            bc.count_file(os.path.join(BAM_DIR, "nope.bam"))
        got, want = bc.finish(), ref.finish()
        assert np.array_equal(got, want) and int(want.sum()) > 3000
    finally:
        bc.close()
        ref.close()
    assert sum(1 for t in row_tid if t < 0) == 2        # chrUn, chrUn2: warned about, never counted

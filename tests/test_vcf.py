"""vcf-vaf-counter (include/vafc.h, "vcf-vaf-counter"): a Python statement of
the contract (tests/vcf_fixture.py) checked against the goldens of the real
reference binary (tests/golden/vcf, written by tests/golden/make_golden_vcf.py)
without a GPU; the C++ header and line rules against the statement on every
golden line and on a seeded fuzz; the stand-alone sanitizer run; and, on the
GPU, the CLI against the goldens and the kernel against the statement, hit
list for hit list."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vcf_fixture as F
from conftest import GOLDEN, PKG, ROOT

CLI = os.path.join(PKG, "lib", "vcf-vaf-counter")
VCF_DIR = os.path.join(GOLDEN, "vcf")
with open(os.path.join(VCF_DIR, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
ROWS = F.load_patterns(F.panel_text().encode())
ROW = {r[2].decode(): i for i, r in enumerate(ROWS)}


def golden(name):
    p = os.path.join(VCF_DIR, name)
    if not os.path.isfile(p):
        return None
    with open(p, "rb") as f:
        return f.read()


def golden_vaf(name):
    e = MANIFEST[name].get("vaf")
    return MANIFEST[e[1:]]["vaf"] if isinstance(e, str) else e


def pairs(name):
    c = golden_vaf(name)["counts"].split()
    return [(int(c[i]), int(c[i + 1])) for i in range(0, len(c), 2)]


def own_lines(stderr: str) -> str:
    return "".join(ln + "\n" for ln in stderr.splitlines() if not re.match(r"\[[EWIDT]::", ln))


# ---------------------------------------------------------------------------
# CPU: the statement is the reference's behaviour
# ---------------------------------------------------------------------------

def test_manifest_covers_the_cases_and_inputs():
    assert set(MANIFEST) == set(F.cases())
    for name, argv in F.cases().items():
        assert MANIFEST[name]["argv"] == argv
    for name, data in F.inputs().items():
        assert golden(name) == data, name


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_statement_equals_reference(name):
    e = MANIFEST[name]
    rc, err, vaf = F.run_statement(e["argv"], golden, lambda fn: not fn.startswith("nodir/"))
    assert rc == e["rc"]
    assert err == e["stderr"]
    assert (F.vaf_entry(vaf) if vaf is not None else None) == golden_vaf(name)


def test_goldens_reach_the_edges():
    """What the issue observed, read off the reference's own output."""
    m0, m1 = pairs("main_s0"), pairs("main_s1")
    assert m0[ROW["rsA"]] == (10, 5) and m0[ROW["rsAdup"]] == (0, 0)          # the first row only
    assert m0[ROW["rsI"]] == (1, 2) and m0[ROW["rsJ"]] == (5, 6)               # chr10, chr1_x beside chr1
    assert m0[ROW["rsG"]] == (1, 1)                                            # a CHROM the header lacks
    assert m0[ROW["rsK"]] == (9, 1)                                            # POS 0: start -1
    assert m0[ROW["rsB"]] == (8, 0) and m1[ROW["rsB"]] == (4, 5)               # leading zeros; DP by genotype
    assert m0[ROW["rsD"]] == (21, 22)                                          # POS 2^32 + 300
    assert m0[ROW["rsE"]] == m0[ROW["rsF"]] == m0[ROW["rsH"]] == (0, 0)        # lower case, ALT ".", "C,G"
    assert m0[ROW["rsL"]] == (6, 1) and m1[ROW["rsL"]] == (60, 10)             # the last qualifying record
    assert m0[ROW["rsM"]] == m0[ROW["rsMdup"]] == (0, 0)                       # no fall-through
    assert m0[ROW["rsN"]] == (11, 12)                                          # POS +900
    assert all(p == (0, 0) for p in pairs("main_s_past"))
    assert golden_vaf("main_gz") == golden_vaf("crlf") == golden_vaf("main_s0")
    assert golden_vaf("main_bgzf") == golden_vaf("opts_after_file") == golden_vaf("main_s1")
    g0, g1 = pairs("gt_s0"), pairs("gt_s1")
    assert g0[ROW["rsA"]] == (2, 3) and g1[ROW["rsA"]] == (0, 0)               # haploid: 2s + 1 >= ngt for sample 1
    assert g0[ROW["rsB"]] == (6, 6) and g1[ROW["rsB"]] == (7, 7)               # triploid: sample 1 reads 1, 0
    assert g0[ROW["rsD"]] == g1[ROW["rsD"]] == (0, 0)                          # .|1 and 0/.
    assert g0[ROW["rsL"]] == (7, 8) and g1[ROW["rsL"]] == (9, 10)              # | as /
    assert g0[ROW["rsN"]] == (1, 2) and g1[ROW["rsN"]] == (0, 0)               # a padding entry
    a0, a1 = pairs("ad_s0"), pairs("ad_s1")
    assert a0[ROW["rsA"]] == (1, 2) and a1[ROW["rsA"]] == (3, 4)               # flat entries 2s, 2s + 1
    assert a0[ROW["rsB"]] == (5, 7) and a1[ROW["rsB"]] == (6, 7)               # one value each; sample 1 falls to DP
    assert a0[ROW["rsD"]] == (7, 8) and a1[ROW["rsD"]] == (0, 13)              # "." is missing: DP
    assert a0[ROW["rsL"]] == (0, 0)                                            # 5 and the vector end: depth < 1
    assert a0[ROW["rsN"]] == (7, 8) and a1[ROW["rsN"]] == (9, 0)               # AD 0,0: DP is tried
    assert pairs("noad_s0")[0] == (7, 8) and pairs("noad_s1")[0] == (0, 7)     # AD undeclared: DP
    d0, d1 = pairs("dp_s0"), pairs("dp_s1")
    assert d0[ROW["rsA"]] == (7, 8) and d1[ROW["rsA"]] == (4, 5) and d0[ROW["rsB"]] == (0, 13) and d1[ROW["rsB"]] == (21, 0)
    assert all(p == (0, 0) for p in pairs("dp_str"))
    assert pairs("depth_d7")[0] == (0, 0) and pairs("depth_d7_s1")[0] == (4, 4)
    assert pairs("depth_d1")[ROW["rsB"]] == (3, 4) and pairs("depth_d0")[ROW["rsB"]] == (0, 0)   # depth 0 overwrites
    for name in MANIFEST:
        if name.startswith("end_") or name == "gt_int":
            assert pairs(name)[ROW["rsO"]] == (0, 0), name       # the hit behind the stopping line
    for name in ("end_pos", "end_empty", "end_hash", "end_ncols", "end_char"):
        assert pairs(name)[ROW["rsA"]] == (3, 4), name           # what came before is kept
    assert pairs("nosample")[ROW["rsO"]] == (30, 40)            # a FORMAT without samples stops nothing
    o0, o1 = pairs("goes_on"), pairs("goes_on_s1")              # 255 tags, an empty CHROM, empty tags, a last GT left empty
    assert o0[ROW["rsO"]] == (30, 40) and o1[ROW["rsO"]] == (50, 60)
    assert o0[ROW["rsB"]] == (2, 3) and o1[ROW["rsB"]] == (3, 4)  # GT::DP: the empty tag is a String tag like any other
    assert o0[ROW["rsD"]] == (8, 9) and o1[ROW["rsD"]] == (10, 11) and o0[ROW["rsL"]] == (2, 3) and o1[ROW["rsL"]] == (0, 0)
    for name in ("abort_gt", "abort_gt_s_past"):              # GT in no sample column of a hit line: exit(1) inside htslib
        assert MANIFEST[name]["rc"] == 1 and "vaf" not in MANIFEST[name] and MANIFEST[name]["stderr"].endswith("Processing VCF file...\n")
    assert pairs("abort_gt_nohit")[ROW["rsO"]] == (30, 40)      # the same columns on a line that passes items 2, 3 for no row
    assert pairs("more_cols")[0] == (5, 6)
    for name in ("junk", "nochrom", "missing_input", "sites"):
        assert MANIFEST[name]["rc"] == 0 and all(p == (0, 0) for p in pairs(name))
    assert "failed to read VCF header" in MANIFEST["junk"]["stderr"]
    assert "failed to open VCF file: nope.vcf" in MANIFEST["missing_input"]["stderr"]
    assert MANIFEST["missing_patterns"]["rc"] == MANIFEST["bad_outdir"]["rc"] == MANIFEST["usage_no_v"]["rc"] == 1
    assert "[3]" in MANIFEST["usage_no_v"]["stderr"] and "[9]" in MANIFEST["usage_no_v"]["stderr"]


# ---------------------------------------------------------------------------
# CPU: the library's header and line rules against the statement
# ---------------------------------------------------------------------------

def same_verdict(v, ev, what):
    assert bool(v.head_ok) == ev["head_ok"], what
    if not ev["head_ok"]:
        assert v.verdict == F.END, what
        return
    assert (v.pos, v.chrom_len, v.n_allele, v.ref_len, v.alt_len) == (
        ev["pos"], len(ev["chrom"]), ev["n_allele"], len(ev["ref"]), len(ev["alt"])), what
    assert v.ref == (ev["ref"][:1] or b"\0")[0] and v.alt == (ev["alt"][:1] or b"\0")[0], what
    want = ev["verdict"]
    if isinstance(want, tuple):
        assert (v.verdict, v.ref_count, v.alt_count) == want, what
    else:
        assert v.verdict == want, what


def check_text(text: bytes, what: str, samples=(-1, 0, 1, 2), depths=(0, 1, 7)):
    import vafc
    hdr = F.parse_header(text)
    if hdr is None:
        with pytest.raises(vafc.VafcError):
            vafc.VcfHeader(text)
        return 0
    h = vafc.VcfHeader(text)
    assert (h.n_samples, h.body) == (hdr[0], hdr[2]), what
    for tag in (b"GT", b"AD", b"DP", b"XX"):
        assert h.type_of(tag.decode()) == hdr[1].get(tag, -1), what
    n = 0
    for off, line in F.body_lines(text, hdr[2]):
        for s in samples:
            for d in depths:
                same_verdict(h.eval_line(line, s, d), F.eval_line(hdr, line, s, d), "%s @%d s=%d d=%d" % (what, off, s, d))
        n += 1
    h.close()
    return n


def test_library_equals_statement_on_every_golden_line():
    n = 0
    for name in sorted(os.listdir(VCF_DIR)):
        if name.endswith((".vcf", ".vcf.gz")):
            n += check_text(F.text_of(golden(name)), name)
    assert n > 100


def test_tile_constant_is_the_headers():
    import vafc
    with open(os.path.join(ROOT, "include", "vafc.h")) as f:
        m = re.search(r"^#define VC_VCF_TILE_BYTES (\d+)$", f.read(), re.M)
    assert m and int(m.group(1)) == vafc.VCF_TILE_BYTES
    assert (vafc.VCF_SKIP, vafc.VCF_SET, vafc.VCF_END, vafc.VCF_ABORT) == (F.SKIP, F.SET, F.END, F.ABORT)


def test_header_needs_its_last_line():
    import vafc
    text = golden("main.vcf")
    body = F.parse_header(text)[2]
    for cut in (0, 5, 16, 40, body - 1):
        with pytest.raises(EOFError):
            vafc.VcfHeader(text[:cut], final=False)
    assert vafc.VcfHeader(text[:body], final=False).body == body
    assert vafc.VcfHeader(text[:body - 1]).body == body - 1      # final: the #CHROM line needs no newline
    with pytest.raises(vafc.VafcError):
        vafc.VcfHeader(text[:body - 30].rsplit(b"\n", 1)[0] + b"\n")   # the file ends before a #CHROM line


def fuzz_lines(rng, n):
    """Lines from inside the contract: well-formed first eight columns, then
    FORMAT and sample columns built from pieces that htslib accepts or rejects
    in the ways item 8 names."""
    gts = ["0/1", "1/1", "0/0", "0|1", "1|0", ".", "./.", ".|1", "0/.", "1", "0", "0/1/1", "2/1", "10/1", "0/x", "", "+1/1", "0/1x"]
    ints = ["3,4", "5", "17", "0,0", ".", "0", "1,2,3", ".,.", "7,.", ".,2", "-3", "+4", "12x", "", "4,", "x", "2147483647", "1,-2147483647"]
    strs = ["abc", "", ".", "a,b", "q/r"]
    tagsets = [["GT", "AD", "DP"], ["GT", "DP"], ["GT", "AD"], ["GT"], ["AD", "DP"], ["DP", "GT"], ["GT", "XX", "DP"],
               ["GT", "AD", "AD"], ["GT", "GT"], ["GT", "FL"], ["GT", "RR", "DP"], ["."], ["GT", ""], ["GT", "DP", "AD", "XX"]]
    out = []
    for _ in range(n):
        tags = tagsets[int(rng.integers(0, 4 if rng.random() < 0.6 else len(tagsets)))]
        ncol = int(rng.choice([2, 2, 2, 2, 2, 2, 1, 3, 0]))
        cols = []
        for _c in range(ncol):
            fields = []
            for t in tags:
                pool = gts if t == "GT" else strs if t == "XX" else ["1.5", ".", "2", "1e3,2", "z"] if t == "RR" else ints
                if rng.random() < 0.8:
                    pool = pool[:5]                                    # mostly plain values
                fields.append(pool[int(rng.integers(0, len(pool)))])
            keep = len(fields) - int(rng.choice([0, 0, 0, 1, 2]))      # trailing fields may be left out
            if rng.random() < 0.03:
                fields.append("9")                                     # one field too many
                keep = len(fields)
            cols.append(":".join(fields[:max(keep, 1)]))
        line = F.rec("chr1", int(rng.integers(0, 3000)), "A", "C", ":".join(tags), *cols)
        if rng.random() < 0.05:
            line = line[:-1] + "\t\n"
        if rng.random() < 0.05:
            line = line[:-1] + "\r\n"
        out.append(line)
    return out


def test_fuzz_of_format_and_sample_columns():
    hdr_text = F.header(extra=('##FORMAT=<ID=FL,Number=0,Type=Flag,Description="f">',
                               '##FORMAT=<ID=RR,Number=.,Type=Float,Description="r">')).encode()
    text = hdr_text + "".join(fuzz_lines(np.random.default_rng(20261020), 3000)).encode()
    assert check_text(text, "fuzz", samples=(0, 1), depths=(0, 5)) == 3000
    hdr = F.parse_header(text)
    seen = [F.eval_line(hdr, ln, 0, 1)["verdict"] for _, ln in F.body_lines(text, hdr[2])]
    kinds = [v[0] if isinstance(v, tuple) else v for v in seen]
    assert min(kinds.count(F.SKIP), kinds.count(F.SET), kinds.count(F.END)) > 300      # not vacuous
    assert kinds.count(F.ABORT) > 5


def test_first_five_columns_against_the_statement():
    heads = ["chr1\t100", "\t100", "chr1\t", "chr1\t+", "chr1\t+7", "chr1\t007", "chr1\t1x", "chr1\t-1", "chr1\t 5",
             "chr1\t4611686018427387903", "chr1\t4611686018427387904", "chr1\t99999999999999999999", "chr1\t4294967396",
             "c" * 300 + "\t5", "chr1", "", "#x\t1"]
    tails = ["\t.\tA\tC\t.\t.\t.", "\t.\tA\tC", "\t.\tA", "\t.\t\t\t.\t.\t.", "\t.\tAC\tC,G\t.\t.\t.", "\t.\tA\t.\t.\t.\t.",
             "\t.\tA\t,\t.\t.\t.\tGT\t0/1\t0/1", "\t.\tA\tC\t.\t.\t.\tGT:AD\t0/1:3,4\t0/1:5,6"]
    text = F.header().encode() + "".join(h + t + "\n" for h in heads for t in tails).encode()
    assert check_text(text, "heads") == len(heads) * len(tails)


def test_probe(tmp_path):
    import gzip
    import vafc
    files = {"a.vcf": golden("main.vcf"), "a.vcf.gz": golden("main.vcf.gz"), "b.vcf.gz": golden("main_bgzf.vcf.gz"),
             "c.bcf": b"BCF\2\2" + b"\0" * 40, "d.bcf": gzip.compress(b"BCF\2\2" + b"\0" * 40), "e.bcf": F.bgzf(b"BCF\2\2" + b"\0" * 40),
             "f.txt": b"hello\n", "g.txt": b""}
    want = {"a.vcf": "plain", "a.vcf.gz": "gzip", "b.vcf.gz": "bgzf", "c.bcf": "bcf", "d.bcf": "bcf", "e.bcf": "bcf",
            "f.txt": "other", "g.txt": "other"}
    for fn, data in files.items():
        (tmp_path / fn).write_bytes(data)
        assert vafc.vcf_probe(str(tmp_path / fn)) == want[fn], fn
    with pytest.raises(FileNotFoundError):
        vafc.vcf_probe(str(tmp_path / "nope"))


DENSE_ROWS = [(b"c", 0, b"r0", b"A", b"C"), (b"c", 4, b"r1", b"G", b"T")]
VCF_WAVE_BYTES = 1024      # a wave of the scan kernel ranks the line starts of 1 KB of a tile


def dense_texts():
    """{what: (line length or None, text)}: texts of one repeated minimal
    line, and a mixed one, that put up to 1,024 line starts into a wave's
    1 KB.  The 15- to 17-byte lines carry an ID of 1 to 3 bytes; 16 bytes is
    the sites-only form, where a 16-byte lane still sees at most one start."""
    lines = {"empty": b"\n", "hit_11": b"c\t1\t.\tA\tC\t\n", "hit_14": b"c\t5\t.\tG\tT\t.\t.\n",
             "hit_15": b"c\t1\ta\tA\tC\t.\t.\t\n", "hit_16": b"c\t1\t.\tA\tC\t.\t.\t.\n", "hit_17": b"c\t1\tabc\tA\tC\t.\t.\t\n"}
    out = {what: (len(ln), ln * (1200 if ln == b"\n" else 400)) for what, ln in lines.items()}
    # a hit, the row's position with other alleles, a line left to the host (five columns), an empty line
    cycle = [b"c\t1\t.\tA\tC\t\n", b"c\t5\t.\tG\tA\t.\n", b"c\t1\t.\tA\tC\n", b"\n", b"c\t5\t.\tG\tT\t\n", b"c\t1\tid\tT\tC\t\n"]
    assert all(8 <= len(ln) <= 12 for ln in cycle if ln != b"\n")
    out["mixed"] = (None, b"".join(cycle[i % len(cycle)] for i in range(900)))
    return out


def starts_per_wave(text: bytes):
    """Line starts in every full 1 KB of a text that lies at alignment 0."""
    offs = np.array([off for off, _ in F.body_lines(text, 0)])
    full = len(text) // VCF_WAVE_BYTES
    return np.bincount(offs // VCF_WAVE_BYTES, minlength=full)[:full]


def test_dense_texts_put_more_than_64_starts_into_a_wave():
    """The CPU side of test_more_than_64_lines_per_wave: the scan kernel hands
    a wave's starts to its lanes 64 at a time, and only these texts make it go
    round twice.  16-byte lines are the edge, exactly 64 starts, 17-byte lines
    lie on its other side."""
    texts = dense_texts()
    for what, (size, text) in texts.items():
        assert 400 <= text.count(b"\n") <= 1200 and text.endswith(b"\n")
        per_wave = starts_per_wave(text)
        assert per_wave.size >= 1
        if size == 16:
            assert (per_wave == 64).all()
        elif size == 17:
            assert ((per_wave == 60) | (per_wave == 61)).all()
        elif size == 1:
            assert (per_wave == 1024).all()
        else:
            assert (per_wave > 64).all(), what
        lines = F.device_lines(DENSE_ROWS, text)
        if size == 1:
            assert lines == [(i, -1) for i in range(1200)]
        elif size is not None:
            assert lines == [(i * size, 1 if size == 14 else 0) for i in range(400)]       # every line a hit
    mixed = F.device_lines(DENSE_ROWS, texts["mixed"][1])
    assert [r for _o, r in mixed[:4]] == [0, -1, -1, 1] and len(mixed) == 600      # two of six lines report nothing


def test_sanitizer_run_of_the_host_parser():
    """tools/vcf_reader_asan.sh: the parser and the inflater under ASan + UBSan in
    a stand-alone program, over the goldens and their truncations."""
    p = subprocess.run([os.path.join(ROOT, "tools", "vcf_reader_asan.sh")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "vcf_reader_asan: all clean" in p.stdout
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def matcher():
    import vafc
    m = vafc.VcfMatcher(rows=[(r[0], r[1], r[3], r[4]) for r in ROWS])
    yield m
    m.close()


def scan(m, text, file_off=0, final=True):
    consumed = m.scan_block(text, file_off, final)
    hits, cons2 = m.hits()
    assert cons2 == consumed
    return [(int(h["off"]), int(h["row"])) for h in hits], consumed


def consumed_of(text, final):
    return len(text) if final else text.rfind(b"\n") + 1


def check_scan(m, rows, text, file_off=0, final=True, index=None):
    got, consumed = scan(m, text, file_off, final)
    assert consumed == consumed_of(text, final)
    assert got == F.device_lines(rows, text[:consumed], file_off, index)
    return got


def sweep_text():
    """A few KB with hits, rows with other alleles, lines of their own and
    every kind of line the device leaves to the host."""
    body = F.synth_vcf(ROWS, 40, 2, seed=5, hit_rate=0.25, header_too=False)
    odd = ["chr1\t100\t.\tA\tC\n", "\t100\t.\tA\tC\t.\n", "chr1\t1x0\t.\tA\tC\t.\n", "chr1\t\t.\tA\tC\t.\n",
           "chr1\t" + "1" * 19 + "\t.\tA\tC\t.\n", "chr1\t000000000000000100\t.\tA\tC\t.\n", "c" * 256 + "\t100\t.\tA\tC\t.\n",
           "c" * 255 + "\t100\t.\tA\tC\t.\n", "chr1\t100\t.\tA\r\tC\t.\n", "\n", "#x\n", "chr1\t0\t.\tA\tC\t.\n",
           "chr1\t%d\t.\tA\tG\t.\n" % ((1 << 32) + 300), "chr1\t100\t.\tA\t,\t.\n", "chr1\t500\t.\tA\t.\t.\n",
           "chr1\t800\t.\tG\tT\t.\n", "chr1\t400\t.\tt\tc\t.\n"]
    lines = body.split(b"\n")[:-1]
    for i, o in enumerate(odd):
        lines.insert(2 * i + 1, o.encode()[:-1])
    return b"chr1\t100\t.\tA\tC\t.\n" + b"\n".join(lines) + b"\nchrX\t1\t.\tA\tC\t.\tlast\n"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_cli_equals_reference(name, tmp_path):
    e = MANIFEST[name]
    for fn in os.listdir(VCF_DIR):
        shutil.copy(os.path.join(VCF_DIR, fn), tmp_path)
    os.mkdir(tmp_path / "o")
    p = subprocess.run([CLI] + e["argv"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == e["rc"], p.stderr[-2000:]
    assert own_lines(p.stderr) == e["stderr"]
    out = tmp_path / "o" / "out.vaf"
    assert (F.vaf_entry(out.read_bytes()) if out.exists() else None) == golden_vaf(name)


@pytest.mark.gpu
def test_bcf_is_refused(tmp_path):
    (tmp_path / "x.bcf").write_bytes(F.bgzf(b"BCF\2\2" + b"\0" * 40))
    (tmp_path / "p.txt").write_text(F.panel_text())
    p = subprocess.run([CLI, "-p", "p.txt", "-v", "x.bcf", "-o", "o.vaf"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "x.bcf is BCF" in p.stderr and not (tmp_path / "o.vaf").exists()


@pytest.mark.gpu
def test_alignment_sweep(matcher):
    """Every line start on every position of a tile and of a 16-byte load: the
    text behind 0..tile bytes of one junk line, and at device pointers 1..15
    bytes off a 16-byte boundary."""
    import torch
    import vafc
    text = sweep_text()
    base = F.device_lines(ROWS, text)
    assert 2000 < len(text) < 8192 and sum(r >= 0 for _, r in base) >= 8 and sum(r < 0 for _, r in base) >= 9
    assert check_scan(matcher, ROWS, text) == base
    for pad in range(1, vafc.VCF_TILE_BYTES + 1):
        got, _ = scan(matcher, b"x" * (pad - 1) + b"\n" + text)
        assert got == [(0, -1)] + [(o + pad, r) for o, r in base], pad
    dev = torch.device("cuda", 0)
    for shift in range(1, 16):
        for pad in (0, 1, 1023 - shift, 4096 - shift):
            t = (b"x" * (pad - 1) + b"\n" if pad else b"") + text
            buf = torch.zeros(len(t) + 64, dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 16 == 0
            buf[shift:shift + len(t)] = torch.frombuffer(bytearray(t), dtype=torch.uint8).to(dev)
            torch.cuda.synchronize()
            matcher.scan_device(buf.data_ptr() + shift, len(t), 7, True, vafc.STREAM_CTX)
            hits, consumed = matcher.hits()
            assert consumed == len(t)
            assert [(int(h["off"]), int(h["row"])) for h in hits] == F.device_lines(ROWS, t, 7), (shift, pad)
            matcher.scan_device(buf.data_ptr() + shift, len(t) - 3, 0, False)      # torch's stream, a cut last line
            hits, consumed = matcher.hits()
            assert consumed == t.rfind(b"\n", 0, len(t) - 3) + 1
            assert [(int(h["off"]), int(h["row"])) for h in hits] == F.device_lines(ROWS, t[:consumed]), (shift, pad)


@pytest.mark.gpu
def test_more_than_64_lines_per_wave():
    """Minimal lines, up to 1,024 starts in a wave's 1 KB: the loop that hands
    a wave's starts to its lanes goes round up to 16 times, and the starts are
    ranked bit by bit.  Behind junk pads of 0..16 bytes, so that the waves'
    borders fall on every byte of a line."""
    import vafc
    m = vafc.VcfMatcher(rows=[(r[0], r[1], r[3], r[4]) for r in DENSE_ROWS])
    try:
        for what, (_size, text) in dense_texts().items():
            for pad in range(0, 17):
                t = (b"x" * (pad - 1) + b"\n" if pad else b"") + text
                got, consumed = scan(m, t)
                want = F.device_lines(DENSE_ROWS, t)
                assert consumed == len(t)
                if got != want:
                    i = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
                    pytest.fail("%s lines behind %d bytes: %d reported, %d expected, first difference at entry %d: %r, expected %r"
                                % (what, pad, len(got), len(want), i, got[i:i + 1], want[i:i + 1]))
    finally:
        m.close()


@pytest.mark.gpu
def test_tile_crossing(matcher):
    import vafc
    T = vafc.VCF_TILE_BYTES
    hit, last = b"chr1\t100\t.\tA\tC\t.\tfirst\n", b"chr1\t1000\t.\tA\tC\t.\tlast"
    long_id = b"chr10\t100\trs" + b"i" * (T + 500) + b"\tA\tC\t.\n"              # longer than a tile, a hit
    long_alt = b"chr1\t100\t.\tA\tC" + b"G" * (2 * T) + b"\t.\n"
    long_chr = b"c" * (T + 10) + b"\t100\t.\tA\tC\t.\n"
    long_tail = b"chr1_x\t100\t.\tA\tC\t.\t" + b"s" * (3 * T) + b"\n"
    text = hit + long_id + long_alt + hit + long_chr + long_tail + last
    for final in (True, False):
        got = check_scan(matcher, ROWS, text, 0, final)
        assert got[0] == (0, ROW["rsA"]) and (got[-1][1] == ROW["rsO"]) == final       # hits on the first and last line
    check_scan(matcher, ROWS, text + b"\n", 0, False)                                  # ends exactly on the newline
    check_scan(matcher, ROWS, text + b"\n", 5, True)
    for blob in (b"x" * 10, b"chr1\t100\t.\tA\tC\t." + b"y" * (2 * T)):                # no newline at all
        assert scan(matcher, blob, 0, False) == ([], 0)
        check_scan(matcher, ROWS, blob, 0, True)
    assert scan(matcher, b"", 0, True) == ([], 0)
    assert scan(matcher, b"\n", 0, False) == ([(0, -1)], 1)
    for cut in range(len(hit) - 2, len(hit) + 3):                                      # a block border around a newline
        check_scan(matcher, ROWS, (hit * 3)[:len(hit) + cut], 0, False)


@pytest.mark.gpu
@pytest.mark.parametrize("block", [1, 64, 1000, 4096])
def test_count_file_does_not_depend_on_the_block_size(block, matcher, tmp_path):
    """A line longer than the block grows the block (vc_vcf_set_block_bytes)."""
    text = golden("main.vcf") + F.synth_vcf(ROWS, 300, 2, seed=9, hit_rate=0.2, header_too=False)
    (tmp_path / "x.vcf").write_bytes(text)
    (tmp_path / "x.vcf.gz").write_bytes(F.bgzf(text, 3000))
    matcher.set_block_bytes(block)
    try:
        for s, d in ((0, 1), (1, 7)):
            want, _ = F.process_vcf(ROWS, text, s, d)
            for fn in ("x.vcf", "x.vcf.gz"):
                got, st = matcher.count_file(str(tmp_path / fn), s, d)
                assert [tuple(p) for p in got.reshape(-1, 2).tolist()] == want, (fn, s, d)
                assert st.bases == len(text) and st.blocks >= (1 if block >= 4096 else 10)
    finally:
        matcher.set_block_bytes(32 << 20)


@pytest.mark.gpu
def test_early_end_inside_a_later_block(matcher, tmp_path):
    text = golden("end_char.vcf")
    (tmp_path / "e.vcf").write_bytes(text)
    matcher.set_block_bytes(100)
    try:
        got, _ = matcher.count_file(str(tmp_path / "e.vcf"))
    finally:
        matcher.set_block_bytes(32 << 20)
    assert [tuple(p) for p in got.reshape(-1, 2).tolist()] == pairs("end_char")


@pytest.mark.gpu
def test_hit_list_overflow():
    import vafc
    rows = [(r[0], r[1], r[3], r[4]) for r in ROWS]
    text = b"".join(b"chr1\t%d\t.\tA\tC\t.\tline%d\n" % (100 * (1 + i % 20), i) for i in range(5000))
    want = F.device_lines(ROWS, text)
    assert len(want) > 3000
    a, b = vafc.VcfMatcher(rows=rows), vafc.VcfMatcher(rows=rows)
    try:
        b.set_max_hits(1)
        assert scan(a, text)[0] == want
        assert scan(b, text)[0] == want
        b.set_max_hits(7)                      # and again below what a later block needs
        assert scan(b, text + text, 11)[0] == F.device_lines(ROWS, text + text, 11)
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_names", [8, 64])
def test_probe_chains_in_a_full_table(n_names):
    """A table with as many slots as entries: every probe of a key that is not
    there walks the whole table, and names are prefixes of one another."""
    import vafc
    names = [b"c" * (1 + i) for i in range(n_names - 3)] + [b"chr1", b"chr10", b"chr1_x"]
    rows = [(nm, 99, b"rs%d" % i, b"A", b"C") for i, nm in enumerate(names)]
    m = vafc.VcfMatcher(rows=[(r[0], r[1], r[3], r[4]) for r in rows], table_slots=n_names)
    try:
        lines = [nm + b"\t100\t.\tA\tC\t.\n" for nm in names]
        lines += [nm + b"x\t100\t.\tA\tC\t.\n" for nm in names] + [nm + b"\t101\t.\tA\tC\t.\n" for nm in names]
        lines += [nm[:-1] + b"\t100\t.\tA\tC\t.\n" for nm in names if len(nm) > 1] + [nm + b"\t100\t.\tA\tG\t.\n" for nm in names]
        got = check_scan(m, rows, b"".join(lines))
        assert sorted(r for _, r in got) == sorted(list(range(n_names)) + list(range(n_names - 4)) + [n_names - 3])
    finally:
        m.close()
    with pytest.raises(vafc.VafcError):
        vafc.VcfMatcher(rows=[(r[0], r[1], r[3], r[4]) for r in rows], table_slots=n_names // 2)
    with pytest.raises(vafc.VafcError):
        vafc.VcfMatcher(rows=[(r[0], r[1], r[3], r[4]) for r in rows], table_slots=n_names + 1)


@pytest.mark.gpu
def test_empty_panel(tmp_path):
    import vafc
    m = vafc.VcfMatcher(rows=[])
    try:
        text = sweep_text()
        got = check_scan(m, [], text)
        assert got and all(r == -1 for _, r in got)
        (tmp_path / "m.vcf").write_bytes(golden("main.vcf"))
        counts, _ = m.count_file(str(tmp_path / "m.vcf"))
        assert counts.size == 0
    finally:
        m.close()


@pytest.mark.gpu
def test_scale_full_panel():
    """The 20,849 rows of the GRCh38 panel against 2 * 10^5 seeded lines."""
    import vafc
    import vafc_synth as S
    bed = S.read_bed(S.default_bed_path())
    rows = [(c.encode(), int(s), rs.encode(), ref.encode(), alt.encode()) for c, s, _e, rs, ref, alt in bed
            if len(ref) == 1 and len(alt) == 1 and ref in "ACGT" and alt in "ACGT"]      # the rows snp-pattern-gen keeps
    assert len(rows) == 20849
    text = F.synth_vcf(rows, 200_000, 1, seed=11, hit_rate=0.01, header_too=False)
    index = F.first_rows(rows)
    m = vafc.VcfMatcher(rows=[(r[0], r[1], r[3], r[4]) for r in rows])
    try:
        got = check_scan(m, rows, text, 1 << 33, False, index)
        assert len(got) > 1000
    finally:
        m.close()


@pytest.mark.gpu
def test_python_mirror(tmp_path):
    import vafc
    (tmp_path / "p.txt").write_text(F.panel_text())
    db = vafc.load_patterns(str(tmp_path / "p.txt"))
    assert vafc.find_pattern(db, "chr1", 99) == ROW["rsA"] and vafc.find_pattern(db, "chr1", -1) == ROW["rsK"]
    assert vafc.find_pattern(db, "chr1", 98) == -1
    got = vafc.process_vcf(os.path.join(VCF_DIR, "main.vcf.gz"), db, 1, 1)
    assert [tuple(p) for p in got.reshape(-1, 2).tolist()] == pairs("main_s1")
    assert not vafc.process_vcf(os.path.join(VCF_DIR, "junk.vcf"), db).any()
    assert not vafc.process_vcf(str(tmp_path / "nope.vcf"), db).any()

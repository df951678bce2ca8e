"""vcf-vaf-counter on BGZF input inflated on the device (VAFC_BGZF=device):
compressed members go to the GPU, the text is produced and scanned in HBM, and
the result is what the host path and the reference's goldens give."""
import json
import os
import subprocess

import numpy as np
import pytest

import bgzf_fixture as B
import vcf_fixture as F
from conftest import GOLDEN, PKG

CLI = os.path.join(PKG, "lib", "vcf-vaf-counter")
VCF_DIR = os.path.join(GOLDEN, "vcf")
with open(os.path.join(VCF_DIR, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
ROWS = F.load_patterns(F.panel_text().encode())


def golden(name):
    with open(os.path.join(VCF_DIR, name), "rb") as f:
        return f.read()


def golden_vaf(name):
    e = MANIFEST[name].get("vaf")
    return MANIFEST[e[1:]]["vaf"] if isinstance(e, str) else e


def own_lines(stderr: str) -> str:
    import re
    return "".join(ln + "\n" for ln in stderr.splitlines() if not re.match(r"\[[EWIDT]::", ln))


@pytest.fixture()
def bgzf_env():
    """VAFC_BGZF for the library loaded into this process, restored afterwards."""
    old = os.environ.get("VAFC_BGZF")

    def use(path):
        os.environ["VAFC_BGZF"] = path
    yield use
    if old is None:
        os.environ.pop("VAFC_BGZF", None)
    else:
        os.environ["VAFC_BGZF"] = old


@pytest.fixture(scope="module")
def matcher():
    import vafc
    m = vafc.VcfMatcher(rows=[(r[0], r[1], r[3], r[4]) for r in ROWS])
    yield m
    m.close()


def pairs_of(counts):
    return [tuple(p) for p in counts.reshape(-1, 2).tolist()]


def cli(argv, cwd, path):
    env = dict(os.environ, VAFC_BGZF=path)
    p = subprocess.run([CLI] + argv, cwd=cwd, capture_output=True, text=True, timeout=120, env=env)
    out = os.path.join(cwd, "o", "out.vaf")
    vaf = open(out, "rb").read() if os.path.exists(out) else None
    if vaf is not None:
        os.remove(out)
    return p.returncode, p.stderr, vaf


@pytest.mark.gpu
@pytest.mark.parametrize("payload", [400, 65280])
@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_goldens_rewrapped_as_bgzf(name, payload, tmp_path, matcher, bgzf_env):
    """Every golden input as BGZF members of `payload` bytes of text, under its own name: the CLI gives the
    golden's .vaf, stderr and exit code, and a file with a VCF header went through the device inflater."""
    e = MANIFEST[name]
    vcfs = []
    for fn in os.listdir(VCF_DIR):
        data = golden(fn)
        if fn.endswith((".vcf", ".vcf.gz")):
            text = F.text_of(data)
            data = B.bgzf_bytes(text, 6, payload)
            if text.startswith(b"##fileformat=VCF") and b"\n#CHROM" in text:
                vcfs.append(fn)
        (tmp_path / fn).write_bytes(data)
    os.mkdir(tmp_path / "o")
    rc, err, vaf = cli(e["argv"], str(tmp_path), "device")
    assert rc == e["rc"], err[-2000:]
    assert own_lines(err) == e["stderr"]
    assert (F.vaf_entry(vaf) if vaf is not None else None) == golden_vaf(name)
    used = [fn for fn in vcfs if fn in e["argv"]]
    bgzf_env("device")
    for fn in used:
        import vafc
        try:
            matcher.count_file(str(tmp_path / fn))
        except vafc.VafcError as ex:
            assert ex.code == vafc.VCF_ABORTED
        device_blocks, host_blocks = matcher.inflate_info()
        assert device_blocks > 0 and host_blocks > 0, fn


def long_line_text():
    """main.vcf's header and lines, then seeded lines with a hit line of more than 800 bytes among them."""
    head = golden("main.vcf")
    body = F.synth_vcf(ROWS, 300, 2, seed=9, hit_rate=0.2, header_too=False).split(b"\n")
    hit = [i for i, ln in enumerate(body) if ln and F.process_vcf(ROWS, head + ln + b"\n", 0, 1) != F.process_vcf(ROWS, head, 0, 1)]
    f = body[hit[3]].split(b"\t")
    f[7] = b"LONG=" + b"x" * 1000
    body[hit[3]] = b"\t".join(f)
    return head + b"\n".join(body), len(b"\t".join(f))


@pytest.mark.gpu
@pytest.mark.parametrize("block", [1, 64, 400, 1000, 4096])
def test_header_and_lines_across_members(block, matcher, tmp_path, bgzf_env):
    """Members of 150 bytes of text: the header is longer than two, the body starts inside one, a hit line spans
    more than three, and at vc_vcf_set_block_bytes of 1 to 4,096 hit lines straddle every kind of piece border."""
    text, long_len = long_line_text()
    body_off = text.index(b"\n#CHROM") + 1
    body_off = text.index(b"\n", body_off) + 1
    assert body_off > 300 and body_off % 150 != 0 and long_len > 800
    (tmp_path / "x.vcf.gz").write_bytes(B.bgzf_bytes(text, 6, 150))
    matcher.set_block_bytes(block)
    try:
        for s, d in ((0, 1), (1, 7)):
            want, _ = F.process_vcf(ROWS, text, s, d)
            got = {}
            for path in ("device", "host"):
                bgzf_env(path)
                counts, st = matcher.count_file(str(tmp_path / "x.vcf.gz"), s, d)
                got[path] = (pairs_of(counts), st.bases, st.seqs, st.blocks)
                assert pairs_of(counts) == want, (path, s, d)
                assert st.bases == len(text)
                info = matcher.inflate_info()
                assert (info[0] > 0) == (path == "device") and info[1] > 0
            assert got["device"] == got["host"]
    finally:
        matcher.set_block_bytes(32 << 20)


@pytest.mark.gpu
def test_early_end_inside_a_later_piece(matcher, tmp_path, bgzf_env):
    text = golden("end_char.vcf")
    (tmp_path / "e.vcf.gz").write_bytes(B.bgzf_bytes(text, 6, 400))
    want, _ = F.process_vcf(ROWS, text, 0, 1)
    matcher.set_block_bytes(100)
    try:
        bgzf_env("device")
        got, _ = matcher.count_file(str(tmp_path / "e.vcf.gz"))
        assert matcher.inflate_info()[0] > 0
    finally:
        matcher.set_block_bytes(32 << 20)
    assert pairs_of(got) == want


def damaged_files():
    text = golden("main.vcf") + F.synth_vcf(ROWS, 300, 2, seed=9, hit_rate=0.2, header_too=False)
    ms = B.wrap(text, 6, payload_size=1000) + [B.EOF_MEMBER]
    good = b"".join(m.raw() for m in ms)
    out = {}
    j = 11
    bad = B.Member(ms[j].payload, ms[j].isize, ms[j].crc ^ 0x40)
    out["wrong_crc"] = b"".join((bad if i == j else m).raw() for i, m in enumerate(ms))
    flipped = bytearray(ms[j].payload)
    flipped[len(flipped) // 2] ^= 0x10
    out["flipped_bit"] = b"".join((B.Member(flipped, ms[j].isize, ms[j].crc) if i == j else m).raw() for i, m in enumerate(ms))
    out["cut"] = good[:len(good) * 2 // 3]
    import zlib
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    at = sum(len(m.raw()) for m in ms[:j])
    out["gzip_member_inside"] = good[:at] + c.compress(text[j * 1000:(j + 1) * 1000]) + c.flush() + good[at + len(ms[j].raw()):]
    out["isize_65537"] = good[:at] + B.malformed_cases()["bad_isize_65537"].raw() + good[at:]
    out["trailing_bytes"] = good + b"not a member"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["wrong_crc", "flipped_bit", "cut", "gzip_member_inside", "isize_65537", "trailing_bytes"])
def test_damaged_files_give_what_the_host_path_gives(kind, tmp_path, matcher, bgzf_env):
    """The whole file is counted again by the host path: .vaf, stderr and exit code are its, byte for byte."""
    (tmp_path / "p.txt").write_text(F.panel_text())
    (tmp_path / "d.vcf.gz").write_bytes(damaged_files()[kind])
    os.mkdir(tmp_path / "o")
    argv = ["-p", "p.txt", "-v", "d.vcf.gz", "-o", "o/out.vaf"]
    host = cli(argv, str(tmp_path), "host")
    dev = cli(argv, str(tmp_path), "device")
    assert dev == host and host[2] is not None
    bgzf_env("device")
    counts, _ = matcher.count_file(str(tmp_path / "d.vcf.gz"))
    assert matcher.inflate_info()[0] == 0 and matcher.inflate_info()[1] > 0   # the host path's result
    assert counts.any()
    bgzf_env("host")
    assert pairs_of(matcher.count_file(str(tmp_path / "d.vcf.gz"))[0]) == pairs_of(counts)


def head_walk(data: bytes) -> int:
    """Members by their heads alone, as vc_vcf_inflate_info counts them after a fallback: the fixed bytes, the extra
    field, a BSIZE that can hold both and the trailer, then a seek past the body (whether or not it is there)."""
    n = at = 0
    while len(data) - at >= 12 and data[at:at + 3] == b"\x1f\x8b\x08" and data[at + 3] & 4:
        xlen = int.from_bytes(data[at + 10:at + 12], "little")
        extra = data[at + 12:at + 12 + xlen]
        if len(extra) != xlen:
            break
        bsize, i = None, 0
        while i + 4 <= xlen and bsize is None:
            slen = int.from_bytes(extra[i + 2:i + 4], "little")
            if extra[i:i + 2] == b"BC" and slen == 2 and i + 6 <= xlen:
                bsize = int.from_bytes(extra[i + 4:i + 6], "little")
            i += 4 + slen
        if bsize is None or bsize + 1 < 12 + xlen + 8:
            break
        at += bsize + 1
        n += 1
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("kind,members", [("wrong_crc", 24), ("flipped_bit", 24), ("cut", 16), ("gzip_member_inside", 11),
                                          ("isize_65537", 25), ("trailing_bytes", 24)])
def test_host_blocks_after_a_fallback_is_the_head_walk(kind, members, tmp_path, matcher, bgzf_env):
    """A member whose head is whole counts even when its body is cut (`cut`: 16, not the 15 whole members)."""
    data = damaged_files()[kind]
    assert head_walk(data) == members
    (tmp_path / "d.vcf.gz").write_bytes(data)
    bgzf_env("device")
    matcher.count_file(str(tmp_path / "d.vcf.gz"))
    assert matcher.inflate_info() == (0, members)


def both_paths(matcher, bgzf_env, path, text, blocks):
    """Counts, st.bases and st.seqs of the device path are the host path's at every block size, and the counts
    process_vcf's; inflate_info of the device path at the last block size."""
    want, _ = F.process_vcf(ROWS, text, 0, 1)
    info = None
    try:
        for block in blocks:
            matcher.set_block_bytes(block)
            got = {}
            for p in ("device", "host"):
                bgzf_env(p)
                counts, st = matcher.count_file(path)
                got[p] = (pairs_of(counts), st.bases, st.seqs)
                assert pairs_of(counts) == want and st.bases == len(text), (p, block)
                if p == "device":
                    info = tuple(matcher.inflate_info())
            assert got["device"] == got["host"], block
    finally:
        matcher.set_block_bytes(32 << 20)
    return want, info


def header_and_body():
    text = golden("main.vcf") + F.synth_vcf(ROWS, 40, 2, seed=9, hit_rate=0.2, header_too=False)
    body_off = text.index(b"\n", text.index(b"\n#CHROM") + 1) + 1
    return text[:body_off], text[body_off:]


@pytest.mark.gpu
@pytest.mark.parametrize("empty_between", [False, True])
def test_first_data_line_at_a_members_first_byte(empty_between, matcher, tmp_path, bgzf_env):
    """The header ends with a member: the device starts behind the header's members, with nothing to skip."""
    header, body = header_and_body()
    data = B.bgzf_bytes(header, 6, 150, eof=False) + (B.EOF_MEMBER.raw() if empty_between else b"") + B.bgzf_bytes(body, 6, 150)
    assert len(data) < 10_000
    (tmp_path / "b.vcf.gz").write_bytes(data)
    want, info = both_paths(matcher, bgzf_env, str(tmp_path / "b.vcf.gz"), header + body, [1, 4096])
    assert any(p != (0, 0) for p in want)
    assert info[0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("eof", [True, False])
def test_header_and_no_data_line(eof, matcher, tmp_path, bgzf_env):
    """Nothing to scan: all counts zero.  The device path finished: a fallback would report (0, every member of
    the file), the EOF member among them; without one the file gives the device nothing to inflate."""
    header, _ = header_and_body()
    (tmp_path / "h.vcf.gz").write_bytes(B.bgzf_bytes(header, 6, 150, eof=eof))
    want, info = both_paths(matcher, bgzf_env, str(tmp_path / "h.vcf.gz"), header, [4096])
    assert all(p == (0, 0) for p in want)
    assert info == ((1 if eof else 0), -(-len(header) // 150))


@pytest.mark.gpu
def test_last_line_without_newline_across_pieces(matcher, tmp_path, bgzf_env):
    """The unterminated last line arrives as the tail of the piece before an empty last piece."""
    head = golden("nonl.vcf")
    n_samples = len(head[head.index(b"\n#CHROM") + 1:].split(b"\n")[0].split(b"\t")) - 9
    more = F.synth_vcf(ROWS, 8, n_samples, seed=5, hit_rate=0.5, header_too=False)
    text = head + b"\n" + more[:-1]
    assert 200 < len(more) < 1000 and more.endswith(b"\n") and not text.endswith(b"\n")
    data = B.bgzf_bytes(text, 6, 150)
    assert len(data) < 10_000
    (tmp_path / "n.vcf.gz").write_bytes(data)
    want, info = both_paths(matcher, bgzf_env, str(tmp_path / "n.vcf.gz"), text, [1, 64, 1000])
    assert any(p != (0, 0) for p in want) and info[0] > 0


@pytest.mark.gpu
def test_scale_full_panel(tmp_path, bgzf_env):
    """2 * 10^4 seeded lines, 65,280-byte members, against the 20,849 rows of the GRCh38 panel."""
    import vafc
    import vafc_synth as S
    bed = S.read_bed(S.default_bed_path())
    rows = [(c.encode(), int(s), rs.encode(), ref.encode(), alt.encode()) for c, s, _e, rs, ref, alt in bed
            if len(ref) == 1 and len(alt) == 1 and ref in "ACGT" and alt in "ACGT"]
    assert len(rows) == 20849
    text = F.synth_vcf(rows, 20_000, 2, seed=12, hit_rate=0.02)
    (tmp_path / "s.vcf.gz").write_bytes(B.bgzf_bytes(text, 6, 65280))
    (tmp_path / "s.vcf").write_bytes(text)
    m = vafc.VcfMatcher(rows=[(r[0], r[1], r[3], r[4]) for r in rows])
    try:
        plain, _ = m.count_file(str(tmp_path / "s.vcf"))
        bgzf_env("device")
        got, st = m.count_file(str(tmp_path / "s.vcf.gz"))
        assert m.inflate_info()[0] >= len(text) // 65280
        assert st.bases == len(text)
        assert np.array_equal(got, plain) and int((got != 0).sum()) > 300
    finally:
        m.close()

"""bam-vaf-counter with BGZF inflated and the records found on the device
($VAFC_BGZF=device; needs an MI355X): every case of tests/golden/bam/manifest.json
through the CLI against its golden .vaf, stderr and exit code, with the line
VAFC_PHASES prints per file showing where the file's members were inflated; the
clean goldens wrapped again at 400, 1,024 and 65,280 bytes of text per member,
whole and in several pieces, plain and beside an index; two input files of
which the second falls back; and a damaged file of each BGZF kind of
tests/test_vcf_bgzf.py, byte for byte against $VAFC_BGZF=host.

What falls back is what include/vafc.h lists at vc_bam_count_file: members
that do not inflate or are no whole members, irregular records (d_mismatch*,
the CG convention of cg.bam), a short block_size (d_bs8).  A missing EOF member
and a last record cut off at a member's end (d_noeof, d_border) end nothing
and a file, as on the host, and stay on the device."""
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bam_fixture as F
import bgzf_fixture as B
from test_bam import BAM_DIR, CLI, MANIFEST, assert_vaf_equals, golden_vaf, own_lines

pytestmark = pytest.mark.gpu

FALLS_BACK = {"cg.bam", "d_midblock.bam", "d_flip.bam", "d_mismatch.bam", "d_mismatch_twice.bam", "d_mismatch_thrice.bam",
              "d_mismatch_batch.bam", "d_bs8.bam"}
PHASE = re.compile(r"^\[P::main\] (\S+): inflate host (\d+) device (\d+) members, (\d+) records, (\d+) bases")


def run_cli(argv, cwd, path, **env):
    e = dict(os.environ, VAFC_BGZF=path, VAFC_PHASES="1", **env)
    p = subprocess.run([CLI] + list(argv), cwd=str(cwd), capture_output=True, timeout=120, env=e)
    lines = p.stderr.decode().splitlines()
    phases = {m.group(1): tuple(int(x) for x in m.groups()[1:]) for m in map(PHASE.match, lines) if m}
    stderr = own_lines("".join(ln + "\n" for ln in lines if not ln.startswith("[P::")))
    out = os.path.join(str(cwd), "o", "out.vaf")
    vaf = None
    if os.path.exists(out):
        with open(out, "rb") as f:
            vaf = f.read()
        os.unlink(out)
    return p.returncode, stderr, vaf, phases


def link_goldens(tmp_path):
    for fn in os.listdir(BAM_DIR):
        os.symlink(os.path.join(BAM_DIR, fn), str(tmp_path / fn))
    os.mkdir(str(tmp_path / "o"))


def members_of(path):
    with open(path, "rb") as f:
        return len(F.bgzf_blocks(f.read()))


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_goldens_on_the_device(name, tmp_path):
    entry = MANIFEST[name]
    link_goldens(tmp_path)
    rc, stderr, vaf, phases = run_cli(entry["argv"], tmp_path, "device")
    assert rc == entry["rc"]
    assert stderr == entry["stderr"]
    want = golden_vaf(name)
    if want is None:
        assert vaf is None
    else:
        out = str(tmp_path / "got.vaf")
        with open(out, "wb") as f:
            f.write(vaf)
        assert_vaf_equals(out, want)
    for fn, (host, device, _recs, _bases) in phases.items():
        if fn in FALLS_BACK:
            assert device == 0 and host > 0, (fn, host, device)
        elif not fn.startswith("d_"):
            # the header's members on the host, every member from the first record's on the device
            assert device >= members_of(os.path.join(BAM_DIR, fn)) - host and device > 0 and host >= 1, (fn, host, device)
        else:
            assert fn in ("d_noeof.bam", "d_border.bam") and device > 0


def text_of(path):
    with open(path, "rb") as f:
        raw = f.read()
    return b"".join(zlib.decompress(raw[o + 18:o + n - 8], -15) for o, n in F.bgzf_blocks(raw))


@pytest.mark.parametrize("block", [400, 1024, 65280])
@pytest.mark.parametrize("src", ["a.bam", "b.bam", "long.bam", "small.bam"])
def test_goldens_rewrapped(src, block, tmp_path, monkeypatch):
    """The same text in members of `block` bytes (at 1,024 nearly every border
    cuts a record), plain and beside an index, whole and in pieces of a few
    members: the counts, records and bases of the host pass."""
    import vafc
    from test_bam import load_rows
    db, _rows = load_rows(os.path.join(BAM_DIR, "p.txt"))
    text = text_of(os.path.join(BAM_DIR, src))
    path = str(tmp_path / "w.bam")
    with open(path, "wb") as f:
        f.write(F.bgzf(text, block))
    n_members = members_of(path)
    bc = vafc.create_snp_map(db, os.path.join(BAM_DIR, "a.bam"))
    try:
        for indexed in (False, True):
            if indexed:
                with open(os.path.join(BAM_DIR, "a.index"), "rb") as f, open(path + ".bai", "wb") as g:
                    g.write(f.read())
            monkeypatch.setenv("VAFC_BGZF", "host")
            monkeypatch.delenv("VAFC_BATCH_BYTES", raising=False)
            bc.reset()
            hst = bc.count_file(path)
            want = bc.finish()
            assert bc.inflate_info() == (n_members, 0) and want.any()
            monkeypatch.setenv("VAFC_BGZF", "device")
            for batch in (None, 3000, 70000):
                if batch:
                    monkeypatch.setenv("VAFC_BATCH_BYTES", str(batch))
                bc.reset()
                st = bc.count_file(path)
                got = bc.finish()
                host, device = bc.inflate_info()
                assert device > 0 and host >= 1 and host + device >= n_members, (indexed, batch, host, device)
                assert (st.seqs, st.bases) == (hst.seqs, hst.bases), (indexed, batch)
                assert np.array_equal(got, want), (indexed, batch, np.nonzero(got != want)[0][:8])
                if batch == 3000 and block <= 1024 and len(text) > 20000:
                    assert st.blocks > 3
    finally:
        bc.close()


def test_second_file_falls_back_and_the_first_files_counts_survive(tmp_path):
    link_goldens(tmp_path)
    argv = ["-p", "p.txt", "-o", "o/out.vaf", "a.bam", "d_mismatch.bam", "b.bam"]
    host = run_cli(argv, tmp_path, "host")
    dev = run_cli(argv, tmp_path, "device")
    assert dev[:3] == host[:3] and host[0] == 0 and host[2] is not None
    assert all(p[1] == 0 for p in host[3].values())
    ph = dev[3]
    assert ph["a.bam"][1] > 0 and ph["d_mismatch.bam"][1] == 0 and ph["b.bam"][1] > 0
    assert {fn: p[2:] for fn, p in ph.items()} == {fn: p[2:] for fn, p in host[3].items()}      # records and bases
    # and the first file alone counts less
    alone = run_cli(["-p", "p.txt", "-o", "o/out.vaf", "a.bam"], tmp_path, "device")
    assert alone[2] != dev[2]


def test_fallback_restores_counts_in_process(tmp_path, monkeypatch):
    import vafc
    from test_bam import load_rows
    db, _rows = load_rows(os.path.join(BAM_DIR, "p.txt"))
    a, bad = os.path.join(BAM_DIR, "a_i.bam"), os.path.join(BAM_DIR, "d_mismatch_thrice.bam")
    bc = vafc.create_snp_map(db, a)
    try:
        monkeypatch.setenv("VAFC_BGZF", "host")
        for fn in (a, bad, a):
            bc.count_file(fn)
        want = bc.finish()
        bc.reset()
        monkeypatch.setenv("VAFC_BGZF", "device")
        seen = []
        for fn in (a, bad, a):
            bc.count_file(fn)
            seen.append(bc.inflate_info()[1] > 0)
        assert seen == [True, False, True]
        assert np.array_equal(bc.finish(), want) and want.any()
    finally:
        bc.close()


def damaged_bams():
    with open(os.path.join(BAM_DIR, "small.bam"), "rb") as f:
        good = f.read()
    blocks = F.bgzf_blocks(good)
    j = len(blocks) // 2
    off, size = blocks[j]
    out = {}
    crc = bytearray(good)
    crc[off + size - 8] ^= 0x40
    out["wrong_crc"] = bytes(crc)
    flipped = bytearray(good)
    flipped[off + 18 + (size - 26) // 2] ^= 0x10
    out["flipped_bit"] = bytes(flipped)
    out["cut"] = good[:len(good) * 2 // 3]
    text = zlib.decompress(good[off + 18:off + size - 8], -15)
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    out["gzip_member_inside"] = good[:off] + c.compress(text) + c.flush() + good[off + size:]
    out["isize_65537"] = good[:off] + B.malformed_cases()["bad_isize_65537"].raw() + good[off:]
    out["trailing_bytes"] = good + b"not a member"
    return out


@pytest.mark.parametrize("kind", ["wrong_crc", "flipped_bit", "cut", "gzip_member_inside", "isize_65537", "trailing_bytes"])
def test_damaged_files_give_what_the_host_path_gives(kind, tmp_path):
    link_goldens(tmp_path)
    (tmp_path / "d.bam").write_bytes(damaged_bams()[kind])
    argv = ["-p", "p.txt", "-o", "o/out.vaf", "d.bam"]
    host = run_cli(argv, tmp_path, "host")
    dev = run_cli(argv, tmp_path, "device")
    assert dev[:3] == host[:3] and host[0] == 0 and host[2] is not None
    assert dev[3]["d.bam"][1] == 0 and dev[3]["d.bam"][2:] == host[3]["d.bam"][2:]
    assert host[3]["d.bam"][2] > 0                   # the records in front of the damage

"""The device BGZF inflater (vc_bgzf_*, kmer-cnt_amd/csrc/vafc_bgzf.hip) against
the statement of tests/bgzf_fixture.py: for every class of stream the text,
the per-block status and the ok prefix are zlib's, and the guard bytes around
every block's output range stay as they were.  vc_bgzf_index, which needs no
GPU, is tested here too."""
import zlib

import numpy as np
import pytest

import bgzf_fixture as F

GUARD = 0xA5
GAP = 24        # guard bytes in front of and behind every block's range


@pytest.fixture(scope="module")
def inflater():
    import vafc
    z = vafc.BgzfInflater()
    yield z
    z.close()


def batch_of(members, gaps=None):
    """(raw bytes, descriptors) of members laid out one behind the other, every output range between guards."""
    import vafc
    raw = b"".join(m.raw() for m in members)
    blocks = np.zeros(len(members), dtype=vafc.BGZF_BLOCK)
    at, out = 0, GAP
    for i, m in enumerate(members):
        blocks[i] = (at + m.payload_offset(), len(m.payload), m.isize, out, m.crc & 0xFFFFFFFF, 0)
        at += len(m.raw())
        room = m.isize if m.isize <= F.MAX_TEXT else 0
        out += room + (GAP if gaps is None else gaps[i])
    return raw, blocks, out


def check(inflater, members, what, gaps=None, device=False):
    """Inflate members as one batch; compare with the statement.  Returns the status list."""
    raw, blocks, cap = batch_of(members, gaps)
    if device:
        import torch
        d_raw = torch.from_numpy(np.frombuffer(raw + b"\0", dtype=np.uint8).copy()).cuda()
        d_blk = torch.from_numpy(blocks.view(np.uint8).copy() if len(blocks) else np.zeros(8, np.uint8)).cuda()
        d_out = torch.full((cap,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        inflater.inflate_device(d_raw.data_ptr(), len(raw), d_blk.data_ptr(), len(blocks), d_out.data_ptr(), cap)
        status, ok_prefix = inflater.status()
        text = d_out.cpu().numpy().tobytes()
    else:
        text = inflater.inflate(raw, blocks, text_cap=cap, fill=GUARD)
        status, ok_prefix = inflater.status()
    assert len(status) == len(members), what
    want_ok = []
    at = 0
    for i, m in enumerate(members):
        ok, want = m.verdict()
        want_ok.append(ok)
        off, room = int(blocks[i]["out_off"]), (m.isize if m.isize <= F.MAX_TEXT else 0)
        assert text[at:off] == bytes([GUARD]) * (off - at), (what, i, "guard in front")
        at = off + room
        assert (status[i] == 0) == ok, (what, i, int(status[i]))
        if ok:
            assert text[off:off + room] == want, (what, i)
        if m.code is not None:
            assert status[i] == m.code, (what, i, int(status[i]))
    assert text[at:] == bytes([GUARD]) * (len(text) - at), (what, "guard behind")
    assert ok_prefix == (want_ok + [False]).index(False), what
    return status


CASES = sorted(F.cases())


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_case_equals_statement(name, inflater):
    """Kinds, hand-encoded lengths and distances, dynamic headers, sizes, payload offsets and the malformed
    streams (each after the sanitizer run of the same decode text, tests/test_bgzf_fixture.py): host bytes."""
    check(inflater, F.cases()[name], name)


@pytest.mark.gpu
def test_device_buffers_outputs_at_every_offset(inflater):
    """HBM-resident input, descriptors and output; the outputs start at every offset mod 16."""
    ms = F.cases()["layout_xlen"] + F.cases()["hand_edges"] + F.cases()["bad_between_good"] + [F.EOF_MEMBER]
    gaps = [GAP + (i * 7 + 3) % 16 for i in range(len(ms))]
    raw, blocks, _cap = batch_of(ms, gaps)
    assert {int(o) % 16 for o in blocks["out_off"]} == set(range(16))
    check(inflater, ms, "device", gaps, device=True)
    assert inflater.kernel_ms() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_batch_sizes(n, inflater):
    text = F.fastq_text(40, 200 * 65)
    ms = [F.member_of(text[200 * i:200 * i + 150 + i], F.deflate_raw(text[200 * i:200 * i + 150 + i], 1 + i % 9)) for i in range(n)]
    status = check(inflater, ms, "batch of %d" % n)
    assert len(status) == n and not status.any()


@pytest.mark.gpu
def test_more_blocks_than_the_grid_holds(inflater):
    """256 CUs x 32 workgroups is the largest grid: 8,500 blocks make every workgroup stride, and a bad block in
    the second round is found where it is."""
    import vafc
    text = F.fastq_text(41, 4000)
    kinds = [F.member_of(text[40 * i:40 * i + 30 + i], F.deflate_raw(text[40 * i:40 * i + 30 + i], 6)) for i in range(50)]
    ms = [kinds[i % 50] for i in range(8500)]
    ms[8300] = F.malformed_cases()["bad_crc"]
    raw, blocks, cap = batch_of(ms)
    out = inflater.inflate(raw, blocks, text_cap=cap, fill=GUARD)
    status, ok_prefix = inflater.status()
    assert ok_prefix == 8300 and status[8300] == F.ECRC and int((status != 0).sum()) == 1
    for i in (0, 49, 8191, 8192, 8299, 8301, 8499):
        off = int(blocks[i]["out_off"])
        assert out[off - GAP:off + ms[i].isize + GAP] == bytes([GUARD]) * GAP + ms[i].verdict()[1] + bytes([GUARD]) * GAP, i
    # descriptors that point outside the buffers are refused untouched
    bad = blocks[:4].copy()
    bad[1]["in_off"] = len(raw) - 3
    bad[2]["out_off"] = cap - 5
    bad[3]["in_len"] = 70000
    out = inflater.inflate(raw, bad, text_cap=cap, fill=GUARD)
    status, ok_prefix = inflater.status()
    assert status.tolist() == [0, F.EISIZE, F.EISIZE, F.EISIZE] and ok_prefix == 1
    assert out[int(blocks[0]["out_off"]) + ms[0].isize:] == bytes([GUARD]) * (cap - int(blocks[0]["out_off"]) - ms[0].isize)


def test_index_of_members():
    """vc_bgzf_index: cut members, a plain gzip member among BGZF ones, trailing bytes, final on and off."""
    import vafc
    text = F.fastq_text(42, 3000)
    ms = F.wrap(text, 6, payload_size=700, xpad=5) + [F.EOF_MEMBER]
    raw = b"".join(m.raw() for m in ms)
    blocks, consumed, why = vafc.bgzf_index(raw)
    assert why == "ok" and consumed == len(raw) and len(blocks) == len(ms) == 6
    at = out = 0
    for b, m in zip(blocks, ms):
        assert (int(b["in_off"]), int(b["in_len"]), int(b["isize"]), int(b["out_off"]), int(b["crc32"]), int(b["reserved"])) == \
            (at + m.payload_offset(), len(m.payload), m.isize, out, m.crc, 0)
        at += len(m.raw())
        out += m.isize
    sizes = np.cumsum([0] + [len(m.raw()) for m in ms])
    # cut at every byte of the second member: the first is whole, the walk asks for more, or refuses when final
    for cut in range(int(sizes[1]), int(sizes[2])):
        b, consumed, why = vafc.bgzf_index(raw[:cut], final=False)
        assert (len(b), consumed, why) == (1, sizes[1], "more" if cut > sizes[1] else "ok"), cut
        b, consumed, why = vafc.bgzf_index(raw[:cut], final=True)
        assert (len(b), consumed, why) == (1, sizes[1], "not_member" if cut > sizes[1] else "ok"), cut
    # a plain gzip member in the middle, trailing bytes, bytes that only begin like a member
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    plain = c.compress(b"plain gzip") + c.flush()
    mixed = raw[:sizes[2]] + plain + raw[sizes[2]:]
    for final in (False, True):
        b, consumed, why = vafc.bgzf_index(mixed, final=final)
        assert (len(b), consumed, why) == (2, sizes[2], "not_member")
        b, consumed, why = vafc.bgzf_index(raw + b"trailing", final=final)
        assert (len(b), consumed, why) == (6, len(raw), "not_member")
    b, consumed, why = vafc.bgzf_index(raw + b"\x1f\x8b\x08", final=False)
    assert (len(b), consumed, why) == (6, len(raw), "more")
    b, consumed, why = vafc.bgzf_index(raw + b"\x1f\x8b\x08\x00", final=False)   # FEXTRA is not set
    assert (len(b), consumed, why) == (6, len(raw), "not_member")
    # a descriptor list that is too short; an ISIZE no BGZF block can have
    b, consumed, why = vafc.bgzf_index(raw, cap=3)
    assert (len(b), consumed, why) == (3, sizes[3], "full")
    big = F.malformed_cases()["bad_isize_65537"].raw()
    b, consumed, why = vafc.bgzf_index(raw[:sizes[1]] + big + raw)
    assert (len(b), consumed, why) == (1, sizes[1], "too_long")
    assert vafc.bgzf_index(b"")[1:] == (0, "ok")
    # a BSIZE too small for its own header and trailer
    m = bytearray(ms[0].raw())
    m[16:18] = (20).to_bytes(2, "little")
    assert vafc.bgzf_index(bytes(m))[1:] == (0, "not_member")

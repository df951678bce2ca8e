"""The cases of tests/bgzf_fixture.py are what they claim to be, and the decode
text of the device inflater passes them on the CPU, under the sanitizers,
before any of them meets a GPU (tools/bgzf_inflate_asan.sh)."""
import os
import subprocess
import zlib

import pytest

import bgzf_fixture as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def info_of(name, i=0):
    m = F.cases()[name][i]
    text, info = F.inspect(m.payload)
    ok, ztext = m.verdict()
    assert ok and text == ztext, name
    return info


def test_helpers_decode_under_zlib_to_what_was_asked():
    for ops in (F.hand_all_codes(), F.hand_edges(), F.hand_far()):
        want = F.expand(ops)
        assert zlib.decompress(F.fixed_stream(ops), -15) == want
    # the writer: level, strategy, payload size, XLEN
    text = F.fastq_text(21, 10000)
    ms = F.wrap(text, 9, payload_size=400, xpad=7)
    assert len(ms) == 25 and all(m.isize == 400 for m in ms)
    raw = b"".join(m.raw() for m in ms) + F.EOF_MEMBER.raw()
    assert zlib.decompress(raw, 31) == text[:400]   # the first gzip member
    d, out = raw, b""
    while d:
        o = zlib.decompressobj(31)
        out += o.decompress(d)
        d = o.unused_data
    assert out == text
    assert all(len(m.raw()) - len(m.payload) == 12 + 6 + 7 + 8 for m in ms)
    # a dynamic block from chosen lengths and a chosen coding of them
    w = F.BitWriter()
    lit = F.complete_lengths(286)
    ops = [("lit", 1), ("lit", 2), ("match", 258, 2), ("match", 3, 1)]
    F.dynamic_block(w, lit, F.complete_lengths(30), ops)
    assert zlib.decompress(w.done(), -15) == F.expand(ops)
    # every non-malformed case is ok under the statement; the plain inflater agrees with zlib on all of them
    for name, ms in F.cases().items():
        if name.startswith(("bad_", "truncated_")):
            continue
        for m in ms:
            ok, text = m.verdict()
            assert ok, name
            assert F.inspect(m.payload)[0] == text, name


def test_kinds_hold_what_they_are_named_for():
    assert set(info_of("stored_level0")["btypes"]) == {0}
    assert 0 in info_of("stored_empty_sync")["stored"] and 2 in info_of("stored_empty_sync")["btypes"]
    assert info_of("stored_65280")["stored"][0] == 65280
    for n in (0, 1, 2, 3):
        assert info_of("fixed_%d" % n)["btypes"] == [1] and F.cases()["fixed_%d" % n][0].isize == n
    assert set(info_of("fixed_text")["btypes"]) == {1} and info_of("fixed_text")["matches"]
    for lvl in (1, 6, 9):
        i = info_of("dynamic_l%d" % lvl)
        assert 2 in i["btypes"] and i["matches"] and F.cases()["dynamic_l%d" % lvl][0].isize == 65280
    i = info_of("huffman_only")
    assert 2 in i["btypes"] and not i["matches"] and all(h["n_dist"] == 0 or h["max_dist"] <= 1 for h in i["headers"])
    i = info_of("rle")
    # (zlib always sends two distance codes; the stream with one is dyn_one_distance_code)
    assert i["matches"] and {d for _l, d, _o in i["matches"]} == {1} and all(h["n_dist"] <= 2 for h in i["headers"])
    for name in ("multi_full_flush", "multi_sync_flush"):
        i = info_of(name)
        assert len(i["btypes"]) >= 7 and i["stored"].count(0) >= 3, name
    assert [m.isize for m in F.cases()["eof_at_end"]][-1] == 0 and F.cases()["eof_at_end"][-1].raw() == F.EOF_MEMBER.raw()
    mid = F.cases()["eof_in_middle"]
    assert mid[1].raw() == F.EOF_MEMBER.raw() and mid[0].isize and mid[2].isize


def test_hand_encoded_lengths_and_distances():
    i = info_of("hand_all_codes")
    for s in range(29):
        assert (s, 0) in i["lsyms"] and (s, (1 << F.LEXTRA[s]) - 1) in i["lsyms"], s
    for d in range(30):
        assert (d, 0) in i["dsyms"] and (d, (1 << F.DEXTRA[d]) - 1) in i["dsyms"], d
    assert (27, 31) in i["lsyms"] and (28, 0) in i["lsyms"]   # 258 both ways
    i = info_of("hand_edges")
    m = {(l, d) for l, d, _o in i["matches"]}
    assert (258, 1) in m and (3, 1) in m
    for d in (2, 3, 63, 64, 65):
        for l in (max(3, d - 1), max(3, d), d + 1, 63, 64, 65, 127, 128, 129, 258):
            assert (l, d) in m, (l, d)
    assert any(d == o for _l, d, o in i["matches"])   # a source that starts at the block's first byte
    i = info_of("hand_far")
    assert (258, 32768, 32768) in i["matches"] and any(d == 32768 and o > 32768 for _l, d, o in i["matches"])


def test_dynamic_headers_hold_what_they_are_named_for():
    assert info_of("dyn_15_bit_code")["headers"][0]["max_lit"] == 15
    i = info_of("dyn_one_distance_code")
    assert i["headers"][0]["n_dist"] == 1 and i["headers"][0]["max_dist"] == 1 and len(i["matches"]) == 3
    h = info_of("dyn_min")["headers"][0]
    assert (h["hlit"], h["hdist"], h["n_dist"]) == (257, 1, 1)
    h = info_of("dyn_min_nodist")["headers"][0]
    assert (h["hlit"], h["hdist"], h["n_dist"]) == (257, 1, 0)
    i = info_of("dyn_max")
    assert (i["headers"][0]["hlit"], i["headers"][0]["hdist"]) == (286, 30)
    assert (28, 0) in i["lsyms"] and any(d == 29 for d, _e in i["dsyms"])
    for use in ((16,), (17,), (18,)):
        syms = info_of("dyn_repeat_%d" % use[0])["headers"][0]["cl_syms"]
        assert use[0] in syms and not (syms & ({16, 17, 18} - set(use))), use
    assert {16, 17, 18} <= info_of("dyn_repeat_16_17_18")["headers"][0]["cl_syms"]
    for name, sym in (("dyn_repeat_crossing_18", 18), ("dyn_repeat_crossing_16", 16)):
        h = info_of(name)["headers"][0]
        assert h["crossing"] and sym in h["cl_syms"], name
    assert F.rle_lengths([5] * 8 + [0] * 150) == [(5, 0), (16, 3), (5, 0), (18, 127), (18, 1)]


def test_sizes_and_layout():
    c = F.cases()
    assert [m.isize for m in c["isize_0"]] == [0, 0, 0]
    assert [m.isize for m in c["isize_1"]] == [1, 1]
    assert [m.isize for m in c["isize_65280"]] == [65280]
    assert [m.isize for m in c["isize_65536"]] == [65536, 65536]
    at, offs = 0, set()
    for m in c["layout_xlen"]:
        offs.add((at + m.payload_offset()) % 16)
        assert m.raw()[m.payload_offset():m.payload_offset() + len(m.payload)] == m.payload
        at += len(m.raw())
    assert offs == set(range(16))


ZLIB_SAYS = {
    F.EBTYPE: ["invalid block type"],
    F.ESTORED: ["invalid stored block lengths"],
    F.ETOOMANY: ["too many length or distance symbols"],
    F.ELENS: ["invalid code lengths set", "invalid literal/lengths set", "invalid distances set"],
    F.EREPEAT: ["invalid bit length repeat"],
    F.ENOEOB: ["missing end-of-block"],
    F.ESYMBOL: ["invalid literal/length code", "invalid distance code"],
    F.EDIST: ["invalid distance too far back"],
}


def test_malformed_verdicts_are_read_off_zlib():
    """Each malformed case is not ok under the statement, and for the reason it is named for: zlib's own message
    for the defects of the stream, a stream that ends early for EINPUT, a whole stream with another length or
    CRC-32 for EPAST, ESHORT and ECRC."""
    bad = F.malformed_cases()
    assert {m.code for m in bad.values()} == set(range(1, 14))   # every status code has its case
    for name, m in bad.items():
        assert m.verdict()[0] is False, name
        d = zlib.decompressobj(-15)
        if m.code in ZLIB_SAYS:
            with pytest.raises(zlib.error) as e:
                d.decompress(m.payload)
            assert any(s in str(e.value) for s in ZLIB_SAYS[m.code]), (name, str(e.value))
            continue
        text = d.decompress(m.payload)
        if m.code == F.EINPUT:
            assert not d.eof, name
        elif m.code == F.EPAST:
            assert len(text) > m.isize, name
        elif m.code == F.ESHORT:
            assert d.eof and len(text) < m.isize, name
        elif m.code == F.ECRC:
            assert d.eof and len(text) == m.isize and zlib.crc32(text) != m.crc, name
        else:
            assert m.code == F.EISIZE and d.eof and len(text) == m.isize == 65537 and zlib.crc32(text) == m.crc, name
    text, payload, cut = F.truncations()
    assert zlib.decompress(payload, -15) == text and len(cut) == len(payload) > 40
    assert not any(m.verdict()[0] for m in cut)
    assert [m.verdict()[0] for m in F.cases()["bad_between_good"]] == [True, False, True, False, True]


def test_sanitizer_run_of_the_decode_text(tmp_path):
    """tools/bgzf_inflate_asan.sh: vafc_inflate.h with a one-lane wave under ASan + UBSan in a stand-alone program,
    over every case, each payload and each text in a heap block of exactly its size.  Its status is 0 exactly
    where the statement says ok, the text is the statement's, and a case built for a code ends in that code."""
    F.write_cases(str(tmp_path))
    p = subprocess.run([os.path.join(ROOT, "tools", "bgzf_inflate_asan.sh"), str(tmp_path)], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "bgzf_inflate_asan: all clean" in p.stdout
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr
    got = {}
    for line in p.stdout.splitlines():
        f = line.split()
        if len(f) == 5 and f[0].endswith(".bgzf"):
            got[(f[0][:-5], int(f[1]))] = (int(f[2]), int(f[3]), int(f[4]))
    n = 0
    for name, ms in F.cases().items():
        for i, m in enumerate(ms):
            ok, text = m.verdict()
            status, isize, adler = got[(name, i)]
            assert (status == 0) == ok, (name, i, status)
            assert isize == m.isize
            if ok:
                assert adler == zlib.adler32(text), (name, i)
            if m.code is not None:
                assert status == m.code, (name, i, status)
            n += 1
    assert n == len(got) > 150

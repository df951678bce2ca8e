"""tests/bam_text_fixture.py without a GPU: every class holds what it is named
for, its statement yields the records of tests/test_bam.py's read_bam_py, the
decoys pass a Python restatement of the guess's rule and so does every regular
record, and the text scan itself (csrc/vafc_bam_text.h, compiled for the host
with a one-lane wave) reports what the statement says on every scan, under
AddressSanitizer and UBSan (tools/bam_text_asan.sh)."""
import os
import struct
import subprocess

import pytest

import bam_fixture as F
import bam_text_fixture as T
from conftest import ROOT

ALL = list(T.CLASSES)


def test_the_classes_of_the_issue_are_there():
    need = {"mod4_short", "mod4_long", "cut_in_head", "cut_at_start", "span_three", "no_start", "tiny_segments",
            "decoy_qual", "decoy_aux", "n_ref0", "fields", "last_cut", "irr_fit", "irr_name", "irr_l_seq", "irr_qlen",
            "irr_cg", "irr_bs8", "n_0", "n_1", "n_63", "n_64", "n_65", "n_2000"}
    assert need <= set(ALL)


@pytest.mark.parametrize("name", ALL)
def test_scans_are_well_formed(name):
    case = T.case_of(name)
    assert case.scans
    for sc, (w, plain, weighted) in zip(case.scans, T.expected(name)):
        assert 0 <= sc.entry <= len(sc.text)
        assert list(sc.cuts) == sorted(sc.cuts) and all(0 <= c <= len(sc.text) for c in sc.cuts)
        assert sc.entry <= w.consumed <= len(sc.text)
        assert plain.size == weighted.size == 2 * len(case.rows)


@pytest.mark.parametrize("name", ALL)
def test_statement_yields_the_host_readers_records(name, tmp_path):
    """A scan without an irregular record and without a short block_size: the
    regular records are those read_bam_py yields for the same text in a file."""
    from test_bam import read_bam_py
    case = T.case_of(name)
    refs = [(nm, (1 << 31) - 1) for nm in case.ref_names]
    done = set()
    for sc, (w, _p, _q) in zip(case.scans, T.expected(name)):
        key = (sc.text, sc.entry, sc.final)
        if w.irregular or w.short_stop or key in done:
            continue
        done.add(key)
        body = sc.text[sc.entry:] if sc.final else sc.text[sc.entry:w.consumed]
        path = str(tmp_path / "t.bam")
        with open(path, "wb") as f:
            f.write(F.bgzf(F.header(refs) + body, 1024))
        names, recs = read_bam_py(path)
        assert names == case.ref_names
        assert recs == w.recs
    if not name.startswith("irr_"):
        assert done


def test_mod4_meets_every_alignment():
    for name, long_ops in (("mod4_short", False), ("mod4_long", True)):
        case = T.case_of(name)
        starts, cigars = set(), set()
        for sc, (w, _p, _q) in zip(case.scans, T.expected(name)):
            for o in w.found:
                starts.add(o % 4)
                n_cigar, = struct.unpack_from("<H", sc.text, o + 16)
                if (n_cigar > 64) == long_ops and n_cigar:
                    cigars.add((o + 36 + sc.text[o + 12]) % 4)
        assert starts == {0, 1, 2, 3} and cigars == {0, 1, 2, 3}, name


def test_cut_in_head_cuts_every_leading_byte():
    case = T.case_of("cut_in_head")
    w = T.expected("cut_in_head")[0][0]
    inside = set()
    for sc in case.scans:
        for c in sc.cuts:
            o = max(f for f in w.found if f <= c)
            inside.add(c - o)
    assert inside >= set(range(1, 36))
    for sc, (w, _p, _q) in zip(T.case_of("cut_at_start").scans, T.expected("cut_at_start")):
        assert set(sc.cuts) <= set(w.found)


def test_segments_of_the_named_shapes():
    case, exp = T.case_of("span_three"), T.expected("span_three")
    for sc, (w, _p, _q) in zip(case.scans, exp):
        assert any(sum(1 for a, b in T.segments(sc) if a < o + 4 + struct.unpack_from("<i", sc.text, o)[0] and b > o) >= 3
                   for o in w.found)
    sc, (w, _p, _q) = T.case_of("no_start").scans[0], T.expected("no_start")[0]
    a, b = T.segments(sc)[1]
    assert not [o for o in w.found if a <= o < b] and T.guess(sc.text, a, b, 2) is None
    sizes = {b - a for sc in T.case_of("tiny_segments").scans for a, b in T.segments(sc)}
    assert {1, 35, 36, 37} <= sizes


@pytest.mark.parametrize("name", ["decoy_qual", "decoy_aux"])
def test_decoy_is_plausible_and_wrong(name):
    case = T.case_of(name)
    for sc, (w, _p, _q) in zip(case.scans, T.expected(name)):
        assert sc.rewalk == "some"
        wrong = 0
        for a, b in T.segments(sc):
            g = T.guess(sc.text, a, b, len(case.ref_names))
            if g is not None and g not in w.found and any(a <= o < b for o in w.found):
                # a whole chain of plausible images, none of them a record
                p = g
                for _ in range(T.CHAIN):
                    ok, nxt = T.plausible(sc.text, p, len(case.ref_names))
                    assert ok and p not in w.found
                    p = nxt
                wrong += 1
        assert wrong >= 1
        assert not w.irregular and not w.short_stop


@pytest.mark.parametrize("name", ALL)
def test_every_regular_record_is_plausible(name):
    case = T.case_of(name)
    seen = 0
    for sc, (w, _p, _q) in zip(case.scans, T.expected(name)):
        for o in w.found:
            if T.classify(sc.text, o)[0]:
                assert T.plausible(sc.text, o, len(case.ref_names))[0], (name, o)
                seen += 1
    assert seen or name == "n_0"


def test_field_classes_hold_their_fields():
    case, exp = T.case_of("fields"), T.expected("fields")
    recs = exp[0][0].recs
    assert any(r[0] == -1 for r in recs) and any(not r[3] and r[4] for r in recs) and any(r[3] and r[4] == 0 for r in recs)
    assert any(not r[3] and r[4] == 0 for r in recs) and any(r[1] == (1 << 31) - 1 for r in recs)
    assert {0x4, 0x200, 0x400} <= {r[2] for r in recs}
    assert exp[0][1].any() and (exp[0][1] != exp[0][2]).any()              # counts, and weights that change them
    top = [i for i, r in enumerate(case.rows) if r[1] >= T.ROW_MAX - 1]
    assert top and any(exp[0][1][2 * i] + exp[0][1][2 * i + 1] for i in top)
    assert T.case_of("n_ref0").ref_names == [] and all(r[0] == -1 for r in T.expected("n_ref0")[0][0].recs)


@pytest.mark.parametrize("kind", T.IRREGULAR)
def test_irregular_classes(kind):
    case, exp = T.case_of("irr_" + kind), T.expected("irr_" + kind)
    for sc, (w, _p, _q) in zip(case.scans, exp):
        if kind == "bs8":
            assert w.short_stop and not w.irregular and 0 < len(w.found) and w.consumed < len(sc.text)
            assert struct.unpack_from("<i", sc.text, w.consumed)[0] == 8
        else:
            assert not w.short_stop and w.irregular and w.consumed == len(sc.text)
            assert all(T.classify(sc.text, o) == (False, kind) for o in w.irregular)
            assert min(w.irregular) > w.found[3] and max(w.irregular) < w.found[-3]      # in the middle of good records
            assert len(w.recs) == len(w.found) - len(w.irregular)
    assert len(exp[-1][0].irregular) == (0 if kind == "bs8" else 2)


def test_last_cut_and_counts():
    case, exp = T.case_of("last_cut"), T.expected("last_cut")
    whole = max(len(sc.text) for sc in case.scans[:20])
    cut_at = set()
    for sc, (w, _p, _q) in zip(case.scans, exp):
        assert len(w.recs) == 6
        if w.consumed < len(sc.text):
            cut_at.add((len(sc.text) - w.consumed, sc.final))
    assert whole and {(j, f) for j in range(1, 53) for f in (True, False)} <= cut_at
    # the cut record whose fields do not fit: irregular as a final piece only
    assert [len(w.irregular) for w, _p, _q in exp[-6:]] == [1, 0, 1, 0, 1, 0]
    for n in T.COUNTS:
        for w, plain, _q in T.expected("n_%d" % n):
            assert len(w.recs) == len(w.found) == n and (n < 60 or plain.any())
    assert any(len(r[3]) > 64 for r in T.expected("n_2000")[0][0].recs)


def test_scan_under_the_sanitizers(tmp_path):
    """The kernels' own text on the CPU: every scan of every class through
    guess, link, emit and check, compared with the statement."""
    n = T.write_cases(str(tmp_path))
    assert n == sum(len(T.case_of(c).scans) for c in ALL) > 200
    p = subprocess.run([os.path.join(ROOT, "tools", "bam_text_asan.sh"), str(tmp_path)], capture_output=True, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    assert out.count(" ok ") == n and "bam_text_asan: all clean" in out

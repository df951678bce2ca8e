"""The device's BAM text scan (vc_bam_scan_text_*, csrc/vafc_bam.hip over
csrc/vafc_bam_text.h; needs an MI355X): every scan of every class of
tests/bam_text_fixture.py through vc_bam_scan_text_block, per long threshold,
plain and weighted, compared exactly with the statement -- counts, consumed,
records, bases, the irregular records and their lowest offset, the short stop
and the offsets' number; segments walked again at least once on the decoys and
never where every segment starts at a record start.  One class also goes
through vc_bam_scan_text_device on a side stream, and one text is scanned as a
whole and as pieces of 1 KB with the tails carried.

tests/test_bam_text_fixture.py shows without a GPU that every class holds what
it is named for and runs the same kernel text on the CPU."""
import numpy as np
import pytest

import bam_text_fixture as T
from bam_statement import make_counter

pytestmark = pytest.mark.gpu

THRESHOLDS = (0, 64, 0xFFFFFFFF)
THR_NAME = {0: "all_long", 64: "64", 0xFFFFFFFF: "never_long"}


def check_result(res, sc, w, where):
    import vafc
    want_off = min(w.irregular) if w.irregular else vafc.BAM_NO_IRREGULAR
    got = (res.consumed, res.records, res.bases, res.irregular, res.irregular_off, res.short_stop, res.found)
    want = (w.consumed, len(w.recs), w.bases, len(w.irregular), want_off, int(w.short_stop), len(w.found))
    assert got == want, "%s: (consumed, records, bases, irregular, its offset, short stop, found) %r, statement %r" % (
        where, got, want)
    if sc.rewalk == "zero":
        assert res.rewalked == 0, "%s: %d segments walked again, every one starts at a record start" % (where, res.rewalked)
    if sc.rewalk == "some":
        assert res.rewalked >= 1, "%s: no segment walked again past a decoy" % where


def first_difference(case, got, want):
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    i = int(bad[0]) // 2
    return "%d of %d counts differ, first row %d %r: counted (ref %d, alt %d), statement (ref %d, alt %d)" % (
        bad.size, got.size, i, tuple(case.rows[i]), int(got[2 * i]), int(got[2 * i + 1]), int(want[2 * i]),
        int(want[2 * i + 1]))


def set_weights(bc, case, weighted):
    regs = T.regions_of(case) if weighted else []
    bc.set_regions(*(zip(*regs) if regs else ((), (), ())))
    return bool(regs) or not weighted


@pytest.mark.parametrize("name", list(T.CLASSES))
def test_class_against_statement(name, tmp_path):
    case, exp = T.case_of(name), T.expected(name)
    bc = make_counter(case.rows, case.ref_names, tmp_path)
    try:
        for thr in THRESHOLDS:
            bc.set_long_threshold(thr)
            for weighted in (False, True):
                if not set_weights(bc, case, weighted):
                    continue                    # no reference, no region: the weights are those of the plain pass
                for i, (sc, (w, plain, wtd)) in enumerate(zip(case.scans, exp)):
                    where = "class %s (%s), scan %d, long threshold %s, %s" % (
                        name, case.note, i, THR_NAME[thr], "weighted" if weighted else "plain")
                    bc.reset()
                    bc.scan_text_block(sc.text, sc.entry, sc.cuts, sc.final)
                    check_result(bc.text_result(), sc, w, where)
                    bad = first_difference(case, bc.finish(), wtd if weighted else plain)
                    assert not bad, "%s: %s" % (where, bad)
        assert min(bc.text_kernel_ms()) > 0
    finally:
        bc.close()


def test_scan_text_device_on_a_side_stream(tmp_path):
    """Text and cuts in HBM, the scan on a torch side stream right after a
    reset on the handle's own stream, no host synchronisation in between."""
    import torch
    import vafc
    name = "mod4_long"
    case, exp = T.case_of(name), T.expected(name)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    bc = make_counter(case.rows, case.ref_names, tmp_path)
    try:
        for i, (sc, (w, plain, _q)) in enumerate(zip(case.scans, exp)):
            d_text = torch.from_numpy(np.frombuffer(sc.text, np.uint8).copy()).to(dev)
            d_cuts = torch.from_numpy(np.asarray(sc.cuts, np.int64)).to(dev)
            torch.cuda.synchronize()
            bc.scan_text_block(sc.text, sc.entry, sc.cuts, sc.final)      # the handle's stream is busy
            bc.reset()
            bc.scan_text_device(d_text.data_ptr(), len(sc.text), sc.entry, d_cuts.data_ptr() if sc.cuts else 0,
                                len(sc.cuts), sc.final, side.cuda_stream)
            check_result(bc.text_result(), sc, w, "scan %d on a side stream" % i)
            bad = first_difference(case, bc.finish(), plain)
            assert not bad, "scan %d on a side stream: %s" % (i, bad)
            bc.scan_text_device(d_text.data_ptr(), len(sc.text), sc.entry, d_cuts.data_ptr() if sc.cuts else 0,
                                len(sc.cuts), sc.final, vafc.STREAM_CTX)
            assert np.array_equal(bc.finish(), plain * np.uint32(2))
    finally:
        bc.close()


@pytest.mark.parametrize("step", [1024, 333])
def test_pieces_with_tails_equal_one_piece(step, tmp_path):
    """The text of a few thousand records as one piece, and as pieces of
    `step` more bytes each, every piece from where the one before stopped."""
    name = "n_2000"
    case = T.case_of(name)
    sc, (w, plain, _q) = case.scans[0], T.expected(name)[0]
    text = sc.text
    bc = make_counter(case.rows, case.ref_names, tmp_path)
    try:
        bc.scan_text_block(text, 0, sc.cuts, True)
        whole = bc.text_result()
        one = bc.finish()
        assert not first_difference(case, one, plain)
        bc.reset()
        start, end, records, bases, pieces = 0, 0, 0, 0, 0
        while True:
            old = end - start
            end = min(end + step, len(text))
            final = end == len(text)
            bc.scan_text_block(text[start:end], 0, [old] if 0 < old < end - start else [], final)
            res = bc.text_result()
            assert not res.irregular and not res.short_stop
            records += res.records
            bases += res.bases
            pieces += 1
            if final:
                assert res.consumed == end - start
                break
            want = T.walk_text(text[start:end], 0, False)
            assert res.consumed == want.consumed, "piece %d" % pieces
            start += res.consumed
        assert pieces > 100 and (records, bases) == (whole.records, whole.bases) == (len(w.recs), w.bases)
        bad = first_difference(case, bc.finish(), plain)
        assert not bad, "pieces of %d bytes: %s" % (step, bad)
    finally:
        bc.close()


def test_arguments(tmp_path):
    import vafc
    case = T.case_of("n_64")
    sc = case.scans[0]
    bc = make_counter(case.rows, case.ref_names, tmp_path)
    try:
        for entry, cuts in ((len(sc.text) + 1, []), (0, [50, 40]), (0, [len(sc.text) + 1])):
            with pytest.raises(vafc.VafcError) as ei:
                bc.scan_text_block(sc.text, entry, cuts, True)
            assert ei.value.code == vafc.VC_EINVAL
        bc.scan_text_block(b"", 0, [], True)
        res = bc.text_result()
        assert (res.consumed, res.records, res.found, res.irregular) == (0, 0, 0, 0)
        # the entry at the text's end: nothing to find, nothing consumed past it
        bc.scan_text_block(sc.text, len(sc.text), [10, 20], False)
        res = bc.text_result()
        assert (res.consumed, res.records, res.found) == (len(sc.text), 0, 0)
        assert not bc.finish().any()
    finally:
        bc.close()

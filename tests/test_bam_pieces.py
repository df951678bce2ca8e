"""The device's piece walk (vc_bam_scan_pieces_*, csrc/vafc_bam.hip over
vbt_piece_walk of csrc/vafc_bam_text.h; needs an MI355X): every class of
tests/bam_seek_fixture.py through vc_bam_scan_pieces_block, per long
threshold, plain and weighted, compared exactly with the serial statement --
per piece its status, its records' offsets and the missing bytes of a cut one,
in total the records, bases, irregular records and counts.  One class also goes
through vc_bam_scan_pieces_device on a side stream; pieces that overlap until
their records outnumber the room end NOROOM and emit nothing.

tests/test_bam_seek_plan.py shows without a GPU that every class holds what it
is named for and runs the same walk on the CPU under the sanitizers."""
import numpy as np
import pytest

import bam_seek_fixture as S
from bam_statement import make_counter

pytestmark = pytest.mark.gpu

THRESHOLDS = (0, 64, 0xFFFFFFFF)


def check(bc, case, want, where):
    import vafc
    res, status, offs = bc.pieces_result()
    assert res.n_pieces == len(case.pieces) == status.size, where
    for i, (st, found, missing) in enumerate(want.per_piece):
        got = status[i]
        assert (int(got["status"]), int(got["found"]), int(got["missing"])) == (st, len(found), missing), \
            "%s: piece %d %r" % (where, i, case.pieces[i])
        if st == S.OK and found:
            first = int(got["first"])
            assert offs[first:first + len(found)].tolist() == found, "%s: piece %d %r" % (where, i, case.pieces[i])
    assert sorted(offs.tolist()) == sorted(want.emitted), where
    want_off = min(want.irregular) if want.irregular else vafc.BAM_NO_IRREGULAR
    got = (res.records, res.bases, res.found, res.irregular, res.irregular_off, res.n_short, res.n_cut, res.n_noroom)
    assert got == (len(want.recs), want.bases, len(want.emitted), len(want.irregular), want_off, want.n_short, want.n_cut,
                   0), where


@pytest.mark.parametrize("name", list(S.CLASSES))
def test_class_against_statement(name, tmp_path):
    import bam_text_fixture as T
    case, want = S.case_of(name), S.want_of(name)
    regs = T.regions_of(T.Case(case.rows, case.ref_names, [], ""))
    bc = make_counter(case.rows, case.ref_names, tmp_path)
    try:
        for thr in THRESHOLDS:
            bc.set_long_threshold(thr)
            for weighted in (False, True):
                bc.set_regions(*(zip(*regs) if weighted else ((), (), ())))
                where = "class %s (%s), long threshold %#x, %s" % (name, case.note, thr, "weighted" if weighted else "plain")
                bc.reset()
                bc.scan_pieces_block(case.text, case.pieces)
                check(bc, case, want, where)
                got, exp = bc.finish(), want.weighted if weighted else want.plain
                assert np.array_equal(got, exp), "%s: rows %r differ" % (where, np.nonzero(got != exp)[0][:8] // 2)
        find, chk = bc.text_kernel_ms()
        assert find > 0 and chk > 0
    finally:
        bc.close()


def test_scan_pieces_device_on_a_side_stream(tmp_path):
    """Text and pieces in HBM, the scan on a torch side stream right after a
    reset on the handle's own stream, no host synchronisation in between."""
    import torch
    import vafc
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    for name in ("n_200", "long"):
        case, want = S.case_of(name), S.want_of(name)
        bc = make_counter(case.rows, case.ref_names, tmp_path)
        try:
            d_text = torch.from_numpy(np.frombuffer(case.text, np.uint8).copy()).to(dev)
            pieces = vafc._bam_pieces(case.pieces)
            d_pieces = torch.from_numpy(pieces.view(np.int64).copy()).to(dev)
            torch.cuda.synchronize()
            bc.scan_pieces_block(case.text, case.pieces)                  # the handle's stream is busy
            bc.reset()
            bc.scan_pieces_device(d_text.data_ptr(), len(case.text), d_pieces.data_ptr(), len(case.pieces), side.cuda_stream)
            check(bc, case, want, "%s on a side stream" % name)
            assert np.array_equal(bc.finish(), want.plain)
            bc.scan_pieces_device(d_text.data_ptr(), len(case.text), d_pieces.data_ptr(), len(case.pieces), vafc.STREAM_CTX)
            assert np.array_equal(bc.finish(), want.plain * np.uint32(2))
        finally:
            bc.close()


def test_overlapping_pieces_never_outgrow_the_list(tmp_path):
    """Records of 36 to 40 bytes, every piece over all of them: the pieces
    that find no room emit nothing, and what is counted is a whole number of
    walks of the text."""
    import bam_fixture as F
    recs = [F.record(0, 10 + i, 0, [], "", name=b"abc") for i in range(400)]
    assert all(len(r) == 40 for r in recs)
    text = b"".join(recs)
    room = len(text) // 36 + 1
    case = S.PieceCase(S.T.dense_rows(), S.T.NAMES, text, [(0, len(text), len(text))] * 70, "")
    bc = make_counter(case.rows, case.ref_names, tmp_path)
    try:
        bc.scan_pieces_block(case.text, case.pieces)
        res, status, offs = bc.pieces_result()
        ok = int((status["status"] == S.OK).sum())
        assert ok == room // 400 == 1 and res.n_noroom == 70 - ok
        assert set(status["status"].tolist()) == {S.OK, S.NOROOM} and (status["found"] == 400).all()
        assert res.found == res.records == 400 * ok and sorted(offs.tolist()) == list(range(0, len(text), 40))
    finally:
        bc.close()


def test_arguments(tmp_path):
    import vafc
    case = S.case_of("n_64")
    bc = make_counter(case.rows, case.ref_names, tmp_path)
    try:
        bc.scan_pieces_block(b"", [])
        res, status, offs = bc.pieces_result()
        assert (res.n_pieces, res.found, res.records, status.size, offs.size) == (0, 0, 0, 0, 0)
        bc.scan_pieces_block(b"", [(0, 10, 10), (5, 2, 1)])
        res, status, offs = bc.pieces_result()
        assert res.n_pieces == 2 and res.found == 0 and (status["status"] == S.OK).all()
        with pytest.raises(vafc.VafcError) as ei:
            bc.scan_pieces_device(0, 10, 0, 1)
        assert ei.value.code == vafc.VC_EINVAL
        with pytest.raises(vafc.VafcError) as ei:
            bc.scan_pieces_device(0, 0, 12, 1)                            # pieces off an 8-byte boundary
        assert ei.value.code == vafc.VC_EINVAL
        assert not bc.finish().any()
    finally:
        bc.close()

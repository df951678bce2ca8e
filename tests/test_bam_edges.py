"""The two bam kernels (csrc/vafc_bam.hip) at their edges (needs an MI355X):
the classes of tests/bam_edges_fixture.py -- more long records than the long
kernel has waves, base indices past l_seq, zero-length operations, rows and
walks at the end of the position range, tids past 16 bits beside references
without rows, regions that touch a record, descriptors that end at and just
past the data -- each counted alone, per long threshold, plain and weighted,
and compared exactly with the statement (tests/bam_statement.py).  A failure
names the class, the threshold, the pass, the batch and the first wrong row.

tests/test_bam_edges_fixture.py shows without a GPU that every class tells
the faulty walks it is meant for from the right one."""
import pytest

import bam_edges_fixture as E
from bam_statement import count_records, pack

pytestmark = pytest.mark.gpu

CASES = [(name, thr) for name in E.CLASSES for thr in E.thresholds_of(name)]
THR_NAME = {0: "all_long", 64: "64", E.NEVER_LONG: "never_long"}


def _n_cu() -> int:
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _odd_cut(n: int) -> int:
    return (n // 2) | 1


@pytest.mark.parametrize("name,thr", CASES, ids=["%s-%s" % (n, THR_NAME[t]) for n, t in CASES])
def test_class_against_statement(name, thr, tmp_path):
    n_cu = _n_cu()
    case = E.case_of(name, n_cu)
    st = E.statement(name, n_cu)
    recs, data = pack(case.recs)
    bc = E.make_counter(case, tmp_path)      # one counter per class: its tids come from the class's names
    try:
        bc.set_long_threshold(thr)
        for weighted in (False, True):
            bc.set_regions(*(zip(*case.regions) if weighted else ((), (), ())))
            for n in E.batches_of(name, case, n_cu):
                want = st.counts(n, weighted)
                cuts = [(n,)] + ([(_odd_cut(n), n)] if name in E.SPLIT and n > 1 else [])
                for cut in cuts:
                    bc.reset()
                    at = 0
                    for end in cut:
                        bc.count_block(recs[at:end], data)
                        at = end
                    bad = E.first_difference(case, bc.finish(), want)
                    if bad:
                        pytest.fail("class %s (%s), long threshold %s, %s, %d records in %d batch(es): %s" % (
                            name, case.note, THR_NAME[thr], "weighted" if weighted else "plain", n, len(cut), bad))
    finally:
        bc.close()


@pytest.mark.parametrize("thr", E.THRESHOLDS, ids=[THR_NAME[t] for t in E.THRESHOLDS])
def test_descriptor_bounds(thr, tmp_path):
    """Class B: a descriptor whose CIGAR and bases end exactly where the data
    ends is followed and counted; one byte, one word or one offset further, or
    off a 4-byte boundary, it is reported by finish() and the handle counts
    again after reset()."""
    import vafc
    case = E.class_B()
    row_tid = E.row_tids(case)
    good = count_records(case.rows, row_tid, case.recs)
    assert good.any()
    bc = E.make_counter(case, tmp_path)
    try:
        bc.set_long_threshold(thr)
        for what, recs, data, accepted, counted in E.b_probes():
            bc.reset()
            bc.count_block(recs, data)
            if accepted:
                bad = E.first_difference(case, bc.finish(), count_records(case.rows, row_tid, counted))
                assert not bad, "class B, long threshold %s, %s: %s" % (THR_NAME[thr], what, bad)
            else:
                with pytest.raises(vafc.VafcError) as ei:
                    bc.finish()
                assert ei.value.code == vafc.VC_EINVAL, what
            bc.reset()
            bc.count_block(*pack(case.recs))
            bad = E.first_difference(case, bc.finish(), good)
            assert not bad, "class B, long threshold %s, after %s and reset: %s" % (THR_NAME[thr], what, bad)
    finally:
        bc.close()

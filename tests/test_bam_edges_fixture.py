"""The bam edge fixture (tests/bam_edges_fixture.py) on the CPU alone: every
class holds what it is named for, the statement's counts of every class equal
a second, plainer restatement and the fault-free kernel model, and differ from
what the named faulty kernels would count.  A class that a faulty walk cannot
tell from the right one would prove nothing on the GPU."""
import time

import numpy as np
import pytest

import bam_edges_fixture as E
import bam_fixture as F
from bam_statement import MATCH_OPS, REF_OPS, rec_end

N_CU = 256
_SPENT = [0.0]


@pytest.fixture(autouse=True)
def _timed():
    t0 = time.perf_counter()
    yield
    _SPENT[0] += time.perf_counter() - t0

# the faults every class must tell from the shipped kernel
MUST_DIFFER = {"no_l_seq_guard": "Q", "pos_32_bits": "PT", "key_shift_32": "PT", "weight_e_ge_pos": "W",
               "weight_s_le_end": "W", "zero_covers": "Z", "stride_dropped": "S", "stale_rp": "S", "stale_cur": "S"}


def _want(name, n, weighted):
    return E.statement(name, N_CU).counts(n, weighted)


def _full(name):
    return len(E.case_of(name, N_CU).recs)


# ---------------------------------------------------------------------------
# the statement three ways
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(E.CLASSES))
def test_statement_equals_count_records_outright(name):
    """Statement hands count_records a window of rows and regions; on the
    classes small enough, count_records over everything says the same."""
    from bam_statement import count_records
    case = E.case_of(name, N_CU)
    n = min(len(case.recs), 300)
    for weighted in (False, True):
        want = count_records(case.rows, E.row_tids(case), case.recs[:n], case.regions if weighted else None)
        assert np.array_equal(_want(name, n, weighted), want), (name, weighted)


@pytest.mark.parametrize("name", sorted(E.CLASSES))
def test_statement_equals_the_expansion_and_the_model(name):
    case = E.case_of(name, N_CU)
    for n in E.batches_of(name, case, N_CU)[-2:]:
        for weighted in (False, True):
            want = _want(name, n, weighted)
            model = E.model_counts(case, n, weighted, None, N_CU)
            assert np.array_equal(model, want), (name, n, weighted, E.first_difference(case, model, want))
            plain, left_out = E.expanded_counts(case, n, weighted)
            # the gigabase walks are not expanded: the model above has checked them, at their few rows
            assert len(left_out) == {"P": 8, "T": 6}.get(name, 0)
            if left_out:
                rest = E.Case(case.rows, case.ref_names, [r for i, r in enumerate(case.recs) if i not in left_out],
                              case.regions, case.note)
                want = E.Statement(rest).counts(len(rest.recs), weighted)
            assert np.array_equal(plain, want), (name, n, weighted, E.first_difference(case, plain, want))


@pytest.mark.parametrize("name", sorted(E.CLASSES))
def test_every_class_counts_and_its_weights_matter(name):
    case = E.case_of(name, N_CU)
    for n in E.batches_of(name, case, N_CU):
        plain, weighted = _want(name, n, False), _want(name, n, True)
        assert plain.any(), (name, n)
        if n >= 4:              # S: the first three records lie outside all regions
            assert weighted.any() and not np.array_equal(plain, weighted), (name, n)


# ---------------------------------------------------------------------------
# the faults
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("fault", E.FAULTS)
def test_fault_changes_the_counts_of_its_classes(fault):
    for name in MUST_DIFFER[fault]:
        case = E.case_of(name, N_CU)
        n = _full(name)
        passes = (True,) if fault.startswith("weight_") else (False, True)
        for weighted in passes:
            got = E.model_counts(case, n, weighted, fault, N_CU)
            assert not np.array_equal(got, _want(name, n, weighted)), (fault, name, weighted)


def test_stride_faults_need_the_second_trip():
    """At 8 * n_cu records every wave has one record and the faults of the loop
    are silent; one record more shows them."""
    case = E.case_of("S", N_CU)
    for fault in ("stride_dropped", "stale_rp", "stale_cur"):
        for weighted in (False, True):
            at, over = 8 * N_CU, 8 * N_CU + 1
            assert np.array_equal(E.model_counts(case, at, weighted, fault, N_CU), _want("S", at, weighted))
            if weighted and fault != "stride_dropped":
                over = E.s_batches(N_CU)[-1]     # record 0 weighs 0 and leaves wave 0 nothing stale: other waves show it
            assert not np.array_equal(E.model_counts(case, over, weighted, fault, N_CU), _want("S", over, weighted))
    # the record that shares wave 0 with the first one is no 5th and no 7th record: it counts, after a 7th
    assert (8 * N_CU) % 5 and (8 * N_CU) % 7 and len(case.recs[0][3]) == 5


def test_which_classes_each_fault_reaches():
    """The whole table, for the record: a fault outside its classes may or may
    not show; inside them it must."""
    table = {}
    for fault in E.FAULTS:
        if fault == "no_l_seq_guard":
            continue            # outside Q its base indices leave the record's bytes
        for name in sorted(E.CLASSES):
            case = E.case_of(name, N_CU)
            n = _full(name)
            hit = any(not np.array_equal(E.model_counts(case, n, w, fault, N_CU), _want(name, n, w)) for w in (False, True))
            table.setdefault(fault, "")
            table[fault] += name if hit else ""
    print(table)
    for fault, names in table.items():
        assert set(MUST_DIFFER[fault]) <= set(names), (fault, names)


# ---------------------------------------------------------------------------
# the classes hold what they are named for
# ---------------------------------------------------------------------------

def test_class_s():
    case = E.case_of("S", N_CU)
    assert E.s_batches(N_CU) == (1, 2, 3, 4, 5, 2047, 2048, 2049, 4103) and len(case.recs) == 4103
    assert all(b[1] - a[1] == 2 for a, b in zip(case.rows, case.rows[1:]))
    plain = _want("S", 4103, False).reshape(-1, 2)
    assert (plain.sum(axis=1) == 1).all() and plain[:, 0].sum() > 1000 and plain[:, 1].sum() > 1000
    weights = [sum(v for _k, v in part) for part in E.statement("S", N_CU).parts(True)]
    assert all(w == 0 for w in weights[::5]) and set(weights) == {0, 1, 2, 3}
    assert all((len(r[3]) == 5) == (i % 7 == 0) and r[4] == (8 if i % 7 == 0 else 1) for i, r in enumerate(case.recs))
    # the long list's launch: blocks of four waves, never more than 8 * n_cu waves
    for n in E.s_batches(N_CU):
        waves = 4 * min(2 * N_CU, (n + 3) // 4)
        assert (waves < n) == (n > 8 * N_CU)


def test_class_q():
    case = E.case_of("Q")
    assert [r[4] for r in case.recs] == [10, 9, 8, 1, 0, 14, 13, 12, 1, 0]
    rows_at = {r[1]: r for r in case.rows}
    for rec in case.recs:
        full = F.query_len([(F.OPS[w & 15], w >> 4) for w in rec[3]])
        assert len(rec[5]) == (full + 1) // 2                      # the whole query stays in the data
        blocks = E.match_blocks(rec[1], [(F.OPS[w & 15], w >> 4) for w in rec[3]])
        assert all(p in rows_at for s, n in blocks for p in range(s, s + n))
    counts = _want("Q", 10, False).reshape(-1, 2)
    assert counts[:, 1].sum() == 0 and counts[:, 0].sum() == 10 + 9 + 8 + 1 + 0 + 9 + 8 + 7 + 0 + 0
    # without the guard, every base behind l_seq is a letter that counts
    loose = E.model_counts(case, 10, False, "no_l_seq_guard").reshape(-1, 2)
    assert loose[:, 0].sum() == 5 * 10 + 5 * 9 and loose[:, 1].sum() == 0


def test_class_z():
    case = E.case_of("Z")
    zero_ops = {w & 15 for r in case.recs for w in r[3] if w >> 4 == 0}
    assert zero_ops == {0, 1, 2, 3, 4, 7, 8}
    places = {"head": 0, "inside": 0, "tail": 0}
    for r in case.recs[:21]:
        z = [i for i, w in enumerate(r[3]) if w >> 4 == 0]
        assert len(z) == 1
        places["head" if z[0] == 0 else "tail" if z[0] == len(r[3]) - 1 else "inside"] += 1
    assert places == {"head": 7, "inside": 7, "tail": 7}
    none, long = case.recs[21], case.recs[22]
    assert rec_end(none) == none[1] + 1 and any((w & 15) in MATCH_OPS for w in none[3])
    assert len(long[3]) == 130 and [long[3][i] >> 4 for i in (63, 64, 127, 128)] == [0] * 4
    assert (long[3][63] & 15) in MATCH_OPS and (long[3][64] & 15) in MATCH_OPS
    # the long record alone shows the fault: it is the one record that threshold 64 leaves to the long kernel
    only = E.Case(case.rows, case.ref_names, [long], case.regions, "")
    assert not np.array_equal(E.model_counts(only, 1, False, "zero_covers"), E.Statement(only).counts(1, False))
    rows_at = {r[1] for r in case.rows}
    for r in case.recs:                # a row at the position every zero-length operation sits on
        cur = r[1]
        for w in r[3]:
            if w >> 4 == 0:
                assert cur in rows_at
            if (w & 15) in REF_OPS:
                cur += w >> 4


def test_class_p():
    case = E.case_of("P")
    pos = {(r[0], r[1]) for r in case.rows}
    for chr_ in case.ref_names:
        assert {(chr_, E.ROW_MAX), (chr_, E.ROW_MAX - 1), (chr_, E.ROW_MAX - 64), (chr_, 0), (chr_, 1)} <= pos
    assert ("chrB", -1) in pos and max(p for _c, p in pos) == E.ROW_MAX == (1 << 31) - 2
    ends = [rec_end(r) for r in case.recs]
    assert sum(e > 1 << 31 for e in ends) >= 8 and sum(e > 1 << 32 for e in ends) == 4
    assert {r[1] for r in case.recs if r[1] < 0} == {-5, -4, -3, -2, -1}
    assert sorted(len(r[3]) for r in case.recs if len(r[3]) > 1) == [17, 17, 35, 35, 70, 70, 70, 70]
    # rows under the first, the seventh and the eighth block of the walk from 100, and they count
    counts = _want("P", len(case.recs), False).reshape(-1, 2).sum(axis=1)
    by_pos = {(r[0], r[1]): int(c) for r, c in zip(case.rows, counts)}
    step = (1 << 28) + 2
    for k in (0, 6, 7):
        assert by_pos[("chrA", 100 + k * step)] == 2           # the 17- and a 70-operation walk
        assert by_pos[("chrB", 100 + k * step)] == 2           # the 35-operation walk and the 17 padded to 70
    assert by_pos[("chrA", E.ROW_MAX)] >= 2 and by_pos[("chrA", 132)] == 0 and by_pos[("chrB", -1)] == 5


def test_class_t():
    case = E.case_of("T")
    assert len(case.ref_names) == 70000
    tids = sorted({int(r[0][1:]) for r in case.rows})
    assert tids == [0, 1, 40000, 65535, 65536, 69999]
    pos = {(int(r[0][1:]), r[1]) for r in case.rows}
    for t in (0, 65535):
        assert (t, E.ROW_MAX) in pos and (t + 1, 0) in pos
    rec_tids = {r[0] for r in case.recs}
    assert set(E.T_EMPTY) <= rec_tids and not set(E.T_EMPTY) & set(tids)
    assert all(any(t > e for t in tids) and any(t < e for t in tids) for e in E.T_EMPTY)
    last = case.recs[-1]
    assert (last[0], last[1]) == (69999, (1 << 31) - 1) and last[1] > max(p for t, p in pos if t == 69999)
    assert all(any(r[0] == t and rec_end(r) > 1 << 31 for r in case.recs) for t in tids)
    assert all(any(r[0] == t and r[1] == -3 for r in case.recs) for t in (1, 65536))
    regs = set(case.regions)
    for t in (0, 65535):
        assert {(t, (1 << 31) - 3, (1 << 31) - 1), (t + 1, 0, 1)} <= regs
    assert any(t not in rec_tids for t, _s, _e in regs)


def test_class_w():
    case = E.case_of("W")
    plain, weighted = _want("W", len(case.recs), False), _want("W", len(case.recs), True)
    lists = E.w_lists()
    assert [w for _what, _r, w in lists] == [0, 1, 1, 0, 1, 1, 3, 2, 0, 4, 5, 2]
    for i, (what, _regs, w) in enumerate(lists):
        assert int(plain[2 * i]) == 1 and int(weighted[2 * i]) == w, what
    zero = case.recs[-1]
    assert rec_end(zero) == zero[1] + 1 and (0, zero[1], zero[1] + 1) in case.regions


def test_class_b():
    from bam_statement import count_records
    case = E.class_B()
    probes = E.b_probes()
    assert [ok for _w, _r, _d, ok, _c in probes] == [True, True, True, False, False, False, False, False]
    for what, recs, data, ok, counted in probes:
        p, n = recs[3], data.size
        assert len(recs) == 5 and int(recs[4]["flag"]) == 0x4 and n - int(recs[4]["off"]) == E.B_TAIL
        off = int(p["off"])
        fits = off % 4 == 0 and off <= n and E.b_need(p) <= n - off          # bam_in_bounds
        assert fits == ok, what
        if ok:
            assert count_records(case.rows, E.row_tids(case), counted).any()
    need = {what: E.b_need(r[3]) - (d.size - int(r[3]["off"])) for what, r, d, _ok, _c in probes}
    assert need["need == data_bytes - off"] == need["need == data_bytes - off, odd l_seq"] == 0
    assert need["l_seq one byte over"] == 1 and need["n_cigar one word over"] == 4
    assert len(case.recs) == 3 and sorted(len(r[3]) for r in case.recs) == [1, 4, 69]


def test_the_file_is_quick():
    """Last in the file: what the tests above took together."""
    print("bam edge fixture: %.1f s" % _SPENT[0])
    assert _SPENT[0] < 30

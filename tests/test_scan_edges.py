"""The k-mer scan kernels (csrc/vafc_scan.h) window by window at every chunk
edge (needs an MI355X): the classes of tests/scan_fixture.py -- whole waves of
equal length for every trip count and tail length, one invalid byte at every
position of a chunk, a quad and a tail, defects around the long-read kernel's
segment borders -- counted in one launch and compared key by key with the
oracle's multiplicities.  Every key is a k-mer of the reads, so a window that
is looked up wrongly, skipped or counted twice changes a count.

On a mismatch the classes are recounted one by one (reset() between them) and
the first failing class is named with its tag: length, byte, position."""
import os
import re

import numpy as np
import pytest

from conftest import PKG
import scan_fixture as F

pytestmark = pytest.mark.gpu


def _define(name):
    with open(os.path.join(PKG, "csrc", "vafc_common.h")) as f:
        return int(re.search(r"#define %s (\d+)u?\b" % name, f.read()).group(1))


BIG_FILTER_BYTES = 4 * _define("VC_BIG_FILTER_WORDS")
FLANK_FILTER_BYTES = 4 << (2 * _define("VC_FLANK_BASES") - 5)
FLANK_MIN_K = _define("VC_FLANK_MIN_K")


def _counter(s, monkeypatch, filt=None, variant=None):
    """A counter for the set's keys; VAFC_FILTER and VAFC_VARIANT are read when
    the counter is made."""
    import vafc
    for name, v in (("VAFC_FILTER", filt), ("VAFC_VARIANT", variant)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    return vafc.KmerMap(s.k, s.keys, s.vals, s.n_pat, 0)


def _count_block(m, seq, offs, lens):
    m.count_block(seq, offs, lens)


def _first_failing_class(s, m, submit):
    """Failure path only: every class counted alone against the oracle."""
    import oracle as O
    orc = O.Oracle(s.k, keys=s.keys, vals=s.vals)
    for i, c in enumerate(s.classes):
        seq, offs, lens = F.class_slice(s, i)
        want, km_want = orc.count_reads(seq, offs, lens, n_patterns=s.n_pat)
        m.reset()
        submit(m, seq, offs, lens)
        got, km = m.finish()
        if km != km_want or not np.array_equal(got, want):
            return ("first failing class: #%d %s %r (reads %d..%d): tally %d, oracle %d; %d keys differ"
                    % (i, c.name, c.tag, s.spans[i][0], s.spans[i][1] - 1, km, km_want, int((got != want).sum())))
    return "no class fails when counted alone"


def _check(s, m, got, km, submit=_count_block, what=""):
    if km == s.tally and np.array_equal(got, s.want):
        return
    head = "%s k=%d: tally %d, oracle %d; %d of %d keys differ" % (
        what, s.k, km, s.tally, int((got != s.want).sum()), s.keys.size)
    pytest.fail(head + "; " + _first_failing_class(s, m, submit))


def _count_and_check(s, m, what=""):
    m.count_block(s.seq, s.offs, s.lens)
    got, km = m.finish()
    _check(s, m, got, km, what=what)
    return got


def _kinds(k):
    return ["bloom"] + (["flank"] if k >= FLANK_MIN_K else []) + ["large"]


@pytest.mark.parametrize("k,kind", [(k, kind) for k in range(16, 32) for kind in _kinds(k)])
def test_packed_kernels_every_class(k, kind, monkeypatch):
    """Every k of the packed scan, in every kernel kind built for it: the
    Bloom filter, the flank bitmap (k >= 21), and a table past
    VC_L2F_MIN_KEYS -- the large-panel kernel for k >= 21 (its 144 KiB filter
    shows that it ran), the second-level filter below."""
    s = F.scan_set(k, large=kind == "large")
    m = _counter(s, monkeypatch, None if kind == "large" else kind)
    try:
        info = m.table_info()
        assert info["n_keys"] == s.keys.size
        if kind == "large":
            assert info["n_keys"] > F.L2F_MIN_KEYS
            if k >= FLANK_MIN_K:
                assert info["filter_bytes"] == BIG_FILTER_BYTES
        elif kind == "flank":
            assert info["filter_bytes"] == FLANK_FILTER_BYTES
        else:
            assert info["filter_bytes"] < FLANK_FILTER_BYTES
        _count_and_check(s, m, kind)
    finally:
        m.close()


@pytest.mark.parametrize("k", [1, 5, 9, 15])
def test_run_time_k_kernel_every_class(k, monkeypatch):
    """The rolling scan (k < 16), whole reads and long-read segments."""
    s = F.scan_set(k)
    m = _counter(s, monkeypatch)
    try:
        _count_and_check(s, m)
    finally:
        m.close()


@pytest.mark.parametrize("k,filt", [(17, "bloom"), (18, "bloom"), (21, "bloom"), (21, "flank"), (31, "bloom"),
                                    (31, "flank")])
def test_variant_switches_count_the_same(k, filt, monkeypatch):
    """$VAFC_VARIANT 1 (no peeled chunk 0), 2 (no chunk-1 skip), 4 (no half last
    chunk) and 7 (none of them) are shipped branches: the same counts as
    variant 0 and the oracle."""
    s = F.scan_set(k)
    base = None
    for variant in (0, 1, 2, 4, 7):
        m = _counter(s, monkeypatch, filt, variant)
        try:
            got = _count_and_check(s, m, "%s variant %d" % (filt, variant))
        finally:
            m.close()
        base = got if base is None else base
        assert np.array_equal(got, base), variant


@pytest.mark.parametrize("slack", [0, 4096], ids=["tight", "slack"])
@pytest.mark.parametrize("k,filt", [(16, "bloom"), (21, "bloom"), (21, "flank")])
def test_device_resident_class_a(k, filt, slack, monkeypatch):
    """count_device on class A in a torch buffer at byte misalignments 0..3.
    tight: seq_bytes ends with the last byte of the last and longest read, so
    the last waves take the clamped loads; slack: 4 KiB of filler behind the
    reads, so every wave takes the unclamped (SAFE) loads."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dev = torch.device("cuda", 0)
    s = F.scan_set_a(k)
    m = _counter(s, monkeypatch, filt)

    def submit_at(mis):
        def submit(m, seq, offs, lens):
            buf = torch.full((mis + seq.size + slack,), 0x4E, dtype=torch.uint8, device=dev)
            buf[mis:mis + seq.size] = torch.from_numpy(np.ascontiguousarray(seq)).to(dev)
            d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
            d_lens = torch.from_numpy(lens.astype(np.int32)).to(dev)
            torch.cuda.synchronize()
            m.count_device(buf.data_ptr() + mis, seq.size + slack, d_offs.data_ptr(), d_lens.data_ptr(), lens.size)
            torch.cuda.synchronize()
            m.keep = (buf, d_offs, d_lens)    # alive until finish()
        return submit

    try:
        for mis in range(4):
            m.reset()
            submit_at(mis)(m, s.seq, s.offs, s.lens)
            got, km = m.finish()
            _check(s, m, got, km, submit_at(mis), "%s misalignment %d" % (filt, mis))
    finally:
        m.close()


# ---------------------------------------------------------------------------
# seq_nt4 mode
# ---------------------------------------------------------------------------

_NT4 = {}


def _nt4_expect(k):
    if k not in _NT4:
        classes = F.nt4_classes()
        keys, mult, tally = F.nt4_kmers(k, F.padded_reads(classes))
        allk = np.concatenate([keys, F.absent_keys(k, keys, 500)])
        want = np.concatenate([mult, np.zeros(500, np.int64)]).astype(np.uint32)
        _NT4.clear()
        _NT4[k] = (classes, allk, want)
    return _NT4[k]


def _nt4_class_counts(k, c, allk):
    keys, mult, _ = F.nt4_kmers(k, c.reads)
    want = np.zeros(allk.size, np.uint32)
    order = np.argsort(allk)
    want[order[np.searchsorted(allk[order], keys)]] = mult
    return want


@pytest.mark.parametrize("k,filt", [(17, "bloom"), (21, "bloom"), (21, "flank"), (31, "bloom"), (31, "flank")])
def test_seq_nt4_mode_equal_short_reads(k, filt, monkeypatch):
    """count_candidate_kmers (every byte through seq_nt4_table) on waves of
    equal short reads: class A up to 120 bases, one bad byte at every position
    of a 40-base read (one read per lane, and whole waves), and the tail
    classes, against the fixture's restatement of the rolling k-mer."""
    import vafc
    classes, allk, want = _nt4_expect(k)
    assert int(want.astype(np.int64).sum()) > 100_000
    monkeypatch.setenv("VAFC_FILTER", filt)
    monkeypatch.delenv("VAFC_VARIANT", raising=False)
    got = vafc.count_candidate_kmers(k, F.padded_reads(classes), allk)
    if np.array_equal(got, want):
        return
    head = "%s k=%d: %d of %d keys differ" % (filt, k, int((got != want).sum()), allk.size)
    for i, c in enumerate(classes):
        g = vafc.count_candidate_kmers(k, F.padded_reads([c]), allk)
        w = _nt4_class_counts(k, c, allk)
        if not np.array_equal(g, w):
            pytest.fail("%s; first failing class: #%d %s %r: %d keys differ"
                        % (head, i, c.name, c.tag, int((g != w).sum())))
    pytest.fail(head + "; no class fails when counted alone")

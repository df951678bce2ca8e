"""What the five kinds of device handle (KmerMap, KmerHistogram, EdCounter,
BamCounter, VcfMatcher) and the one-shot correlation share around their
kernels: the kernel timer, the device lists that grow between batches, creation
and destruction, and a launch on a caller's stream.  KmerMap and KmerHistogram
are the two kinds of one read counter (vc_ctx): each refuses the other's calls,
and both go through the same file reader.

The long-read list of KmerMap starts at 2^30 / 16385 + 1 entries and cannot be
made to grow at a test-sized shape: its regrow path (ensure_long_cap in
vafc_host.cpp) is checked by reading, not here."""
import math

import numpy as np
import pytest

import bam_fixture as BF
import vcf_fixture as VF
from test_kc import oracle_reads

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)

# --- one tiny block per handle kind --------------------------------------------

QUERY = b"ACGTTGCAAGGCTTAACCGTA"                       # 21 bases
READS = [b"TTGACCATG" + QUERY + b"GGATCCATTC", b"C" * 40, QUERY + b"A" * 19, b"GATTACAGATTACAGATTAC" + QUERY[:20]]
VCF_ROWS = VF.load_patterns(VF.panel_text().encode())
VCF_TEXT = b"chr1\t100\t.\tA\tC\t.\tx\nchr1\t1000\t.\tA\tC\t.\ty\nchrX\t1\t.\tA\tC\t.\tz\n"
BAM_ROWS = [("chr1", 10, "A", "C"), ("chr1", 11, "C", "A")]


def pack_reads(reads):
    lens = np.array([len(r) for r in reads], np.uint32)
    offs = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    return np.frombuffer(b"".join(reads) + b"N", np.uint8), offs, lens


def canonical(kmer: bytes) -> int:
    fw = rc = 0
    for ch in kmer:
        c = b"ACGT".index(ch)
        fw = fw << 2 | c
        rc = rc >> 2 | (3 - c) << 2 * (len(kmer) - 1)
    return min(fw, rc)


def pack_bam(recs):
    import struct
    import vafc
    out = np.zeros(len(recs), vafc.BAM_REC)
    data = bytearray()
    for i, (tid, pos, flag, words, l_seq, seq) in enumerate(recs):
        out[i] = (tid, pos, flag, len(words), l_seq, 0, len(data))
        data += struct.pack("<%dI" % len(words), *words) + seq
        data += b"\0" * (-len(data) % 4)
    return out, np.frombuffer(bytes(data), np.uint8)


def bam_counter(rows, names, tmp_path):
    import vafc
    path = str(tmp_path / "rows.txt")
    with open(path, "w") as f:
        for i, (c, p, ref, alt) in enumerate(rows):
            f.write("%s\t%d\t%d\trs%d\t%s\t%s\tACGTACGTACGTACGTACGTA\tACGTACGTACCTACGTACGTA\n" % (c, p, p + 1, i, ref, alt))
    db = vafc.load_patterns(path)
    assert db.n == len(rows)
    return vafc.BamCounter(db, names)


def kc_result(h):
    h.finish()
    hist, distinct, kmers = h.histogram()
    return hist.tolist(), distinct, kmers


class Kind:
    """create() -> handle; block(h) queues the tiny block; result(h) finishes."""

    def __init__(self, create, block, result):
        self.create, self.block, self.result = create, block, result


def kinds(tmp_path):
    import vafc
    bam_block = pack_bam([(0, 9, 0, BF.cigar_words([("M", 4)]), 4, bytes([0x12, 0x12]))] * 4)
    return {
        "kmer": Kind(lambda: vafc.KmerMap(21, np.array([canonical(QUERY)], np.uint64), np.zeros(1, np.uint32), 1),
                     lambda h: h.count_block(*pack_reads(READS)),
                     lambda h: (h.finish()[0].tolist(), h.finish()[1])),
        "kc": Kind(lambda: vafc.KmerHistogram(21, 1 << 16),
                   lambda h: h.count_block(*pack_reads(READS)),
                   kc_result),
        "ed": Kind(lambda: vafc.EdCounter(queries=[QUERY, QUERY[:12]], max_edit=1),
                   lambda h: h.count_block(*pack_reads(READS)),
                   lambda h: h.finish().tolist()),
        "bam": Kind(lambda: bam_counter(BAM_ROWS, ["chr1"], tmp_path),
                    lambda h: h.count_block(*bam_block),
                    lambda h: h.finish().tolist()),
        "vcf": Kind(lambda: vafc.VcfMatcher(rows=[(r[0], r[1], r[3], r[4]) for r in VCF_ROWS]),
                    lambda h: h.scan_block(VCF_TEXT),
                    lambda h: [(int(x["off"]), int(x["row"])) for x in h.hits()[0]]),
    }


# QUERY is whole in two reads; 20 k-mers of 21 bases per 40-base read
WANT = {"kmer": ([2, 0], 4 * 20), "ed": None, "bam": [0, 4, 0, 4], "vcf": VF.device_lines(VCF_ROWS, VCF_TEXT)}


def kc_oracle(reads):
    hist, distinct, kmers = oracle_reads(21, *pack_reads(reads))
    return hist.tolist(), distinct, kmers


@pytest.fixture(scope="module", autouse=True)
def kc_want(built):
    """WANT["kc"]: the oracle's histogram of READS, once the oracle is built."""
    WANT["kc"] = kc_oracle(READS)


def raises_einval(h):
    import vafc
    with pytest.raises(vafc.VafcError) as e:
        h.kernel_ms()
    assert e.value.code == vafc.VC_EINVAL


# --- 1. the timer ----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ed", "bam", "vcf"])
def test_kernel_ms_needs_a_launch(kind, tmp_path):
    K = kinds(tmp_path)[kind]
    h = K.create()
    try:
        raises_einval(h)
        K.block(h)
        got = K.result(h)
        ms = h.kernel_ms()
        assert math.isfinite(ms) and ms > 0
        assert WANT[kind] is None or got == WANT[kind]
    finally:
        h.close()


def timer_follows_switch(K, want):
    h = K.create()
    try:
        raises_einval(h)
        K.block(h)
        assert K.result(h) == want
        raises_einval(h)                       # timing is off: nothing was recorded
        h.set_timing(True)
        raises_einval(h)
        K.block(h)
        h.finish()
        ms = h.kernel_ms()
        assert math.isfinite(ms) and ms > 0
        h.set_timing(True)                     # the switch clears what was recorded
        raises_einval(h)
        h.set_timing(False)
        K.block(h)
        h.finish()
        raises_einval(h)
    finally:
        h.close()


def test_kernel_ms_of_the_kmer_counter_follows_its_switch(tmp_path):
    timer_follows_switch(kinds(tmp_path)["kmer"], WANT["kmer"])


def test_kernel_ms_of_the_histogram_follows_its_switch(tmp_path):
    timer_follows_switch(kinds(tmp_path)["kc"], WANT["kc"])


# --- 2. lists that grow between batches ------------------------------------------

def bam_records(rng, n):
    recs = []
    for i in range(n):
        cigar = BF.random_cigar(rng, (1, 2, 3, 5, 8)[i % 5], 6, "MMMM=XIDN")
        l_seq = BF.query_len(cigar)
        nib = np.array([1, 2, 4, 8])[rng.integers(0, 4, l_seq + 1)]
        seq = bytes(int(nib[j]) << 4 | (int(nib[j + 1]) if j + 1 < l_seq else 0) for j in range(0, l_seq, 2))
        recs.append((0, int(rng.integers(0, 380)), 0, BF.cigar_words(cigar), l_seq, seq))
    return recs


def test_bam_long_list_regrows_between_batches(tmp_path):
    """8 records size the list to 8 + 2 + 1024 entries; 1,100 records do not fit
    it.  With a threshold of 0 the long kernel walks every entry of the list."""
    rng = np.random.default_rng(71)
    rows = [("chr1", p, "ACGT"[p % 4], "ACGT"[(p + 1 + p // 7) % 4]) for p in range(0, 400, 3)]
    first, second = bam_records(rng, 8), bam_records(rng, 1100)
    assert len(first) + len(first) // 4 + 1024 < len(second)

    def run(*batches):
        bc = bam_counter(rows, ["chr1"], tmp_path)
        try:
            bc.set_long_threshold(0)
            for b in batches:
                bc.count_block(*pack_bam(b))
            return bc.finish().astype(np.uint64)
        finally:
            bc.close()

    grown, only_first, only_second, together = run(first, second), run(first), run(second), run(first + second)
    assert int(only_first.sum()) > 0 and int(only_second.sum()) > 100
    assert np.array_equal(grown, together)
    assert np.array_equal(grown, only_first + only_second)


def test_kc_long_list_regrows_between_batches():
    """k = 21: 800 bytes need a list of 1 entry, 13,300 bytes one of 4 (a read
    longer than 4,096 bases takes an entry and a row of segment starts)."""
    import vafc
    rng = np.random.default_rng(72)
    first = [ACGT[rng.integers(0, 4, 100)].tobytes() for _ in range(8)]
    second = [ACGT[rng.integers(0, 4, n)].tobytes() for n in (4200, 9000, 100)]

    def run(*batches):
        h = vafc.KmerHistogram(21, 1 << 16)
        try:
            for b in batches:
                h.count_block(*pack_reads(b))
            h.finish()
            hist, d, km = h.histogram()
            return hist.tolist(), d, km
        finally:
            h.close()

    grown, only_second, together = run(first, second), run(second), run(first + second)
    assert grown == together == kc_oracle(first + second)
    assert only_second == kc_oracle(second)
    assert grown[2] == only_second[2] + kc_oracle(first)[2] and kc_oracle(first)[2] == 8 * 80


# --- 3. create / destroy churn ---------------------------------------------------

@pytest.mark.parametrize("kind", ["kmer", "kc", "ed", "bam", "vcf"])
def test_create_destroy_rounds(kind, tmp_path):
    K = kinds(tmp_path)[kind]
    first = None
    for r in range(20):
        h = K.create()
        try:
            K.block(h)
            if r == 7:
                continue                       # closed with the batch in flight
            got = K.result(h)
            first = got if first is None else first
            assert got == first, r
        finally:
            h.close()
    assert WANT[kind] is None or first == WANT[kind]
    assert first and any(first)


def test_correlation_rounds():
    """3 samples x 40 SNPs; sample 2 holds a NaN at a row deep enough to count,
    so its pairs are done again by the second kernel (the pair list)."""
    import vafc
    rng = np.random.default_rng(73)
    vaf = rng.random((3, 40))
    vaf[2, 5] = np.nan
    depth = rng.integers(5, 60, (3, 40)).astype(np.int32)
    first = None
    for r in range(20):
        corr, ms = vafc.correlation_matrix_raw(vaf, depth, min_snps=20, min_depth=1)
        first = corr if first is None else first
        assert np.array_equal(corr, first, equal_nan=True), r
        assert ms > 0
    assert np.isfinite(first[0, 1]) and first[0, 1] != 0 and np.isnan(first[0, 2]) and np.isnan(first[1, 2])
    assert first[0, 0] == first[1, 1] == first[2, 2] == 1.0


# --- 4. the two kinds of read counter ---------------------------------------------

def test_histogram_handle_refuses_pattern_calls(tmp_path):
    """The calls that mean something only for one kind are VC_EINVAL (NULL, 0)
    on the other; what every read counter has still answers, and both handles
    count afterwards."""
    import ctypes as C
    import vafc
    L, K = vafc.lib(), kinds(tmp_path)
    n = C.c_uint64()
    h = K["kc"].create()
    try:
        assert L.vc_bind_outputs(h._h, None, None) == vafc.VC_EINVAL
        assert L.vc_table_info(h._h, C.byref(n), None, None) == vafc.VC_EINVAL
        assert L.vc_set_nt4_decode(h._h, 1) == vafc.VC_EINVAL
        assert L.vc_device_counts(h._h) is None and L.vc_device_tally(h._h) is None
        assert L.vc_stream(h._h) and L.vc_shard_count(h._h) == 1
        assert L.vc_reserve_file_ingest(h._h, 2) == vafc.VC_OK
        K["kc"].block(h)
        assert K["kc"].result(h) == WANT["kc"]
    finally:
        h.close()
    m = K["kmer"].create()
    try:
        hist = np.zeros(256, np.uint64)
        assert L.vc_kc_histogram(m._h, hist.ctypes.data, None, None) == vafc.VC_EINVAL
        assert L.vc_kc_set_partition(m._h, 1, 0) == vafc.VC_EINVAL
        assert L.vc_kc_track_first(m._h, 1) == vafc.VC_EINVAL
        assert L.vc_kc_slots(m._h) == 0 and not hist.any()
        K["kmer"].block(m)
        assert K["kmer"].result(m) == WANT["kmer"]
    finally:
        m.close()


def test_histogram_and_map_through_the_parallel_file_reader(tmp_path, monkeypatch):
    """3,000 reads of 100 bases, with VAFC_INGEST_MIN=1 a file for the parallel
    reader (DeviceSink) at -t 2: a KmerHistogram, then a KmerMap, then the
    histogram again after reset(), in one process.  QUERY is planted in every
    500th read, on either strand."""
    import vafc
    import oracle as O
    rng = np.random.default_rng(74)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    reads = [ACGT[rng.integers(0, 4, 100)].tobytes() for _ in range(3000)]
    for i in range(0, 3000, 500):
        q = QUERY if i % 1000 else QUERY.translate(comp)[::-1]
        reads[i] = reads[i][:30 + i % 7] + q + reads[i][51 + i % 7:]
    assert all(len(r) == 100 for r in reads)
    fq = str(tmp_path / "reads.fq")
    with open(fq, "wb") as f:
        f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * 100) for i, r in enumerate(reads)))
    monkeypatch.setenv("VAFC_INGEST_MIN", "1")
    key = np.array([canonical(QUERY)], np.uint64)
    orc = O.Oracle(21, keys=key, vals=np.zeros(1, np.uint32))
    want_counts, want_kmers = orc.count_reads(*pack_reads(reads), n_patterns=1)
    orc.close()
    want_kc = kc_oracle(reads)
    assert want_counts.tolist() == [6, 0] and want_kmers == want_kc[2] == 3000 * 80
    h = vafc.KmerHistogram(21, 1 << 20)
    m = vafc.KmerMap(21, key, np.zeros(1, np.uint32), 1)
    try:
        st = h.count_file(fq, 10_000_000, 2)
        assert (st.seqs, st.bases) == (3000, 300_000)
        assert kc_result(h) == want_kc
        st = m.count_file(fq, 10_000_000, 2)
        assert (st.seqs, st.bases) == (3000, 300_000)
        counts, kmers = m.finish()
        assert counts.tolist() == want_counts.tolist() and kmers == want_kmers
        h.reset()
        h.count_file(fq, 10_000_000, 2)
        assert kc_result(h) == want_kc
    finally:
        h.close()
        m.close()


# --- 5. VcfMatcher on a caller's stream ------------------------------------------

def test_vcf_scan_device_on_a_side_stream():
    """scan_device on a torch side stream straight after a scan_block on the
    handle's own stream: hits() gives the lines of both, each at its offset."""
    import torch
    import vafc
    body = VF.synth_vcf(VCF_ROWS, 60, 1, seed=8, hit_rate=0.3, header_too=False)
    want_dev = VF.device_lines(VCF_ROWS, body, len(VCF_TEXT))
    assert sum(r >= 0 for _, r in want_dev) >= 5
    dev = torch.device("cuda", 0)
    d_text = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(dev)
    side = torch.cuda.Stream(device=dev)
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    m = vafc.VcfMatcher(rows=[(r[0], r[1], r[3], r[4]) for r in VCF_ROWS])
    try:
        assert m.scan_block(VCF_TEXT) == len(VCF_TEXT)
        m.scan_device(d_text.data_ptr(), len(body), len(VCF_TEXT), True, side.cuda_stream)
        hits, consumed = m.hits()
        assert consumed == len(body)
        assert [(int(h["off"]), int(h["row"])) for h in hits] == WANT["vcf"] + want_dev
    finally:
        m.close()

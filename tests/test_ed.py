"""ed-vaf-counter: approximate pattern search in reads.

CPU: a Python statement of the contract (include/vafc.h, vc_ed_create; it
lives in tests/ed_fixture.py): a plain DP and a numpy form over queries,
checked against each other; the
statement, run through Python restatements of the pattern loader
(ed-vaf-counter.c:47-83), the kseq reader (kseq.h:192-232) and the .vaf writer
(ed-vaf-counter.c:204-228), reproduces every golden .vaf of
tests/golden/ed/manifest.json (written by the reference binary,
tests/golden/make_golden_ed.py); csrc/vafc_opt.h equals vafc.ketopt_scan.

GPU: the CLI equals the manifest, EdCounter equals the statement.  Equality is
exact everywhere."""
import gzip
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from ed_fixture import Statement, dp_hits, pad_w, rule, scan_read  # noqa: F401  (the statement)

ED = os.path.join(GOLDEN, "ed")
CLI = os.path.join(PKG, "lib", "ed-vaf-counter")

with open(os.path.join(ED, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
for _case in MANIFEST.values():      # "=<case>": the same content as that case's file of the same name
    for _fn, _text in _case["files"].items():
        if _text.startswith("="):
            _case["files"][_fn] = MANIFEST[_text[1:]]["files"][_fn]


def test_fast_form_equals_dp():
    rng = np.random.default_rng(11)
    total = 0
    for it in range(160):
        m = int(rng.choice([1, 2, 5, 21, 31, 32, 33, 40]))
        sig = int(rng.integers(2, 6))
        alpha = np.frombuffer(b"ACGTNacgt\xe9\x00", np.uint8)[:sig + int(rng.integers(0, 5))]
        qs = [bytes(rng.choice(alpha, m)) for _ in range(3)]
        n = int(rng.integers(0, 70))
        T = bytearray(rng.choice(alpha, n).tobytes())
        if n >= m and it % 2:
            at = int(rng.integers(0, n - m + 1))
            T[at:at + m] = qs[0]
            if m > 2:
                T[at + m // 2] = int(alpha[0])
        T = bytes(T)
        st = Statement(qs, [T])
        for e in (0, 1, 2, 3, 5, -1, m, m + 5, 200):
            want = [dp_hits(q, T, e) for q in qs]
            assert st.counts(e).tolist() == want, (m, n, e)
            total += sum(want)
    assert total > 0


# ---------------------------------------------------------------------------
# loader, reader, writer
# ---------------------------------------------------------------------------

WS = b" \t\n\v\f\r"


def load_patterns_py(data: bytes):
    """fscanf(fp, "%255s%d%d%255s %c %c%127s%127s") == 8 rows (ed-vaf-counter.c:62-79)."""
    pos, rows = 0, []

    def skip():
        nonlocal pos
        while pos < len(data) and data[pos] in WS:
            pos += 1

    def word(width):
        nonlocal pos
        skip()
        b = pos
        while pos < len(data) and data[pos] not in WS and pos - b < width:
            pos += 1
        return data[b:pos] if pos > b else None

    def integer():
        nonlocal pos
        skip()
        b = pos
        if pos < len(data) and data[pos] in b"+-":
            pos += 1
        d = pos
        while pos < len(data) and 48 <= data[pos] <= 57:
            pos += 1
        return int(data[b:pos]) if pos > d else None

    def char():
        nonlocal pos
        skip()
        if pos >= len(data):
            return None
        pos += 1
        return data[pos - 1:pos]

    while True:
        rec = []
        for get in (lambda: word(255), integer, integer, lambda: word(255), char, char, lambda: word(127),
                    lambda: word(127)):
            v = get()
            if v is None:
                return rows
            rec.append(v)
        rows.append(rec)


def queries_of(rows):
    """Two queries per row: ref_kmer, and the first strlen(ref_kmer) bytes of
    alt_kmer, NUL-padded when it is shorter."""
    out = []
    for r in rows:
        m = len(r[6])
        out.append(r[6])
        out.append((r[7][:m]).ljust(m, b"\0"))
    return out


def kseq_records(data: bytes):
    """Sequences of the records kseq_read returns >= 0 for, up to the first
    negative return (kseq.h:192-232)."""
    pos, n = 0, len(data)
    last = 0
    seqs = []

    def getc():
        nonlocal pos
        if pos >= n:
            return -1
        pos += 1
        return data[pos - 1]

    def line(acc: bytearray):
        """ks_getuntil2(KS_SEP_LINE, append): -1 at the end of the input."""
        nonlocal pos
        if pos >= n:
            return -1
        e = data.find(b"\n", pos)
        if e < 0:
            acc += data[pos:]
            pos = n
        else:
            acc += data[pos:e]
            pos = e + 1
        if len(acc) > 1 and acc[-1] == 13:
            del acc[-1]
        return len(acc)

    while True:
        if last == 0:
            c = getc()
            while c != -1 and c not in (62, 64):
                c = getc()
            if c == -1:
                return seqs
            last = c
        if pos >= n:
            return seqs            # ks_getuntil(name) < 0
        c = -1
        while pos < n:             # the name: up to an isspace byte
            c = getc()
            if c in WS:
                break
            c = -1
        if c != 10 and c != -1:
            line(bytearray())      # the comment
        seq = bytearray()
        c = getc()
        while c != -1 and c not in (62, 43, 64):
            if c != 10:
                seq.append(c)
                line(seq)
            c = getc()
        if c in (62, 64):
            last = c
        if c != 43:
            seqs.append(bytes(seq))      # FASTA; at the end of the input last_char stays set
            continue
        c = getc()
        while c != -1 and c != 10:
            c = getc()
        if c == -1:
            return seqs            # -2: no quality string
        qual = bytearray()
        while line(qual) >= 0 and len(qual) < len(seq):
            pass
        last = 0
        if len(qual) != len(seq):
            return seqs            # -2
        seqs.append(bytes(seq))


def read_file_py(path):
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return None
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    return kseq_records(data)


def vaf_text(rows, counts):
    """ed-vaf-counter.c:204-228."""
    n = len(rows)
    tot = sum(int(c) for c in counts[:2 * n])
    out = ["# Average depth: %.2f\n" % (tot / (n if n > 0 else 1)),
           "CHR\tPOS\tRSID\tREF\tALT\tREF_COUNT\tALT_COUNT\tTOTAL_COUNT\tVAF\n"]
    for i, r in enumerate(rows):
        rc, ac = int(counts[2 * i]), int(counts[2 * i + 1])
        t = (rc + ac) & 0xFFFFFFFF
        out.append("%s\t%d\t%s\t%s\t%s\t%d\t%d\t%d\t%.4f\n" % (
            r[0].decode("latin-1"), r[1], r[3].decode("latin-1"), r[4].decode("latin-1"), r[5].decode("latin-1"),
            rc, ac, t, (ac / t) if t > 0 else 0.0))
    return "".join(out)


_statements = {}


def statement_for(pattern_fn, read_fn):
    key = (pattern_fn, read_fn)
    if key not in _statements:
        with open(os.path.join(ED, pattern_fn), "rb") as f:
            rows = load_patterns_py(f.read())
        reads = read_file_py(os.path.join(ED, read_fn))
        _statements[key] = (rows, None if reads is None else Statement(queries_of(rows), reads))
    return _statements[key]


def test_kseq_restatement_on_fixtures():
    assert kseq_records(b"@a x\nACGT\n+\nIIII\n@b\n\n+\n\n>c\nAC\nGT\n\n>d\n") == [b"ACGT", b"", b"ACGT", b""]
    assert kseq_records(b"@a\nACGT\n+\nII") == []
    assert kseq_records(b"@a\r\nACGT\r\n+\r\nIIII\r\n") == [b"ACGT"]
    assert len(read_file_py(os.path.join(ED, "r_trunc.fq"))) == 9     # ten records, the last one cut
    assert read_file_py(os.path.join(ED, "r150.fq.gz")) == read_file_py(os.path.join(ED, "r150.fq"))


def test_statement_reproduces_every_golden_vaf():
    import vafc
    done = 0
    for name, case in sorted(MANIFEST.items()):
        o, files = vafc.ed_parse_args(case["argv"])
        if not o["p"] or not o["o"] or not files:
            assert case["rc"] == 1 and not case["files"], name
            continue
        if not os.path.exists(os.path.join(ED, o["p"])) or os.path.dirname(o["o"]) != "o":
            assert case["rc"] == 1 and not case["files"], name      # no pattern file, no output directory
            continue
        assert case["rc"] == 0, name
        total = None
        for fn in files:
            rows, st = statement_for(o["p"], fn)
            if total is None:
                total = np.zeros(2 * len(rows), np.uint32)
            if st is not None:
                total = total + st.counts(o["e"])      # uint32: wraps
        assert case["files"] == {o["o"]: vaf_text(rows, total)}, name
        done += 1
    assert done >= 60


# ---------------------------------------------------------------------------
# csrc/vafc_opt.h against the Python mirror
# ---------------------------------------------------------------------------

OPT_PROG = r"""
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "vafc_opt.h"
int main(int argc, char **argv)
{
	FILE *fp = fopen(argv[1], "rb");
	if (!fp) return 2;
	std::string all;
	char buf[4096];
	size_t k;
	while ((k = fread(buf, 1, sizeof buf, fp)) > 0) all.append(buf, k);
	fclose(fp);
	size_t pos = 0;
	while (pos < all.size()) {
		size_t e = all.find('\n', pos);
		std::string ln = all.substr(pos, e - pos);
		pos = e + 1;
		std::vector<std::string> words(1, "prog");
		if (ln != "!") {
			size_t b = 0;
			for (;;) {
				size_t s = ln.find('\x1f', b);
				words.push_back(ln.substr(b, s == std::string::npos ? s : s - b));
				if (s == std::string::npos) break;
				b = s + 1;
			}
		}
		std::vector<char *> av;
		for (auto &w : words) av.push_back(&w[0]);
		av.push_back(nullptr);
		VcOpt o;
		int c;
		while ((c = vc_opt_next(o, (int)words.size(), av.data(), "p:o:e:")) >= 0)
			printf("O\t%d\t%s\t%s\n", c, o.arg ? "1" : "0", o.arg ? o.arg : "");
		for (const char *f : o.files) printf("F\t%s\n", f);
		printf("END\n");
	}
	return 0;
}
"""


def test_opt_header_equals_python_mirror(tmp_path):
    import vafc
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    assert cxx, "no C++ compiler"
    src = tmp_path / "opt_prog.cpp"
    src.write_text(OPT_PROG)
    exe = str(tmp_path / "opt_prog")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(PKG, "csrc"), str(src), "-o", exe],
                   check=True)
    rng = np.random.default_rng(5)
    words = ["-p", "-o", "-e", "-e5", "-e-1", "-pfile", "-x", "-xe", "-xp", "-ep", "--", "--oops", "--p=1", "-", "",
             "a.fq", "b", "-:", "-o:", "-?", "2", "-e2x", "p.txt", "-\xe9"]
    lists = [c["argv"] for _, c in sorted(MANIFEST.items())]
    for _ in range(400):
        lists.append([words[i] for i in rng.integers(0, len(words), int(rng.integers(0, 8)))])
    inp = tmp_path / "cases.txt"
    inp.write_bytes(b"".join((b"\x1f".join(w.encode("latin-1") for w in lst) if lst else b"!") + b"\n"
                             for lst in lists))
    out = subprocess.run([exe, str(inp)], check=True, capture_output=True).stdout.decode("latin-1")
    blocks = out.split("END\n")[:-1]
    assert len(blocks) == len(lists)
    n_opts = 0
    for lst, blk in zip(lists, blocks):
        got_o, got_f = [], []
        for ln in blk.split("\n")[:-1]:
            f = ln.split("\t")
            if f[0] == "O":
                got_o.append((chr(int(f[1])), f[3] if f[2] == "1" else None))
            else:
                got_f.append(f[1])
        want_o, want_f = vafc.ketopt_scan(lst, "p:o:e:")
        assert (got_o, got_f) == (want_o, want_f), lst
        n_opts += len(got_o)
    assert n_opts > 400
    assert [vafc.c_atoi(s) for s in ("2x", "abc", " -3", "+7", "", "-", "1e3")] == [2, 0, -3, 7, 0, 0, 1]


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def pack(reads):
    lens = np.array([len(r) for r in reads], np.uint32)
    offs = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    blob = np.frombuffer(b"".join(reads), np.uint8) if lens.sum() else np.zeros(0, np.uint8)
    return blob, offs, lens


def gpu_counts(queries, reads, e, max_ranges=0):
    import vafc
    ed = vafc.EdCounter(queries=queries, max_edit=e)
    try:
        ed.set_max_ranges(max_ranges)
        ed.count_block(*pack(reads))
        return ed.finish()
    finally:
        ed.close()


def planted(rng, queries, n_reads, max_len, alphabet, min_len=0):
    """Random reads, most with a mutated copy of a query in them."""
    alphabet = np.frombuffer(bytes(alphabet), np.uint8)
    reads = []
    for i in range(n_reads):
        n = int(rng.integers(min_len, max_len + 1))
        T = bytearray(rng.choice(alphabet, n).tobytes())
        q = bytearray(queries[int(rng.integers(0, len(queries)))])
        if i % 4 and len(q) <= n:
            for _ in range(i % 3):
                j = int(rng.integers(0, len(q)))
                kind = int(rng.integers(0, 3))
                if kind == 0:
                    q[j] = int(alphabet[int(rng.integers(0, len(alphabet)))])
                elif kind == 1 and len(q) > 1:
                    del q[j]
                elif len(q) < n:
                    q.insert(j, int(alphabet[int(rng.integers(0, len(alphabet)))]))
            at = int(rng.integers(0, n - len(q) + 1))
            T[at:at + len(q)] = q
        reads.append(bytes(T))
    return reads


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_cli_equals_reference(name, tmp_path):
    case = MANIFEST[name]
    work = tmp_path / "w"
    work.mkdir()
    for fn in os.listdir(ED):
        if fn != "manifest.json":
            os.symlink(os.path.join(ED, fn), str(work / fn))
    (work / "o").mkdir()
    p = subprocess.run([CLI] + case["argv"], cwd=str(work), capture_output=True, timeout=120)
    files = {}
    for fn in sorted(os.listdir(str(work / "o"))):
        with open(str(work / "o" / fn)) as f:
            files["o/" + fn] = f.read()
    assert p.stderr.decode() == case["stderr"]
    assert p.returncode == case["rc"]
    assert files == case["files"]


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 31, 32, 33, 63, 64, 65, 127])
def test_fuzz_word_widths_and_lane_edges(m):
    rng = np.random.default_rng(1000 + m)
    alpha = b"ACGT" if m > 2 else b"AC"
    base = [bytes(rng.choice(np.frombuffer(alpha, np.uint8), m)) for _ in range(8)]
    queries = []
    for i in range(129):      # relatives of eight base queries: hits spread over the lanes
        q = bytearray(base[i % 8])
        if i >= 8:
            q[int(rng.integers(0, m))] = alpha[int(rng.integers(0, len(alpha)))]
        queries.append(bytes(q))
    reads = planted(rng, base, 56, 300, alpha) + [b"", b"A", bytes(base[0][:max(m - 1, 0)]), base[1]]
    st = Statement(queries, reads)
    total = 0
    for e in (0, 1, 3, m, -1):
        want = st.counts(e)
        for nq in (1, 2, 63, 64, 65, 129):
            got = gpu_counts(queries[:nq], reads, e)
            assert np.array_equal(got, want[:nq]), (m, e, nq, np.nonzero(got != want[:nq])[0][:5])
        total += int(want.astype(np.int64).sum())
    assert total > 0


@pytest.mark.gpu
def test_fuzz_mixed_lengths_in_one_handle():
    rng = np.random.default_rng(77)
    lens = [1, 2, 21, 21, 31, 32, 33, 48, 63, 64, 65, 100, 126, 127] * 14
    a = np.frombuffer(b"ACGT", np.uint8)
    queries = [bytes(rng.choice(a, m)) for m in lens]
    reads = planted(rng, queries, 40, 260, b"ACGT") + [b""]
    st = Statement(queries, reads)
    for e in (0, 2, -1):
        want = st.counts(e)
        assert np.array_equal(gpu_counts(queries, reads, e), want), e
        assert int(want.astype(np.int64).sum()) > 0


_range_sets = {}


def range_workload(kind):
    """Queries, unique reads and an order in which a read range of hundreds of
    reads meets every way a block lays reads out in its 4,096-byte chunks: runs
    of more than 64 empty and tiny reads (the 64-read cut), 100-200 byte reads
    (the byte cut after about 27), reads of 1-3 KB (the cut falls in the
    middle of a range), and one 9,000-byte read between short ones (its tail
    shares a chunk with the reads after it).  The order repeats few unique
    reads, so the statement scans each once."""
    if kind in _range_sets:
        return _range_sets[kind]
    rng = np.random.default_rng(31)
    a = np.frombuffer(b"ACGT", np.uint8)
    if kind == "three_widths":          # one-wave blocks of each word width
        queries = [bytes(rng.choice(a, m)) for m in (12, 32, 50, 100) for _ in range(2)]
    else:                               # 300 queries of one width: four-wave blocks, two of them
        base = [bytes(rng.choice(a, 10)) for _ in range(6)]
        queries = []
        for i in range(300):
            q = bytearray(base[i % 6])
            if i >= 6:
                q[int(rng.integers(0, 10))] = int(a[int(rng.integers(0, 4))])
            queries.append(bytes(q))
    plant = queries[:8]
    shorts = planted(rng, plant, 120, 40, b"ACGT", min_len=20)
    tiny = [b"", b"A", b"AC", b"ACG", b"", b"T"]
    medium = planted(rng, plant, 40, 200, b"ACGT", min_len=100)
    mids = planted(rng, plant, 5, 3000, b"ACGT", min_len=1000)
    big = bytearray(rng.choice(a, 9000).tobytes())
    for at, q in ((4096 - 5, plant[0]), (8192 - len(plant[-1]) + 3, plant[-1]), (9000 - len(plant[1]), plant[1])):
        big[at:at + len(q)] = q
    uniq = shorts + tiny + medium + mids + [bytes(big)]
    i_short, i_tiny = np.arange(0, 120), np.arange(120, 126)
    i_med, i_mid, i_big = np.arange(126, 166), np.arange(166, 171), 171
    order = []
    for blk in range(6):
        order += rng.choice(i_short, 100).tolist()
        order += rng.choice(i_tiny, 80).tolist()
        order += [int(i_mid[blk % 5])]
        order += rng.choice(i_med, 45).tolist()
        if blk == 3:
            order += rng.choice(i_short, 7).tolist() + [i_big] + rng.choice(i_tiny, 3).tolist()
        order += rng.choice(i_short, 30).tolist()
    order = np.array(order)
    times = np.bincount(order, minlength=len(uniq))
    _range_sets[kind] = (queries, [uniq[i] for i in order], Statement(queries, uniq), times)
    return _range_sets[kind]


@pytest.mark.gpu
@pytest.mark.parametrize("max_ranges", [1, 3, 7, 40])
@pytest.mark.parametrize("kind", ["three_widths", "five_groups"])
def test_read_ranges_of_many_reads(kind, max_ranges):
    """Blocks that walk hundreds of reads each (vc_ed_set_max_ranges: by
    default a batch of this size would be cut into one read per block)."""
    queries, reads, st, times = range_workload(kind)
    assert len(reads) > 1500
    for e in (0, 2, -1):
        want = st.counts(e, times)
        got = gpu_counts(queries, reads, e, max_ranges)
        assert np.array_equal(got, want), (e, np.nonzero(got != want)[0][:5])
        assert int(want.sum()) > 0


@pytest.mark.gpu
def test_many_short_reads_one_read_per_block():
    """5,000 reads against three queries: with the default grid every block
    takes one read (the widest grid a batch gets)."""
    rng = np.random.default_rng(3)
    a = np.frombuffer(b"ACGT", np.uint8)
    queries = [bytes(rng.choice(a, 12)) for _ in range(3)]
    reads = planted(rng, queries, 5000, 40, b"ACGT", min_len=20)
    st = Statement(queries, reads)
    for e in (0, 2):
        want = st.counts(e)
        assert np.array_equal(gpu_counts(queries, reads, e), want)
        assert int(want.sum()) > 0


@pytest.mark.gpu
def test_one_long_read_carries_state_across_chunks():
    rng = np.random.default_rng(4)
    a = np.frombuffer(b"ACGT", np.uint8)
    queries = [bytes(rng.choice(a, m)) for m in (21, 40, 70, 21)]
    T = bytearray(rng.choice(a, 20000).tobytes())
    for at, q in ((4090, queries[0]), (4096 - 30, queries[1]), (8192 - 5, queries[2]), (19979, queries[3]),
                  (12288 - 21, queries[0])):
        T[at:at + len(q)] = q          # copies that straddle or touch the chunk boundaries
    reads = [bytes(T), b"ACGT", bytes(T[:4096]), bytes(T[:4097]), bytes(T[:4095]), b"", bytes(T[4000:12300])]
    st = Statement(queries, reads)
    for e in (0, 1, 3):
        want = st.counts(e)
        assert np.array_equal(gpu_counts(queries, reads, e), want), e
        assert int(want.sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("alphabet", [b"acgtACGTN", bytes(range(0x80, 0x80 + 12)) + b"AC\x00",
                                      bytes(range(40, 110)), bytes(range(256))],
                         ids=["lower_N", "high_bytes", "70_symbols", "all_256"])
def test_byte_sets(alphabet):
    """Exact byte equality over small and large symbol sets.  With 70 symbols
    and with all 256 byte values every width reads its masks from HBM: the 200
    queries of up to 32 bytes make four-wave blocks (71 classes x 4 waves x 64
    lanes x 4 bytes = 71 KiB against the 32 KiB kept in LDS), the 64-bit and
    2x64-bit groups exceed it with one wave."""
    rng = np.random.default_rng(len(alphabet))
    a = np.frombuffer(alphabet, np.uint8)
    lens = [5, 21, 33, 64, 100, 127] * 12 + [5, 21] * 88
    queries = [bytes(rng.choice(a, m)) for m in lens]
    if len(alphabet) == 256:
        queries[3] = bytes(range(0, 64))
        queries[4] = bytes(range(64, 164))
        queries[5] = bytes(range(129, 256))
    reads = planted(rng, queries, 30, 200, alphabet) + [queries[5] + queries[4], b"\xff" * 10]
    if len(alphabet) < 256:
        reads.append(bytes(range(256)))     # bytes outside the query set
    st = Statement(queries, reads)
    for e in (0, 2):
        want = st.counts(e)
        assert np.array_equal(gpu_counts(queries, reads, e), want), e
        assert int(want.sum()) > 0


@pytest.mark.gpu
def test_short_reads_around_the_pad_width_and_empty_reads():
    rng = np.random.default_rng(9)
    a = np.frombuffer(b"ACGT", np.uint8)
    lens = [1, 21, 31, 33, 63, 65, 100, 127]
    queries = [bytes(rng.choice(a, m)) for m in lens for _ in range(2)]
    reads = []
    for m in lens:
        w = pad_w(m)
        for n in sorted({0, 1, m - 1, m, w - 1, w, w + 1} - {-1}):
            reads += [bytes(rng.choice(a, n)), queries[2 * lens.index(m)][:n], b""]
    st = Statement(queries, reads)
    seen = set()
    for e in (0, 1, 3, 21, 127, 500, -1, -7):
        want = st.counts(e)
        assert np.array_equal(gpu_counts(queries, reads, e), want), e
        seen.add(tuple(want.tolist()))
    assert len(seen) >= 5     # the bound, and the extra candidate, change the counts


@pytest.mark.gpu
def test_accumulation_reset_and_wrap():
    import torch
    import vafc
    rng = np.random.default_rng(21)
    a = np.frombuffer(b"ACGT", np.uint8)
    queries = [bytes(rng.choice(a, m)) for m in (21, 21, 40, 90, 5)]
    reads = planted(rng, queries, 90, 200, b"ACGT") + [b""]
    want = Statement(queries, reads).counts(2)
    assert int(want.sum()) > 0
    ed = vafc.EdCounter(queries=queries, max_edit=2)
    try:
        ed.count_block(*pack(reads))
        assert np.array_equal(ed.finish(), want)
        ed.reset()
        assert not ed.finish().any()
        ed.count_block(*pack(reads[:30]))
        ed.count_block(*pack(reads[30:60]))
        blob, offs, lens = pack(reads[60:])
        dev = torch.device("cuda", 0)
        d_seq = torch.from_numpy(blob.copy()).to(dev)
        d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
        d_lens = torch.from_numpy(lens.astype(np.int32)).to(dev)
        ed.count_device(d_seq.data_ptr(), blob.size, d_offs.data_ptr(), d_lens.data_ptr(), lens.size,
                        torch.cuda.current_stream().cuda_stream)
        assert np.array_equal(ed.finish(), want)
        assert ed.kernel_ms() > 0
        # counts wrap at 2^32 like the reference's uint32 fields
        start = np.full(len(queries), 0xFFFFFFFF, np.uint32)
        start[1] = 0xFFFFFFF0
        ed.set_counts(start)
        ed.count_device(d_seq.data_ptr(), blob.size, d_offs.data_ptr(), d_lens.data_ptr(), lens.size, vafc.STREAM_CTX)
        part = Statement(queries, reads[60:]).counts(2)
        assert int(part.min()) > 0
        assert np.array_equal(ed.finish(), start + part)      # uint32 arithmetic
        # a device read past seq_bytes is reported, not followed
        ed.reset()
        ed.count_device(d_seq.data_ptr(), blob.size - 1, d_offs.data_ptr(), d_lens.data_ptr(), lens.size)
        with pytest.raises(vafc.VafcError):
            ed.finish()
    finally:
        ed.close()


@pytest.mark.gpu
def test_invalid_lengths_are_rejected():
    import vafc
    for qs in ([b""], [b"A" * 128], [b"ACGT", b""]):
        with pytest.raises(vafc.VafcError) as ei:
            vafc.EdCounter(queries=qs)
        assert ei.value.code == vafc.VC_EINVAL
    ed = vafc.EdCounter(queries=[b"A" * 127, b"C"])
    ed.close()


@pytest.mark.gpu
def test_count_file_and_pattern_handle(tmp_path):
    import vafc
    db = vafc.load_patterns(os.path.join(ED, "p_mixed.txt"))
    ed = vafc.EdCounter(db, max_edit=1)
    try:
        st = ed.count_file(os.path.join(ED, "r_mix.fq"))
        reads = read_file_py(os.path.join(ED, "r_mix.fq"))
        assert (st.seqs, st.bases) == (len(reads), sum(len(r) for r in reads))
        with pytest.raises(FileNotFoundError):
            ed.count_file(os.path.join(ED, "nope.fq"))
        ed.count_file(os.path.join(ED, "r150.fq.gz"))
        got = ed.finish()
    finally:
        ed.close()
    rows, s1 = statement_for("p_mixed.txt", "r_mix.fq")
    _, s2 = statement_for("p_mixed.txt", "r150.fq.gz")
    assert np.array_equal(got, s1.counts(1) + s2.counts(1))
    # a shorter alt_kmer is NUL-padded
    pat = tmp_path / "p.txt"
    pat.write_text("chr1\t1\t2\trs1\tA\tC\tACGTACGTACGTACGTACGTA\tACGTACGTAC\n"
                   "chr1\t5\t6\trs2\tA\tC\tACGTA\tACGTACGTACGTACGTACGTA\n")
    db2 = vafc.load_patterns(str(pat))
    reads = [b"TTACGTACGTACGTACGTACGTATT", b"ACGTACGTAC", b"ACGTA"]
    ed = vafc.EdCounter(db2, max_edit=11)
    try:
        ed.count_block(*pack(reads))
        got = ed.finish()
    finally:
        ed.close()
    qs = [b"ACGTACGTACGTACGTACGTA", b"ACGTACGTAC" + b"\0" * 11, b"ACGTA", b"ACGTA"]
    assert np.array_equal(got, Statement(qs, reads).counts(11))


def batches_of(lens, limit, max_reads):
    """How many batches the file pass's writer submits (csrc/vafc_stage.h): a
    batch is closed by the read that would take it past `limit` bytes or
    `max_reads` reads; a longer read is a batch of its own."""
    n_batches, nbytes, n = 0, 0, 0
    for ln in lens:
        if n and (nbytes + ln > limit or n >= max_reads):
            n_batches, nbytes, n = n_batches + 1, 0, 0
        nbytes, n = nbytes + ln, n + 1
    return n_batches + (1 if n else 0)


_batch_file = {}


def batch_file_workload():
    """Four queries, one per word width and a second 32-bit one, and reads for
    3,000-byte batches: 150-base reads, one read of exactly the batch size, a
    20,000-base read (it grows an empty slot of 3000 + 750 + 4096 bytes), more
    short reads and a 20,000-base read as the last record.  Copies of the
    queries, some with one substitution, lie in every kind of read."""
    if not _batch_file:
        rng = np.random.default_rng(58)
        a = np.frombuffer(b"ACGT", np.uint8)
        queries = [bytes(rng.choice(a, m)) for m in (21, 33, 65, 100)]

        def long_read(n):
            T = bytearray(rng.choice(a, n).tobytes())
            for j, at in enumerate(range(50, n - 200, max(n // 7, 300))):
                q = bytearray(queries[j % 4])
                if j % 2:
                    q[len(q) // 2] = ord("A") if q[len(q) // 2] != ord("A") else ord("C")
                T[at:at + len(q)] = q
            return bytes(T)

        reads = (planted(rng, queries, 30, 150, b"ACGT", min_len=150) + [long_read(3000), long_read(20000)]
                 + planted(rng, queries, 30, 150, b"ACGT", min_len=150) + [long_read(20000)])
        _batch_file.update(queries=queries, reads=reads, st=Statement(queries, reads))
    return _batch_file["queries"], _batch_file["reads"], _batch_file["st"]


@pytest.mark.gpu
@pytest.mark.parametrize("e", [0, 1])
def test_count_file_small_batches_and_slot_growth(e, tmp_path, monkeypatch):
    """vc_ed_count_file through the batch writer it shares with vc_count_file,
    with VAFC_BATCH_BYTES=3000: the file is split into many batches, two of
    them one long read in a slot grown for it, the last of these flushed at
    the end of the file."""
    import vafc
    queries, reads, st = batch_file_workload()
    lens = [len(r) for r in reads]
    assert lens[30:32] == [3000, 20000] and lens[-1] == 20000 and set(lens) == {150, 3000, 20000}
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    monkeypatch.setenv("VAFC_BATCH_BYTES", "3000")
    ed = vafc.EdCounter(queries=queries, max_edit=e)
    try:
        fs = ed.count_file(str(fq))
        got = ed.finish()
    finally:
        ed.close()
    want = st.counts(e)
    assert np.array_equal(got, want), (got, want)
    assert int(want.min()) > 0
    assert (fs.seqs, fs.bases) == (len(reads), sum(lens))
    n_batches = batches_of(lens, 3000, 1 << 18)
    assert n_batches == 7 and fs.blocks == n_batches      # 20 reads of 150 bases fill a batch


@pytest.mark.gpu
def test_count_device_side_stream_after_reset():
    """vc_ed_count_device on a torch side stream right after a vc_ed_reset on
    the handle's own stream, which is still busy with an earlier batch, and no
    host synchronisation in between: the reset comes first, and vc_ed_finish
    sees the launch.  The counts equal the same reads through count_block."""
    import torch
    import vafc
    rng = np.random.default_rng(59)
    a = np.frombuffer(b"ACGT", np.uint8)
    queries = [bytes(rng.choice(a, m)) for m in (21, 33, 65, 100)]
    reads = planted(rng, queries, 2000, 150, b"ACGT", min_len=100)
    blob, offs, lens = pack(reads)
    dev = torch.device("cuda", 0)
    d_seq = torch.from_numpy(blob.copy()).to(dev)
    d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ed = vafc.EdCounter(queries=queries, max_edit=1)
    try:
        ed.count_block(blob, offs, lens)
        want = ed.finish().copy()
        assert int(want.min()) > 0
        ed.count_block(blob, offs, lens)      # queued on the handle's stream, to be reset
        ed.reset()
        ed.count_device(d_seq.data_ptr(), blob.size, d_offs.data_ptr(), d_lens.data_ptr(), lens.size,
                        side.cuda_stream)
        got = ed.finish()
    finally:
        ed.close()
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_exact_search_is_the_forward_share_of_the_kmer_counter(tmp_path):
    """-e 0 counts the exact forward occurrences: with distinct, non-palindromic
    k-mers, forward hits plus the hits in the reverse-complemented reads are
    what the canonical k-mer counter (vc_count_block) counts."""
    import vafc
    import vafc_synth as S
    panel = S.make_panel(S.read_bed(S.default_bed_path())[:150])
    pat = str(tmp_path / "p.txt")
    panel.write_patterns(pat, 21)
    db = vafc.load_patterns(pat)
    keys, vals, coll = db.keys(21)
    assert coll == 0 and keys.size == 2 * db.n
    reads = [r.tobytes() for r in S.gen_reads(panel, 400, f_snp=0.9)]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    rc_reads = [r.translate(comp)[::-1] for r in reads]
    kmap = vafc.create_combined_kmer_map(db, 21)
    kmap.count_block(*pack(reads))
    both, _ = kmap.finish()
    kmap.close()
    ed = vafc.EdCounter(db, max_edit=0)
    try:
        ed.count_block(*pack(reads))
        fwd = ed.finish().copy()
        ed.reset()
        ed.count_block(*pack(rc_reads))
        rev = ed.finish().copy()
    finally:
        ed.close()
    assert int(fwd.sum()) > 0 and int(rev.sum()) > 0
    assert np.array_equal(fwd + rev, both)
    recs = [db.record(i) for i in range(db.n)]
    want = np.zeros(2 * db.n, np.uint32)
    for i, r in enumerate(recs):
        for al, k in enumerate((r[5], r[6])):
            want[2 * i + al] = sum(sum(1 for j in range(len(t) - 20) if t[j:j + 21] == k) for t in reads)
    assert np.array_equal(fwd, want)

#!/usr/bin/env python3
"""Golden fixtures for bam-vaf-counter from the REAL reference binary.

Build the two programs by hand into a scratch directory.  The reference's own
rule links -lcurl -lcrypto -ldeflate; zlib alone is enough:

    cp -r <reference>/htslib <scratch>/htslib && cd <scratch>/htslib
    ./configure --disable-bz2 --disable-lzma --disable-libcurl --disable-gcs --disable-s3 --without-libdeflate
    make lib-static
    gcc -g -Wall -O2 -I<reference> -I<scratch>/htslib <reference>/bam-vaf-counter.c <reference>/kthread.c \\
        <scratch>/htslib/libhts.a -lz -lm -lpthread -o <scratch>/bam-vaf-counter
    # the indexer: a C program of ten lines whose main calls sam_index_build(argv[i], 0) for every argument
    gcc -O2 -I<scratch>/htslib bai_index.c <scratch>/htslib/libhts.a -lz -lm -lpthread -o <scratch>/bai-index

    python tests/golden/make_golden_bam.py --ref-bin <scratch>/bam-vaf-counter --index-bin <scratch>/bai-index

Writes tests/golden/bam/: five small .bam files (written by
tests/bam_fixture.py), the indexes the indexer wrote for three of them, the
pattern files, and manifest.json with, per case, the argv, the exit code, the
reference program's own stderr lines (htslib's [E::..] / [W::..] lines are
left out) and the .vaf it wrote, kept as the md5 of its bytes, its first line
and the "REF_COUNT ALT_COUNT" pairs of its rows.  A .vaf that an earlier case
(in name order) already holds is stored as "=<that case>".  The cases run in a
directory that bam_fixture.derive() makes of those files (the tests make the
same one): a.bam again as a_i.bam + a_i.bam.bai, a_j.bam + a_j.bai and a_k.bam
beside an index with a wrong magic, long.bam again as long_i.bam + its index,
and the damaged files d_*.bam cut from small.bam.  a.index and long.index are
the indexes under a name that no lookup finds.

The files:
  a.bam       600 records on chr1, chr2, chrM, coordinate-sorted: CIGARs of
              every op (P, B and a reserved code included) over a panel that
              is dense on chr1:100-180, so that rows sit at the first and last
              base of match blocks, inside D and N, right after I and S and at
              end - 1; odd l_seq; n_cigar = 0; l_seq = 0 without CIGAR; every
              skipped flag, secondary and supplementary; IUPAC and = bases;
              unplaced records at the end
  b.bam       other records under a header that orders the references
              chr2, chr1, chrM; indexed
  long.bam    a record of 5,000 CIGAR ops among short ones
  cg.bam      a record in the CG:B,I long-CIGAR convention
  small.bam   200 records in 1 KB blocks, the base of the damage cases:
              d_noeof (no EOF block), d_midblock (cut inside a block),
              d_border (cut at a block border inside a record), d_flip (one
              payload byte flipped), d_mismatch (a CIGAR / l_seq mismatch in
              the middle: the reference drops the record and reads on),
              d_mismatch_batch (the same after 1,000 good records: the
              reference's batch closes empty, once), d_mismatch_twice (two in
              a row: one empty batch again), d_mismatch_thrice (three in a
              row: the second empty batch ends the file), d_bs8 (a block_size
              of 8 in the middle: the words behind it fail twice)
  p.txt       the panel: dense, adjacent, duplicate and sparse rows, ref ==
              alt, lower-case and IUPAC alleles, a chromosome absent from the
              headers; p_empty.txt
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bam_fixture as F  # noqa: E402

OUT = os.path.join(HERE, "bam")
REFS = [("chr1", 3000), ("chr2", 2000), ("chrM", 500)]


def genome(rng):
    return {name: "".join("ACGT"[i] for i in rng.integers(0, 4, n)) for name, n in REFS}


def panel(rng, g):
    """[(chr, pos, rsid, ref, alt)] in file order (not sorted)."""
    rows = []

    def add(chr_, pos, ref=None, alt=None):
        ref = ref or g[chr_][pos] if chr_ in g else (ref or "A")
        alt = alt or "ACGT"[("ACGT".index(ref) + 1 + int(rng.integers(0, 3))) % 4] if ref in "ACGT" else (alt or "C")
        rows.append((chr_, pos, "rs%d" % len(rows), ref, alt))

    for pos in range(100, 180):
        add("chr1", pos)
    pos = 300
    while pos < 2900:
        add("chr1", pos)
        pos += int(rng.integers(1, 90))
    for pos in (400, 401, 402, 404, 700, 700, 701):      # adjacent and duplicate rows
        add("chr1", pos)
    pos = 50
    while pos < 1900:
        add("chr2", pos)
        pos += int(rng.integers(1, 120))
    for pos in range(10, 400, 37):
        add("chrM", pos)
    add("chrUn", 100)                                     # absent from every header
    add("chr1", 500, "A", "A")                            # ref == alt
    add("chr1", 501, "C", "C")
    add("chr1", 502, "g", "t")                            # lower case never matches
    add("chr1", 503, "a", "C")
    for pos, ref, alt in ((504, "N", "A"), (505, "R", "G"), (506, "=", "A"), (507, "A", "N"), (508, "Y", "="),
                          (120, "N", "="), (121, "M", "R")):
        add("chr1", pos, ref, alt)
    add("chrUn2", 5)
    order = rng.permutation(len(rows))                    # the file is not sorted
    return [rows[i] for i in order]


def pattern_text(rows):
    return "".join("%s\t%d\t%d\t%s\t%s\t%s\tA\tC\n"
                   % (c, p, p + 1, rs, ref, alt) for c, p, rs, ref, alt in rows)


def read_of(rng, g, chr_, pos, cigar, iupac=0.03):
    """The query of an alignment: the genome under M/=/X with a few changed
    bases, random bases under I and S."""
    out, cur = [], pos
    for w in F.cigar_words(cigar):
        op, n = w & 15, w >> 4
        if op in (0, 7, 8):
            for i in range(n):
                b = g[chr_][(cur + i) % len(g[chr_])]
                r = rng.random()
                if r < iupac:
                    b = F.NT16[int(rng.integers(0, 16))]
                elif r < 0.3:
                    b = "ACGT"[int(rng.integers(0, 4))]
                out.append(b)
            cur += n
        elif op in (1, 4):
            out.extend("ACGT"[i] for i in rng.integers(0, 4, n))
        elif op in (2, 3):
            cur += n
    return "".join(out)


FLAGS = (0, 16, 0, 99, 147, 0x100, 0x800, 0x4, 0x200, 0x400, 0x604, 0x900, 0, 16, 83, 163)


def records(rng, g, order, n, max_ops=9, seed_ops="MMMM=XIDNSHP"):
    """n records sorted by (tid in `order`, pos), then two unplaced ones."""
    recs = []
    for i in range(n):
        chr_ = order[int(rng.integers(0, 10)) % 3 if i % 7 else 0]
        tid = order.index(chr_)
        glen = len(g[chr_])
        pos = int(rng.integers(0, glen - 300)) if chr_ != "chr1" or i % 3 else int(rng.integers(40, 200))
        kind = i % 40
        flag = FLAGS[i % len(FLAGS)]
        if kind == 11:
            cigar, seq = [], read_of(rng, g, chr_, pos, [("M", 31)])     # n_cigar = 0, bases but no CIGAR
        elif kind == 23:
            cigar, seq = [], ""                                           # l_seq = 0 without CIGAR
        elif kind == 31:
            cigar = [("I", 5), ("S", 3)] if i % 80 == 31 else [("H", 4), ("P", 2)]   # no reference length: rlen 1
            seq = read_of(rng, g, chr_, pos, cigar)
        else:
            cigar = F.random_cigar(rng, 1 + int(rng.integers(0, max_ops)), 14, seed_ops)
            if kind in (5, 17):
                cigar.insert(1 + int(rng.integers(0, len(cigar))), (9 if kind == 5 else 13, 4))   # B, reserved
            if not F.query_len(cigar):
                cigar.append(("M", 7))
            if kind == 7 and F.query_len(cigar) % 2 == 0:
                cigar.append(("M", 1))                                    # odd l_seq: the last nibble
            seq = read_of(rng, g, chr_, pos, cigar)
        recs.append((tid, pos, F.record(tid, pos, flag, cigar, seq, name=b"q%d" % i)))
    recs.sort(key=lambda r: (r[0], r[1]))
    tail = [F.record(-1, -1, 0x4, [], "ACGTN", name=b"u1"), F.record(-1, -1, 0, [("M", 5)], "ACGTA", name=b"u2")]
    return [r[2] for r in recs] + tail


def long_record(rng, g, n_ops=5000):
    cigar = [("S", 3)]
    while len(cigar) < n_ops - 1:
        cigar.append(("MMM=XIDN"[int(rng.integers(0, 8))], int(rng.integers(1, 4))))
    cigar.append(("M", 2))
    big = {"chr1": g["chr1"] * 8}
    return F.record(0, 40, 0, cigar, read_of(rng, big, "chr1", 40, cigar), name=b"long")


def cg_record(rng, g):
    import struct
    real = [("S", 2), ("M", 30), ("D", 3), ("M", 20), ("I", 2), ("M", 40)]
    seq = read_of(rng, g, "chr1", 110, real)
    words = F.cigar_words(real)
    aux = b"NMC\x01" + b"CGBI" + struct.pack("<i%dI" % len(words), len(words), *words) + b"XSZab\0"
    fake = [("S", len(seq)), ("N", F.ref_len(real))]
    return F.record(0, 110, 0, fake, seq, name=b"cg", aux=aux)


def write(name, data):
    with open(os.path.join(OUT, name), "wb") as f:
        f.write(data if isinstance(data, bytes) else data.encode())


def make_inputs(rng):
    g = genome(rng)
    rows = panel(rng, g)
    write("p.txt", pattern_text(rows))
    write("p_empty.txt", "")
    order_a = [r[0] for r in REFS]
    write("a.bam", F.bam(REFS, records(rng, g, order_a, 600)))
    order_b = ["chr2", "chr1", "chrM"]
    write("b.bam", F.bam([(n, dict(REFS)[n]) for n in order_b], records(rng, g, order_b, 150)))
    short = records(rng, g, order_a, 60)
    lr = long_record(rng, g)
    at = next(i for i, r in enumerate(short) if struct.unpack_from("<ii", r, 4) >= (0, 40) or r[4:8] == b"\xff" * 4)
    write("long.bam", F.bam(REFS, short[:at] + [lr] + short[at:]))
    cg = records(rng, g, order_a, 20, max_ops=4)
    write("cg.bam", F.bam(REFS, [cg_record(rng, g)] + cg[-8:]))
    write("small.bam", F.bgzf(F.header(REFS) + b"".join(records(rng, g, order_a, 200)), 1024))


def cases():
    P = ["-p", "p.txt", "-o", "o/out.vaf"]
    c = {
        "noidx": P + ["a.bam"],
        "idx_bam_bai": P + ["a_i.bam"],
        "idx_bai": P + ["a_j.bam"],
        "idx_wrong_magic": P + ["a_k.bam"],
        "two_headers_noidx": P + ["a.bam", "b.bam"],
        "two_headers_idx": P + ["a_i.bam", "b.bam"],
        "two_headers_swapped": P + ["b.bam", "a_i.bam"],
        "missing_second": P + ["a.bam", "nope.bam", "b.bam"],
        "missing_first": P + ["nope.bam", "a.bam"],
        "opts_after_files": ["a.bam", "-t16", "b.bam", "-o", "o/out.vaf", "-pp.txt"],
        "empty_patterns": ["-p", "p_empty.txt", "-o", "o/out.vaf", "a.bam"],
        "missing_patterns": ["-p", "nope.txt", "-o", "o/out.vaf", "a.bam"],
        "usage_no_o": ["-p", "p.txt", "-t", "7", "a.bam"],
        "usage_no_files": P,
        "bad_outdir": ["-p", "p.txt", "-o", "nodir/out.vaf", "a.bam"],
        "long_noidx": P + ["long.bam"],
        "long_idx": P + ["long_i.bam"],
        "cg_tag": P + ["cg.bam"],
        "small": P + ["small.bam"],
    }
    for d in ("noeof", "midblock", "border", "flip", "mismatch", "mismatch_batch", "mismatch_twice", "mismatch_thrice", "bs8"):
        c["damage_" + d] = P + ["d_%s.bam" % d]
    c["damage_then_good"] = P + ["d_flip.bam", "small.bam"]
    return c


def own_lines(stderr: str) -> str:
    """The reference program's own lines: htslib's start with [E:: or [W::."""
    return "".join(ln + "\n" for ln in stderr.splitlines() if not re.match(r"\[[EWIDT]::", ln))


def vaf_entry(vaf: bytes):
    """A .vaf as the manifest keeps it: the md5 of its bytes, its first line,
    and the REF_COUNT ALT_COUNT pairs of its rows (in the order of p.txt; the
    other columns follow from them and from p.txt)."""
    lines = vaf.decode().splitlines()
    return {"md5": hashlib.md5(vaf).hexdigest(), "depth": lines[0],
            "counts": " ".join("%s %s" % tuple(ln.split("\t")[5:7]) for ln in lines[2:])}


def run_case(binary, argv, cwd):
    out_dir = os.path.join(cwd, "o")
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    p = subprocess.run([binary] + argv, cwd=cwd, capture_output=True, timeout=600)
    vaf = None
    if os.path.exists(os.path.join(out_dir, "out.vaf")):
        with open(os.path.join(out_dir, "out.vaf"), "rb") as f:
            vaf = f.read()
    shutil.rmtree(out_dir, ignore_errors=True)
    return p.returncode, p.stderr.decode(), vaf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference's bam-vaf-counter, built as the docstring says")
    ap.add_argument("--index-bin", required=True, help="a program that calls sam_index_build(file, 0) per argument")
    a = ap.parse_args()
    ref, indexer = os.path.abspath(a.ref_bin), os.path.abspath(a.index_bin)
    rng = np.random.default_rng(20261020)
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    make_inputs(rng)
    with tempfile.TemporaryDirectory() as tmp:          # the indexer writes FILE.bai beside FILE
        for fn in ("a.bam", "b.bam", "long.bam"):
            shutil.copy(os.path.join(OUT, fn), tmp)
        subprocess.run([indexer, "a.bam", "b.bam", "long.bam"], cwd=tmp, check=True)
        for fn, to in (("a.bam.bai", "a.index"), ("long.bam.bai", "long.index"), ("b.bam.bai", "b.bam.bai")):
            shutil.copy(os.path.join(tmp, fn), os.path.join(OUT, to))
    manifest, first = {}, {}
    with tempfile.TemporaryDirectory() as work:
        F.derive(OUT, work)
        for name, argv in sorted(cases().items()):
            rc, err, vaf = run_case(ref, argv, work)
            manifest[name] = {"argv": argv, "rc": rc, "stderr": own_lines(err)}
            if vaf is not None:
                manifest[name]["vaf"] = "=" + first[vaf] if vaf in first else vaf_entry(vaf)
                first.setdefault(vaf, name)
            print("%-22s rc=%d %s" % (name, rc, str(manifest[name].get("vaf"))[:60]))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    sizes = {fn: os.path.getsize(os.path.join(OUT, fn)) for fn in sorted(os.listdir(OUT))}
    print("fixture bytes: %d (largest %s); manifest md5 %s" % (
        sum(sizes.values()), max(sizes.items(), key=lambda kv: kv[1]),
        hashlib.md5(open(os.path.join(OUT, "manifest.json"), "rb").read()).hexdigest()))


if __name__ == "__main__":
    main()

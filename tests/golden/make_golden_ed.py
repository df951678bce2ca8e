#!/usr/bin/env python3
"""Golden fixtures for ed-vaf-counter from the REAL reference binary.  Build it
by hand from the reference's own Makefile rule (Makefile:46-47: CXX, -g -Wall
-O2 -std=c++11, ed-vaf-counter.c edlib.cpp, -lz -lstdc++) into a scratch
directory and pass its path:

    python tests/golden/make_golden_ed.py --ref-bin /path/to/ed-vaf-counter

Writes tests/golden/ed/: small pattern and read files and manifest.json with,
per case, the argv (run from tests/golden/ed/), the exit code, stderr and the
content of every file the reference wrote under o/.  A file whose content
another case (earlier in name order) already holds is stored as "=<that
case>" instead of the text again.

Cases: -e 0, 1, 2, 3, -1, a value >= m, "abc" and "2x"; query lengths 1, 21,
31, 32, 33, 64, 65, 127 one by one and mixed in one file; an alt_kmer longer
than its ref_kmer; reads of length 0, 1, m - 1, m, W - 1 and W (W = 64 *
ceil(m / 64) - m) with -e >= m and -e -1, where edlib reports an end location
-1 out of its padded last block; 150 bp reads with planted substitutions,
insertions and deletions; lower case and N; FASTA, multi-line FASTQ, a
truncated last record, gzip, two files, a missing file, an empty pattern
file, a row that stops fscanf; exact-repeat reads that give many locations;
argv: options after files, --oops, a missing -o, -e as the last word, "--".
No case has an alt_kmer shorter than its ref_kmer: the reference then reads
stale bytes of earlier rows.
"""
import argparse
import gzip
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ed")
LENGTHS = (1, 21, 31, 32, 33, 64, 65, 127)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def mutate(rng, s, n_sub=0, n_ins=0, n_del=0, alphabet="ACGT"):
    s = list(s)
    for _ in range(n_sub):
        if s:
            i = int(rng.integers(0, len(s)))
            s[i] = alphabet[(alphabet.index(s[i]) + 1 + int(rng.integers(0, len(alphabet) - 1))) % len(alphabet)] \
                if s[i] in alphabet else alphabet[0]
    for _ in range(n_ins):
        s.insert(int(rng.integers(0, len(s) + 1)), alphabet[int(rng.integers(0, len(alphabet)))])
    for _ in range(n_del):
        if len(s) > 1:
            del s[int(rng.integers(0, len(s)))]
    return "".join(s)


def pattern_rows(rng, m, n, tag, alphabet="ACGT", alt_extra=0):
    rows = []
    for i in range(n):
        ref = rand_seq(rng, m, alphabet)
        mid = m // 2
        alt_base = alphabet[(alphabet.index(ref[mid]) + 1) % len(alphabet)]
        alt = ref[:mid] + alt_base + ref[mid + 1:] + rand_seq(rng, alt_extra, alphabet)
        rows.append(("chr%d" % (1 + i % 22), 1000 + 17 * i, 1001 + 17 * i, "rs%s%d" % (tag, i),
                     ref[mid].upper() if ref[mid].upper() in "ACGT" else "A", alt_base.upper(), ref, alt))
    return rows


def pattern_text(rows):
    return "".join("%s\t%d\t%d\t%s\t%s\t%s\t%s\t%s\n" % r for r in rows)


def planted_reads(rng, rows, n_reads, read_len, alphabet="ACGT", edits=((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1),
                                                                           (2, 0, 0), (1, 1, 1), (3, 0, 0))):
    reads = []
    for i in range(n_reads):
        r = rows[int(rng.integers(0, len(rows)))]
        kmer = r[6] if rng.random() < 0.5 else r[7][:len(r[6])]
        sub, ins, dele = edits[i % len(edits)]
        ins_k = mutate(rng, kmer, sub, ins, dele, alphabet)
        L = max(read_len, len(ins_k))
        at = int(rng.integers(0, L - len(ins_k) + 1))
        body = rand_seq(rng, at, alphabet) + ins_k + rand_seq(rng, L - at - len(ins_k), alphabet)
        if i % 5 == 4:   # a second, exact copy: more than one location
            body = body + kmer
        reads.append(body)
    for i in range(max(2, n_reads // 8)):
        reads.append(rand_seq(rng, read_len, alphabet))
    return reads


def fastq(reads, multi=0):
    out = []
    for i, s in enumerate(reads):
        q = "I" * len(s)
        if multi and len(s) > multi:
            s = "\n".join(s[j:j + multi] for j in range(0, len(s), multi))
            q = "\n".join(q[j:j + multi] for j in range(0, len(q), multi))
        out.append("@r%d some comment\n%s\n+\n%s\n" % (i, s, q))
    return "".join(out)


def fasta(reads, width=60):
    return "".join(">s%d\n%s\n" % (i, "\n".join(s[j:j + width] for j in range(0, len(s), width)) if s else "")
                   for i, s in enumerate(reads))


def make_inputs(rng):
    files = {}
    by_len = {m: pattern_rows(rng, m, 3, "m%d_" % m) for m in LENGTHS}
    for m, rows in by_len.items():
        files["p_m%d.txt" % m] = pattern_text(rows)
    mixed = [r for m in (21, 1, 127, 32, 65, 31, 64, 33) for r in by_len[m][:2]]
    files["p_mixed.txt"] = pattern_text(mixed)
    p21 = pattern_rows(rng, 21, 12, "k")
    files["p21.txt"] = pattern_text(p21)
    files["p_altlong.txt"] = pattern_text(pattern_rows(rng, 21, 4, "al", alt_extra=7) +
                                          pattern_rows(rng, 33, 2, "al33_", alt_extra=40))
    low = pattern_rows(rng, 21, 3, "lo", alphabet="acgt") + pattern_rows(rng, 21, 3, "n", alphabet="ACGTN") + \
        pattern_rows(rng, 21, 2, "up")
    files["p_lower.txt"] = pattern_text(low)
    files["p_empty.txt"] = ""
    stop = pattern_text(p21[:2]) + "chr3\tnotanumber\t5\trsBAD\tA\tC\tACGT\tACTT\n" + pattern_text(p21[2:4])
    files["p_stop.txt"] = stop
    files["p_rep.txt"] = pattern_text([("chr1", 10, 11, "rsrep1", "A", "C", "AAA", "AAC"),
                                       ("chr1", 20, 21, "rsrep2", "A", "T", "ACACACAC", "ACACTCAC"),
                                       ("chr2", 30, 31, "rsrep3", "G", "A", "G", "A")])

    files["r150.fq"] = fastq(planted_reads(rng, p21, 21, 150))
    mix_reads = []
    for m in LENGTHS:
        mix_reads += planted_reads(rng, by_len[m], 3, max(90, m + 20))
    files["r_mix.fq"] = fastq(mix_reads)
    short = []
    for n in (0, 1, 2, 20, 21, 30, 31, 32, 33, 42, 43, 62, 63, 64, 65, 126, 127, 128):
        short.append(rand_seq(rng, n))
        src = by_len[127][0][6] + by_len[65][0][6]
        short.append(src[:n])                        # a prefix of a query
        short.append(by_len[21][0][6][:n] if n <= 21 else rand_seq(rng, n - 21) + by_len[21][0][6])
    files["r_short.fq"] = fastq(short)
    lower_reads = planted_reads(rng, low[:3], 8, 80, alphabet="acgt") + \
        planted_reads(rng, low[3:6], 8, 80, alphabet="ACGTN") + \
        [x.lower() for x in planted_reads(rng, low[6:], 4, 80)] + planted_reads(rng, low[6:], 4, 80)
    files["r_lower.fq"] = fastq(lower_reads)
    fa_reads = planted_reads(rng, p21, 10, 150) + [""] + planted_reads(rng, p21, 3, 30)
    files["r.fa"] = fasta(fa_reads)
    files["r_multi.fq"] = fastq(planted_reads(rng, p21, 10, 150), multi=50)
    tr = fastq(planted_reads(rng, p21, 8, 150))
    files["r_trunc.fq"] = tr[:len(tr) - 60]          # the last record's quality is cut short
    files["r_rep.fq"] = fastq(["A" * 30, "A" * 3, "AA", "AC" * 20, "AAAC" * 8, "G", "GGGG", "T" * 12, "",
                               "AAACAAAGAAAT", "CACACACACTCACACAC"])
    return files, {"r150.fq.gz": files["r150.fq"]}


def cases():
    P = ["-p", "p21.txt"]
    c = {}
    for e in ("0", "1", "2", "3", "-1", "25", "abc", "2x"):
        c["e_%s" % e.replace("-", "neg")] = P + ["-e", e, "-o", "o/out.vaf", "r150.fq"]
    c["e_default"] = P + ["-o", "o/out.vaf", "r150.fq"]
    c["e_glued"] = ["-pp21.txt", "-e1", "-oo/out.vaf", "r150.fq"]
    for m in LENGTHS:
        c["m%d_e2" % m] = ["-p", "p_m%d.txt" % m, "-e", "2", "-o", "o/out.vaf", "r_mix.fq"]
        c["m%d_short_ebig" % m] = ["-p", "p_m%d.txt" % m, "-e", str(m if m % 2 and m > 1 else 200), "-o", "o/out.vaf",
                                   "r_short.fq"]
        c["m%d_short_eneg" % m] = ["-p", "p_m%d.txt" % m, "-e", "-1", "-o", "o/out.vaf", "r_short.fq"]
        c["m%d_short_e1" % m] = ["-p", "p_m%d.txt" % m, "-e", "1", "-o", "o/out.vaf", "r_short.fq"]
    for e in ("0", "1", "3", "-1"):
        c["mixed_e%s" % e.replace("-", "neg")] = ["-p", "p_mixed.txt", "-e", e, "-o", "o/out.vaf", "r_mix.fq",
                                                  "r_short.fq"]
    c["altlong_e1"] = ["-p", "p_altlong.txt", "-e", "1", "-o", "o/out.vaf", "r150.fq", "r_mix.fq"]
    c["altlong_eneg"] = ["-p", "p_altlong.txt", "-e", "-1", "-o", "o/out.vaf", "r_short.fq"]
    c["lower_e0"] = ["-p", "p_lower.txt", "-o", "o/out.vaf", "r_lower.fq"]
    c["lower_e2"] = ["-p", "p_lower.txt", "-e", "2", "-o", "o/out.vaf", "r_lower.fq"]
    c["fasta_e1"] = P + ["-e", "1", "-o", "o/out.vaf", "r.fa"]
    c["multiline_e1"] = P + ["-e", "1", "-o", "o/out.vaf", "r_multi.fq"]
    c["trunc_e1"] = P + ["-e", "1", "-o", "o/out.vaf", "r_trunc.fq", "r_rep.fq"]
    c["gzip_e2"] = P + ["-e", "2", "-o", "o/out.vaf", "r150.fq.gz"]
    c["two_files_e1"] = P + ["-e", "1", "-o", "o/out.vaf", "r150.fq", "r.fa"]
    c["missing_file"] = P + ["-e", "1", "-o", "o/out.vaf", "nope.fq", "r150.fq", "also/nope.fq"]
    c["only_missing"] = P + ["-o", "o/out.vaf", "nope.fq"]
    c["missing_patterns"] = ["-p", "nope.txt", "-o", "o/out.vaf", "r150.fq"]
    c["empty_patterns"] = ["-p", "p_empty.txt", "-e", "1", "-o", "o/out.vaf", "r150.fq"]
    c["stop_row"] = ["-p", "p_stop.txt", "-e", "1", "-o", "o/out.vaf", "r150.fq"]
    for e in ("0", "1", "2", "3", "-1"):
        c["repeats_e%s" % e.replace("-", "neg")] = ["-p", "p_rep.txt", "-e", e, "-o", "o/out.vaf", "r_rep.fq"]
    c["opts_after_files"] = ["r150.fq", "-e", "1", "r.fa", "-o", "o/out.vaf", "-p", "p21.txt"]
    c["oops"] = ["--oops", "-p", "p21.txt", "-x", "-o", "o/out.vaf", "r150.fq"]
    c["cluster_unknown"] = ["-xe1", "-p", "p21.txt", "-o", "o/out.vaf", "r150.fq"]
    c["dashdash"] = P + ["-o", "o/out.vaf", "--", "r150.fq", "-e", "3"]
    c["dashdash_first"] = ["r150.fq", "--", "-p", "p21.txt", "-o", "o/out.vaf"]
    c["lone_dash"] = P + ["-o", "o/out.vaf", "-", "r150.fq"]
    c["usage_no_o"] = P + ["-e", "4", "r150.fq"]
    c["usage_no_files"] = P + ["-o", "o/out.vaf"]
    c["e_last_word"] = P + ["-o", "o/out.vaf", "r150.fq", "-e"]
    c["usage_o_last"] = P + ["r150.fq", "-o"]
    c["e_eats_option"] = P + ["-e", "-o", "o/out.vaf", "r150.fq"]
    c["usage_none"] = []
    c["bad_outdir"] = P + ["-o", "nodir/out.vaf", "r150.fq"]
    return c


def run_case(binary, argv, cwd):
    out_dir = os.path.join(cwd, "o")
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    p = subprocess.run([binary] + argv, cwd=cwd, capture_output=True, timeout=600)
    files = {}
    for fn in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, fn)) as f:
            files["o/" + fn] = f.read()
    shutil.rmtree(out_dir, ignore_errors=True)
    return p.returncode, p.stderr.decode(), files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference's ed-vaf-counter, built from its Makefile rule")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref_bin)
    rng = np.random.default_rng(20261019)
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    files, gz = make_inputs(rng)
    for name, text in files.items():
        with open(os.path.join(OUT, name), "w", newline="") as f:
            f.write(text)
    for name, text in gz.items():
        with open(os.path.join(OUT, name), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0,
                                                                      filename="") as g:
            g.write(text.encode())
    manifest, first = {}, {}
    for name, argv in sorted(cases().items()):
        rc, err, out = run_case(ref, argv, OUT)
        for fn, text in out.items():
            out[fn] = "=" + first[(fn, text)] if (fn, text) in first else text
            first.setdefault((fn, text), name)
        manifest[name] = {"argv": argv, "rc": rc, "stderr": err, "files": out}
        print("%-22s rc=%d files=%s" % (name, rc, sorted(out)))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    total = sum(os.path.getsize(os.path.join(d, fn)) for d, _, fs in os.walk(OUT) for fn in fs)
    print("fixture bytes: %d; manifest md5 %s" % (
        total, hashlib.md5(open(os.path.join(OUT, "manifest.json"), "rb").read()).hexdigest()))


if __name__ == "__main__":
    main()

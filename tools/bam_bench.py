#!/usr/bin/env python3
"""Throughput of bam-vaf-counter: the two kernels on descriptors resident in
HBM, and the CLI's wall clock on one synthetic BAM.

Kernel legs (default).  Panel: the first --patterns SNPs of the GRCh38 panel (0
= all 20,849), tids in BED order.  Records are synthetic descriptors made on
the host and copied to HBM once:

  short   147 to 150 bases, CIGARs 150M / 5S145M / 70M2D78M / 60M3I87M; a
          fraction --f-snp of the records is placed over a panel row, the
          rest uniformly over the chromosomes (whole-genome data has about
          one record in a thousand over a row of this panel)
  long    --long-ops CIGAR operations each (M / = / X of 1..8 bases between
          short I and D), every one placed over a panel row

One step = one vc_bam_count_device call; its time comes from HIP events around
the two launches (vc_bam_kernel_ms).  Steps are repeated --steps times after
--warmup and the median with its spread is reported, one JSON line per leg.
Each leg is run with all weights 1 and with the region weights of an indexed
file.  The counts of a sample must not depend on the long threshold.

CLI leg (--cli FILE.bam --cli-patterns FILE.txt): the wall clock of
lib/bam-vaf-counter -t 16 on that file, median of --steps runs.  --make-bam
writes such a file with tests/bam_fixture.py (no GPU needed), so that the
reference binary can be timed on the same bytes on a CPU host; this tool never
compares the kernel with itself.

    python tools/bam_bench.py [--patterns 0] [--records 4000000]
    python tools/bam_bench.py --make-bam /tmp/s.bam --make-patterns /tmp/p.txt --records 400000
    python tools/bam_bench.py --cli /tmp/s.bam --cli-patterns /tmp/p.txt
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmer-cnt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHORT_CIGARS = ([("M", 150)], [("S", 5), ("M", 145)], [("M", 70), ("D", 2), ("M", 78)], [("M", 60), ("I", 3), ("M", 87)])


def panel_rows(n_patterns):
    import vafc_synth as S
    rows = S.read_bed(S.default_bed_path())
    rows = [r for r in rows if len(r[4]) == 1 and len(r[5]) == 1 and r[4] in "ACGT" and r[5] in "ACGT"]
    return rows[:n_patterns] if n_patterns > 0 else rows


def write_patterns(rows, path):
    with open(path, "w") as f:
        for c, s, e, rs, ref, alt in rows:
            f.write("%s\t%d\t%d\t%s\t%s\t%s\tACGTACGTACGTACGTACGTA\tACGTACGTACCTACGTACGTA\n" % (c, s, e, rs, ref, alt))


def placements(rng, rows, names, n, f_snp, span):
    """(tid, pos) of n records: a fraction over a row, the rest anywhere."""
    tid_of = {c: i for i, c in enumerate(names)}
    r_tid = np.array([tid_of[r[0]] for r in rows], np.int32)
    r_pos = np.array([r[1] for r in rows], np.int64)
    chr_len = np.zeros(len(names), np.int64)
    np.maximum.at(chr_len, r_tid, r_pos + 1000)
    over = rng.random(n) < f_snp
    pick = rng.integers(0, len(rows), n)
    tid = np.where(over, r_tid[pick], rng.integers(0, len(names), n)).astype(np.int32)
    anywhere = (rng.random(n) * chr_len[tid]).astype(np.int64)
    pos = np.where(over, np.maximum(r_pos[pick] - rng.integers(0, span, n), 0), anywhere).astype(np.int32)
    return tid, pos


def short_records(rng, rows, names, n, f_snp):
    import bam_fixture as F
    import vafc
    tid, pos = placements(rng, rows, names, n, f_snp, 140)
    cls = rng.integers(0, 8, n) % 4 * (rng.random(n) < 0.3)        # 70 % plain 150M
    words = [F.cigar_words(c) for c in SHORT_CIGARS]
    n_cig = np.array([len(w) for w in words], np.uint32)[cls]
    l_seq = np.array([F.query_len(c) for c in SHORT_CIGARS], np.uint32)[cls]
    size = (4 * n_cig + (l_seq + 1) // 2 + 3) // 4 * 4
    off = np.concatenate(([0], np.cumsum(size, dtype=np.uint64)[:-1])).astype(np.uint64)
    data = np.zeros(int(size.sum()), np.uint8)
    data32 = data.view(np.uint32)
    bases = np.array([a << 4 | b for a in (1, 2, 4, 8) for b in (1, 2, 4, 8)], np.uint8)
    for k, w in enumerate(words):
        idx = np.nonzero(cls == k)[0]
        for j, word in enumerate(w):
            data32[(off[idx] >> np.uint64(2)).astype(np.int64) + j] = word
        nb = (F.query_len(SHORT_CIGARS[k]) + 1) // 2
        at = off[idx].astype(np.int64)[:, None] + 4 * len(w) + np.arange(nb)[None, :]
        data[at] = bases[rng.integers(0, 16, (idx.size, nb))]
    recs = np.zeros(n, vafc.BAM_REC)
    recs["tid"], recs["pos"], recs["n_cigar"], recs["l_seq"], recs["off"] = tid, pos, n_cig, l_seq, off
    recs["flag"] = np.where(rng.random(n) < 0.02, 0x400, 0)
    return recs, data


def long_records(rng, rows, names, n, n_ops):
    import vafc
    tid, pos = placements(rng, rows, names, n, 1.0, 2000)
    recs = np.zeros(n, vafc.BAM_REC)
    parts, at = [], 0
    bases = np.array([a << 4 | b for a in (1, 2, 4, 8) for b in (1, 2, 4, 8)], np.uint8)
    for i in range(n):
        op = np.array([0, 0, 0, 0, 0, 0, 7, 8, 1, 2], np.uint32)[rng.integers(0, 10, n_ops)]
        ln = np.where(op <= 2, rng.integers(1, 9, n_ops), rng.integers(1, 4, n_ops)).astype(np.uint32)
        ln = np.where((op == 1) | (op == 2), 1 + ln % 2, ln)
        w = (ln << np.uint32(4)) | op
        l_seq = int(ln[(op != 2)].sum())
        seq = bases[rng.integers(0, 16, (l_seq + 1) // 2)]
        blob = w.astype("<u4").tobytes() + seq.tobytes()
        blob += b"\0" * (-len(blob) % 4)
        recs[i] = (tid[i], pos[i], 0, n_ops, l_seq, 0, at)
        parts.append(blob)
        at += len(blob)
    return recs, np.frombuffer(b"".join(parts), np.uint8)


def region_arrays(vafc, db, names):
    tid_of = {c: i for i, c in enumerate(names)}
    regs = [(tid_of[c], s, e) for c, s, e in vafc.build_regions(db) if c in tid_of]
    return tuple(np.array(x, np.int32) for x in zip(*regs))


def kernel_legs(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("bam_bench: no GPU; a rate is only measured on one")
    import vafc
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    rows = panel_rows(a.patterns)
    names = list(dict.fromkeys(r[0] for r in rows))
    with tempfile.TemporaryDirectory() as tmp:
        pat = os.path.join(tmp, "p.txt")
        write_patterns(rows, pat)
        db = vafc.load_patterns(pat)
    bc = vafc.BamCounter(db, names)
    regions = region_arrays(vafc, db, names)
    stream = torch.cuda.current_stream().cuda_stream
    legs = (("short", short_records(rng, rows, names, a.records, a.f_snp)),
            ("short_targeted", short_records(rng, rows, names, a.records, 1.0)),
            ("long", long_records(rng, rows, names, a.long_records, a.long_ops)))
    for shape, (recs, data) in legs:
        d_recs = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
        d_data = torch.from_numpy(data.copy()).to(dev)
        torch.cuda.synchronize()

        def step(n=recs.size):
            bc.count_device(d_recs.data_ptr(), n, d_data.data_ptr(), data.size, stream)
            return bc.kernel_ms()

        # a sample through both kernels: the counts must not depend on the threshold
        m = min(recs.size, 2000)
        sample = []
        for thr in (64, 0, vafc.BAM_NEVER_LONG):
            bc.set_long_threshold(thr)
            bc.reset()
            step(m)
            sample.append(bc.finish())
        bc.set_long_threshold(64)
        same = bool(all(np.array_equal(sample[0], s) for s in sample[1:]))
        for weights in ("ones", "regions"):
            bc.set_regions(*(regions if weights == "regions" else ((), (), ())))
            for _ in range(a.warmup):
                step()
            bc.reset()
            ms = [step() for _ in range(a.steps)]
            counts = bc.finish().astype(np.uint64)
            med = float(np.median(ms))
            ops = int(recs["n_cigar"].astype(np.uint64).sum())
            print(json.dumps({
                "tool": "bam-vaf-counter", "what": "vc_bam_count_device, records resident in HBM, kernel time from HIP events",
                "shape": shape, "weights": weights, "patterns": db.n, "records": int(recs.size), "cigar_ops": ops,
                "data_bytes": int(data.size), "steps": a.steps, "warmup": a.warmup,
                "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
                "spread_pct": round(100.0 * (max(ms) - min(ms)) / med, 2),
                "value": round(recs.size / (med * 1e-3), 1), "unit": "records / s",
                "cigar_ops_per_s": round(ops / (med * 1e-3), 1),
                "counts_per_step": int(counts.sum() // np.uint64(a.steps)),
                "threshold_independent_sample": same,
            }), flush=True)
        del d_recs, d_data
    bc.close()


def make_bam(a):
    import bam_fixture as F
    rng = np.random.default_rng(2)
    rows = panel_rows(a.patterns)
    names = list(dict.fromkeys(r[0] for r in rows))
    write_patterns(rows, a.make_patterns)
    tid, pos = placements(rng, rows, names, a.records, a.f_snp, 140)
    order = np.lexsort((pos, tid))
    letters = np.array(list("ACGT"))
    refs = [(c, 250_000_000) for c in names]
    with open(a.make_bam, "wb") as f:
        text = [F.header(refs)]
        for n, i in enumerate(order):
            cigar = SHORT_CIGARS[int(rng.integers(0, 8)) % 4 if rng.random() < 0.3 else 0]
            seq = "".join(letters[rng.integers(0, 4, F.query_len(cigar))])
            text.append(F.record(int(tid[i]), int(pos[i]), 0, cigar, seq, name=b"read%d" % n))
            if len(text) >= 4096:
                f.write(F.bgzf(b"".join(text), eof=False, level=1))
                text = []
        f.write(F.bgzf(b"".join(text), level=1))
    print("wrote %s: %d records, %d bytes; %s: %d rows" % (a.make_bam, a.records, os.path.getsize(a.make_bam),
                                                          a.make_patterns, len(rows)))


def cli_leg(a):
    cli = os.path.join(ROOT, "kmer-cnt_amd", "lib", "bam-vaf-counter")
    secs = []
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.vaf")
        for _ in range(a.steps):
            t0 = time.perf_counter()
            p = subprocess.run([cli, "-p", a.cli_patterns, "-o", out, "-t", str(a.threads), a.cli], capture_output=True)
            secs.append(time.perf_counter() - t0)
            if p.returncode != 0:
                sys.exit("bam_bench: the CLI failed: " + p.stderr.decode()[-400:])
        with open(out, "rb") as f:
            vaf = f.read()
    import hashlib
    med = float(np.median(secs))
    print(json.dumps({
        "tool": "bam-vaf-counter", "what": "CLI wall clock, process start to exit, one synthetic BAM",
        "file_bytes": os.path.getsize(a.cli), "threads": a.threads, "steps": a.steps,
        "seconds_median": round(med, 3), "seconds_min": round(min(secs), 3), "seconds_max": round(max(secs), 3),
        "spread_pct": round(100.0 * (max(secs) - min(secs)) / med, 2),
        "vaf_first_line": vaf.split(b"\n")[0].decode(), "vaf_md5": hashlib.md5(vaf).hexdigest(),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=0, help="SNPs of the panel (0 = all)")
    ap.add_argument("--records", type=int, default=4_000_000, help="short records per step, or records of --make-bam")
    ap.add_argument("--f-snp", type=float, default=0.001, help="fraction of short records placed over a row")
    ap.add_argument("--long-records", type=int, default=4000)
    ap.add_argument("--long-ops", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--make-bam")
    ap.add_argument("--make-patterns")
    ap.add_argument("--cli")
    ap.add_argument("--cli-patterns")
    a = ap.parse_args()
    if a.make_bam:
        make_bam(a)
    elif a.cli:
        cli_leg(a)
    else:
        kernel_legs(a)


if __name__ == "__main__":
    main()

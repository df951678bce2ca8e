#!/usr/bin/env python3
"""Throughput of vcf-vaf-counter: the line-matching kernel on VCF text resident
in HBM, and the CLI's wall clock on one synthetic .vcf.gz.

Kernel legs (default).  Text: seeded WGS-shaped records of
tests/vcf_fixture.synth_vcf (GT:AD:DP sample columns; about 0.4 % of the lines
on a panel row with its alleles, as many on a row with other alleles), a chunk
of --chunk-lines lines made on the host and repeated on the device until it
holds at least --bytes.  Shapes: 1 sample per line (about 60 bytes a line) and
100 samples (about 1.2 KB).  Panels: the 20,849 SNPs of the GRCh38 panel, and
200,000 synthetic rows (vafc_synth.synthetic_bed).

One step = one vc_vcf_scan_device call over the whole text as a final block;
its time comes from HIP events around the launches (vc_vcf_kernel_ms: the
counter reset, the tail kernel and the scan kernel).  Steps are repeated
--steps times after --warmup; the median with its spread is reported, one JSON
line per leg, with bytes / s and the share of the 8 TB/s HBM peak (the
algorithm's bytes are the text, read once).  The lines reported by a step are
compared with the Python statement on the first chunk.

CLI leg (--cli FILE --cli-patterns FILE): the wall clock of lib/vcf-vaf-counter
on that file, median of --steps runs: a whole-program time (process start,
inflate, header, blocks, .vaf), not a kernel rate.  --make-vcf writes such a
file (no GPU needed), so that the reference binary can be timed on the same
bytes on a CPU host; this tool never compares the kernel with itself.

    python tools/vcf_bench.py [--bytes 1073741824]
    python tools/vcf_bench.py --make-vcf /tmp/s.vcf.gz --make-patterns /tmp/p.txt --lines 5000000
    python tools/vcf_bench.py --cli /tmp/s.vcf.gz --cli-patterns /tmp/p.txt
"""
import argparse
import gzip
import hashlib
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

HBM_PEAK = 8e12


def panel_rows(kind):
    """Rows as vcf_fixture.load_patterns gives them: (chr, start, rsid, ref, alt) in bytes."""
    import vafc_synth as S
    rows = S.read_bed(S.default_bed_path()) if kind == "grch38" else S.synthetic_bed(200_000)
    rows = [r for r in rows if len(r[4]) == 1 and len(r[5]) == 1 and r[4] in "ACGT" and r[5] in "ACGT"]
    return [(str(c).encode(), int(s), str(rs).encode(), str(ref).encode(), str(alt).encode()) for c, s, _e, rs, ref, alt in rows]


def write_patterns(rows, path):
    with open(path, "wb") as f:
        for c, s, rs, ref, alt in rows:
            f.write(b"%s\t%d\t%d\t%s\t%s\t%s\tACGTACGTACGTACGTACGTA\tACGTACGTACCTACGTACGTA\n" % (c, s, s + 1, rs, ref, alt))


def kernel_legs(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("vcf_bench: no GPU; a rate is only measured on one")
    import vafc
    import vcf_fixture as F
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    for panel in ("grch38", "synthetic200k"):
        rows = panel_rows(panel)
        index = F.first_rows(rows)
        m = vafc.VcfMatcher(rows=[(r[0], r[1], r[3], r[4]) for r in rows])
        for n_samples in (1, 100):
            lines = a.chunk_lines if n_samples == 1 else max(a.chunk_lines // 16, 1000)
            chunk = F.synth_vcf(rows, lines, n_samples, seed=3, header_too=False)
            reps = max(1, -(-a.bytes // len(chunk)))
            d_text = torch.from_numpy(np.frombuffer(chunk, np.uint8).copy()).to(dev).repeat(reps)
            torch.cuda.synchronize()
            total = len(chunk) * reps

            def step():
                m.scan_device(d_text.data_ptr(), total, 0, True, stream)
                ms = m.kernel_ms()
                return ms, m.hits()[0]

            want = F.device_lines(rows, chunk, 0, index)
            for _ in range(a.warmup):
                step()
            ms, hits = [], None
            for _ in range(a.steps):
                t, hits = step()
                ms.append(t)
            first = [(int(h["off"]), int(h["row"])) for h in hits[:len(want)]]
            med = float(np.median(ms))
            rate = total / (med * 1e-3)
            print(json.dumps({
                "tool": "vcf-vaf-counter", "what": "vc_vcf_scan_device, text resident in HBM, kernel time from HIP events",
                "panel": panel, "patterns": len(rows), "samples_per_line": n_samples, "text_bytes": total,
                "lines": lines * reps, "bytes_per_line": round(len(chunk) / lines, 1), "steps": a.steps, "warmup": a.warmup,
                "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
                "spread_pct": round(100.0 * (max(ms) - min(ms)) / med, 2),
                "value": round(rate / 1e9, 2), "unit": "GB of text / s", "lines_per_s": round(lines * reps / (med * 1e-3), 1),
                "share_of_hbm_peak_8TBps": round(rate / HBM_PEAK, 4),
                "lines_reported_per_step": int(hits.size), "first_chunk_equals_statement": first == want and hits.size == len(want) * reps,
            }), flush=True)
            del d_text
        m.close()


def make_vcf(a):
    import vcf_fixture as F
    rows = panel_rows("grch38")
    write_patterns(rows, a.make_patterns)
    step, md5, n_bytes = 250_000, hashlib.md5(), 0
    with gzip.open(a.make_vcf, "wb", compresslevel=1) as f:
        for i, first in enumerate(range(0, a.lines, step)):
            part = F.synth_vcf(rows, min(step, a.lines - first), a.samples, seed=100 + i, header_too=(i == 0))
            f.write(part)
            md5.update(part)
            n_bytes += len(part)
    print("wrote %s: %d lines, %d bytes of text (md5 %s), %d bytes; %s: %d rows" % (
        a.make_vcf, a.lines, n_bytes, md5.hexdigest(), os.path.getsize(a.make_vcf), a.make_patterns, len(rows)))


def cli_leg(a):
    cli = os.path.join(ROOT, "kmer-cnt_amd", "lib", "vcf-vaf-counter")
    secs = []
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.vaf")
        for _ in range(a.steps):
            t0 = time.perf_counter()
            p = subprocess.run([cli, "-p", a.cli_patterns, "-v", a.cli, "-o", out], capture_output=True)
            secs.append(time.perf_counter() - t0)
            if p.returncode != 0:
                sys.exit("vcf_bench: the CLI failed: " + p.stderr.decode()[-400:])
        with open(out, "rb") as f:
            vaf = f.read()
    med = float(np.median(secs))
    print(json.dumps({
        "tool": "vcf-vaf-counter", "what": "CLI wall clock, process start to exit, one synthetic .vcf.gz (whole program, not a kernel rate)",
        "file_bytes": os.path.getsize(a.cli), "steps": a.steps,
        "seconds_median": round(med, 3), "seconds_min": round(min(secs), 3), "seconds_max": round(max(secs), 3),
        "spread_pct": round(100.0 * (max(secs) - min(secs)) / med, 2),
        "vaf_first_line": vaf.split(b"\n")[0].decode(), "vaf_md5": hashlib.md5(vaf).hexdigest(),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30, help="text resident in HBM per step, at least")
    ap.add_argument("--chunk-lines", type=int, default=200_000, help="lines of the chunk that is repeated")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lines", type=int, default=5_000_000, help="lines of --make-vcf")
    ap.add_argument("--samples", type=int, default=1, help="sample columns of --make-vcf")
    ap.add_argument("--make-vcf")
    ap.add_argument("--make-patterns")
    ap.add_argument("--cli")
    ap.add_argument("--cli-patterns")
    a = ap.parse_args()
    if a.make_vcf:
        make_vcf(a)
    elif a.cli:
        cli_leg(a)
    else:
        kernel_legs(a)


if __name__ == "__main__":
    main()

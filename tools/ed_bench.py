#!/usr/bin/env python3
"""Throughput of the approximate pattern search (ed-vaf-counter's hot path,
vc_ed_count_device) on one GPU.

Workload: the first --patterns SNPs of the GRCh38 panel (0 = all 20,849) as
ref/alt k-mers of length --k, searched with edit bound --e in reads of
--read-len bases generated on the device by the vafc_synth generator
(vc_synth_reads) and left resident in HBM.  One step = one vc_ed_count_device
call over all reads; its kernel time comes from HIP events around the launches
(vc_ed_kernel_ms).  The read count is sized so that a step lasts about
--target-ms, steps are repeated --steps times after --warmup, and the median
with its spread is reported.

The figure is read-bases x queries per second (every query is advanced by one
table column per read base), and the same times the query length as cell
updates per second.  The CPU comparison point is the reference binary timed on
a CPU host; this tool never compares the kernel with
itself.  A sample of the counts (-e 0: exact forward occurrences) is checked
on the host.

    python tools/ed_bench.py [--patterns 2000] [--k 21] [--e 2]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmer-cnt_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=2000, help="SNPs of the panel (0 = all)")
    ap.add_argument("--k", type=int, default=21, help="query length (1..127)")
    ap.add_argument("--e", type=int, default=2, help="edit bound (-e)")
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reads", type=int, default=0, help="reads per step (0 = sized for --target-ms)")
    ap.add_argument("--target-ms", type=float, default=400.0)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--f-snp", type=float, default=0.5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ed_bench: no GPU; a rate is only measured on one")
    import vafc
    import vafc_synth as S
    dev = torch.device("cuda", 0)
    rows = S.read_bed(S.default_bed_path())
    panel = S.make_panel(rows[:a.patterns] if a.patterns > 0 else rows)
    L = a.read_len
    win = torch.from_numpy(panel.windows().reshape(-1)).to(dev)
    dos = torch.from_numpy(panel.dosage.astype(np.uint8)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def gen(n):
        seq = torch.empty(n * L, dtype=torch.uint8, device=dev)
        offs = torch.empty(n, dtype=torch.int64, device=dev)
        lens = torch.empty(n, dtype=torch.int32, device=dev)
        vafc.synth_reads(seq.data_ptr(), offs.data_ptr(), lens.data_ptr(), 0, n, L, S.READ_SEED_R1, a.f_snp,
                         win.data_ptr(), dos.data_ptr(), panel.n, stream)
        torch.cuda.synchronize()
        return seq, offs, lens

    with tempfile.TemporaryDirectory() as tmp:
        pat = os.path.join(tmp, "p.txt")
        panel.write_patterns(pat, a.k)
        db = vafc.load_patterns(pat)
    ed = vafc.EdCounter(db, a.e)
    n_queries = 2 * db.n

    def step(bufs, n):
        ed.count_device(bufs[0].data_ptr(), n * L, bufs[1].data_ptr(), bufs[2].data_ptr(), n, stream)
        return ed.kernel_ms()

    n = a.reads
    if n <= 0:       # size the step from a small probe (after one call that loads the code object)
        probe = 4096
        bufs = gen(probe)
        step(bufs, probe)
        ms = min(step(bufs, probe) for _ in range(3))
        n = int(min(max(probe * a.target_ms / max(ms, 1e-3), probe), 4_000_000))
        del bufs
    bufs = gen(n)
    for _ in range(a.warmup):
        step(bufs, n)
    ed.reset()
    ms = [step(bufs, n) for _ in range(a.steps)]
    counts = ed.finish().astype(np.uint64) // np.uint64(a.steps)

    # host check of a sample: with -e 0 a count is the number of exact forward occurrences
    check = None
    if a.e == 0:
        m = min(n, 300)
        sample = bufs[0][:m * L].cpu().numpy().tobytes()
        ed.reset()
        ed.count_device(bufs[0].data_ptr(), m * L, bufs[1].data_ptr(), bufs[2].data_ptr(), m, stream)
        got = ed.finish()
        reads = [sample[i * L:(i + 1) * L] for i in range(m)]
        ok = True
        for q in range(0, min(n_queries, 200)):
            rec = db.record(q // 2)
            kmer = rec[5 + (q & 1)][:a.k]
            want = sum(sum(1 for j in range(L - a.k + 1) if r[j:j + a.k] == kmer) for r in reads)
            ok = ok and int(got[q]) == want
        check = bool(ok)
    ed.close()

    med = float(np.median(ms))
    cols = float(n) * L * n_queries
    line = {
        "tool": "ed-vaf-counter", "what": "vc_ed_count_device, reads resident in HBM, kernel time from HIP events",
        "patterns": db.n, "queries": n_queries, "k": a.k, "e": a.e, "reads": n, "read_len": L,
        "steps": a.steps, "warmup": a.warmup,
        "kernel_ms_median": round(med, 3), "kernel_ms_min": round(min(ms), 3), "kernel_ms_max": round(max(ms), 3),
        "spread_pct": round(100.0 * (max(ms) - min(ms)) / med, 2),
        "value": round(cols / (med * 1e-3), 1), "unit": "read-bases x queries / s",
        "cell_updates_per_s": round(cols * a.k / (med * 1e-3), 1),
        "hits_per_step": int(counts.sum()),
        "exact_sample_check": check,
    }
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

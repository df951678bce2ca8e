#!/usr/bin/env python3
"""Throughput of the device's BAM text scan (vc_bam_scan_text_device): finding
the records (guess + link + emit), checking them, and counting them where they
lie, each from HIP events, on text resident in HBM.

The text: a seeded chunk of whole 150-bp records (tests/bam_fixture.record;
positions and CIGARs as tools/bam_bench.py's short leg, over the GRCh38 panel)
repeated until it holds at least --bytes.  Two shapes of cuts:

    aligned   every member ends where a record ends (what htslib writes): the
              cuts are record starts, at most 65,280 bytes apart
    straddle  a cut every 65,280 bytes, wherever that falls

One step = one vc_bam_scan_text_device call; --steps steps after --warmup, the
median of each part with its spread, as GB of text / s and records / s, one
JSON line per shape.  The counts of a step must be those of the host reader's
descriptors of the same records through vc_bam_count_device.

Beside each shape: the inflate kernel's rate on the same members (level 6, the
method of tools/bgzf_bench.py), and the host pass's rate on the same file
(vc_bam_count_file under VAFC_BGZF=host at --host-threads threads, a host clock
around the call, best of three).

    python tools/bam_text_bench.py [--bytes 1073741824] [--out profiles/bam_text_bench_v1.jsonl]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmer-cnt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PAYLOAD = 65280


def chunk_records(rows, names, n, seed=5):
    import bam_bench as BB
    import bam_fixture as F
    rng = np.random.default_rng(seed)
    tid, pos = BB.placements(rng, rows, names, n, 0.001, 140)
    order = np.lexsort((pos, tid))
    letters = np.array(list("ACGT"))
    out = []
    for k, i in enumerate(order):
        cigar = BB.SHORT_CIGARS[int(rng.integers(0, 8)) % 4 if rng.random() < 0.3 else 0]
        seq = "".join(letters[rng.integers(0, 4, F.query_len(cigar))])
        out.append(F.record(int(tid[i]), int(pos[i]), 0x400 if rng.random() < 0.02 else 0, cigar, seq,
                            name=b"A00123:45:HXXXXXXXX:1:1101:%d" % k, aux=b"NMC\x01ASC\x96"))
    return out


def member_starts(records, aligned):
    """Text offsets at which the chunk's members start (the first at 0)."""
    total = sum(len(r) for r in records)
    if not aligned:
        return list(range(0, total, PAYLOAD))
    starts, at, begin = [0], 0, 0
    for r in records:
        if at + len(r) - begin > PAYLOAD:
            starts.append(at)
            begin = at
        at += len(r)
    return starts


def bgzf_member(piece, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = c.compress(piece) + c.flush()
    total = 18 + len(comp) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + (total - 1).to_bytes(2, "little") + comp +
            zlib.crc32(piece).to_bytes(4, "little") + len(piece).to_bytes(4, "little")), len(comp)


def spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30, help="text in HBM, at least")
    ap.add_argument("--chunk-records", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--shapes", default="aligned,straddle")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bam_text_bench: no GPU; a rate is only measured on one")
    import bam_bench as BB
    import bam_fixture as F
    import vafc
    dev = torch.device("cuda", 0)
    rows = BB.panel_rows(0)
    names = list(dict.fromkeys(r[0] for r in rows))
    records = chunk_records(rows, names, a.chunk_records)
    chunk = b"".join(records)
    reps = max(1, -(-a.bytes // len(chunk)))
    n_text, n_recs = len(chunk) * reps, len(records) * reps
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as tmp:
        pat = os.path.join(tmp, "p.txt")
        BB.write_patterns(rows, pat)
        db = vafc.load_patterns(pat)
        bc = vafc.BamCounter(db, names)
        z = vafc.BgzfInflater()
        d_text = torch.from_numpy(np.frombuffer(chunk, np.uint8).copy()).to(dev).repeat(reps)
        stream = torch.cuda.current_stream().cuda_stream
        lines = []
        for shape in a.shapes.split(","):
            starts = np.array(member_starts(records, shape == "aligned"), np.uint64)
            cuts = (np.tile(starts, reps) + np.repeat(np.arange(reps, dtype=np.uint64), starts.size) * np.uint64(len(chunk)))[1:]
            d_cuts = torch.from_numpy(cuts.view(np.int64).copy()).to(dev)
            torch.cuda.synchronize()
            find, check, count = [], [], []
            for step in range(a.warmup + a.steps):
                bc.reset()
                bc.scan_text_device(d_text.data_ptr(), n_text, 0, d_cuts.data_ptr(), cuts.size, True, stream)
                res = bc.text_result()
                if (res.consumed, res.records, res.irregular, res.short_stop) != (n_text, n_recs, 0, 0):
                    sys.exit("bam_text_bench: the scan found %d of %d records, consumed %d of %d" % (
                        res.records, n_recs, res.consumed, n_text))
                if step >= a.warmup:
                    f, c = bc.text_kernel_ms()
                    find.append(f)
                    check.append(c)
                    count.append(bc.kernel_ms())
            got = bc.finish()
            rewalked = res.rewalked
            # the same members compressed: the inflate kernel's rate, and a file for the host pass
            ends = list(starts[1:]) + [len(chunk)]
            parts, blocks, at = [], [], 0
            for s, e in zip(starts, ends):
                m, n_comp = bgzf_member(chunk[int(s):int(e)])
                parts.append(m)
                blocks.append((at + 18, n_comp, int(e - s), int(s), zlib.crc32(chunk[int(s):int(e)]), 0))
                at += len(m)
            raw, blocks = b"".join(parts), np.array(blocks, dtype=vafc.BGZF_BLOCK)
            all_blocks = np.tile(blocks, reps)
            rep_of = np.repeat(np.arange(reps, dtype=np.uint64), len(blocks))
            all_blocks["in_off"] += rep_of * np.uint64(len(raw))
            all_blocks["out_off"] += rep_of * np.uint64(len(chunk))
            d_raw = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev).repeat(reps)
            d_blk = torch.from_numpy(all_blocks.view(np.uint8).copy()).to(dev)
            d_out = torch.zeros(n_text, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            inflate = []
            for step in range(a.warmup + a.steps):
                z.inflate_device(d_raw.data_ptr(), d_raw.numel(), d_blk.data_ptr(), len(all_blocks), d_out.data_ptr(), n_text)
                status, ok = z.status()
                if ok != len(all_blocks):
                    sys.exit("bam_text_bench: block %d has status %d" % (ok, status[ok]))
                if step >= a.warmup:
                    inflate.append(z.kernel_ms())
            if not torch.equal(d_out, d_text):
                sys.exit("bam_text_bench: the inflated text differs")
            del d_raw, d_blk, d_out
            path = os.path.join(tmp, shape + ".bam")
            with open(path, "wb") as f:
                f.write(F.bgzf(F.header([(c, 250_000_000) for c in names]), eof=False))
                for _ in range(reps):
                    f.write(raw)
                f.write(F.EOF_BLOCK)
            os.environ["VAFC_BGZF"] = "host"
            host = []
            for _ in range(3):
                bc.reset()
                t0 = time.perf_counter()
                st = bc.count_file(path, a.host_threads)
                host.append(time.perf_counter() - t0)
                if st.seqs != n_recs:
                    sys.exit("bam_text_bench: the host pass read %d of %d records" % (st.seqs, n_recs))
            same = bool(np.array_equal(bc.finish(), got))
            os.unlink(path)

            def rates(ms):
                med, lo, hi = spread(ms)
                return dict(ms_median=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                            text_GBps=round(n_text / med / 1e6, 2), records_per_s=round(n_recs / med * 1e3, 1))

            line = dict(tool="bam_text_bench", shape=shape, text_bytes=n_text, records=n_recs, segments=int(cuts.size + 1),
                        rewalked=int(rewalked), steps=a.steps, warmup=a.warmup, find=rates(find), check=rates(check),
                        count=rates(count), inflate=rates(inflate), compressed_bytes=len(raw) * reps,
                        host_threads=a.host_threads, host_seconds_best=round(min(host), 3),
                        host_seconds_all=[round(h, 3) for h in host], host_text_GBps=round(n_text / min(host) / 1e9, 3),
                        host_records_per_s=round(n_recs / min(host), 1), counts_equal_host_pass=same,
                        counts_per_step=int(got.astype(np.uint64).sum()))
            print(json.dumps(line), flush=True)
            lines.append(line)
            if not same:
                sys.exit("bam_text_bench: the counts differ from the host pass's")
        bc.close()
        z.close()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

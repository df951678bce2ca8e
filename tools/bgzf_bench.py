#!/usr/bin/env python3
"""Throughput of the device BGZF inflater: the kernel alone, on text resident
in HBM as compressed members, and the host reader's rate on the same bytes.

Input: a seeded chunk of text, cut into members of 65,280 bytes of text (what
bgzip writes), compressed on the host with zlib at the leg's level, and the
compressed chunk repeated on the device until the members hold at least
--bytes of text (as tools/vcf_bench.py repeats its chunk).  Shapes:

    fastq_l1, fastq_l6   150-bp FASTQ records (seeded bases and qualities)
    vcf1_l6              WGS-shaped VCF lines with one sample column
    vcf100_l6            ... with 100 sample columns

One step = one vc_bgzf_inflate_device call over all members; its time comes
from HIP events around the kernel (vc_bgzf_kernel_ms).  --steps steps after
--warmup; the median with its spread, as GB/s of text and of compressed bytes,
one JSON line per leg.  Every block's status is 0 and the first and last
chunk's text are compared with the input.

Beside each leg goes the host's rate on the same members on the same machine:
the members written to a file and read through the project's host reader
(vc_gz_inflate_parallel, what vcf-vaf-counter's host path reads BGZF with) at
--host-threads threads, a host clock around the whole read, best of three.

    python tools/bgzf_bench.py [--bytes 1073741824] [--out profiles/bgzf_bench_v1.jsonl]
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

PAYLOAD = 65280


def fastq_chunk(n_bytes, seed=7, read_len=150):
    rng = np.random.default_rng(seed)
    n = n_bytes // (2 * read_len + 30) + 1
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, read_len))]
    quals = np.frombuffer(b"FFFFFFFF:,#", np.uint8)[rng.integers(0, 11, (n, read_len))]
    out = []
    for i in range(n):
        out.append(b"@SRR000001.%d %d/1\n%s\n+\n%s\n" % (i + 1, i + 1, bases[i].tobytes(), quals[i].tobytes()))
    return b"".join(out)[:n_bytes]


def vcf_chunk(n_bytes, n_samples):
    import vcf_fixture as F
    import vafc_synth as S
    rows = [(str(c).encode(), int(s), str(rs).encode(), str(ref).encode(), str(alt).encode())
            for c, s, _e, rs, ref, alt in S.read_bed(S.default_bed_path()) if len(ref) == 1 and len(alt) == 1]
    per_line = 60 if n_samples == 1 else 12 * n_samples + 60
    return F.synth_vcf(rows, n_bytes // per_line + 1, n_samples, seed=3, header_too=False)[:n_bytes]


def members_of(text, level):
    """(the members as bytes, descriptors relative to them) of text cut every PAYLOAD bytes."""
    import vafc
    parts, blocks = [], []
    at = out = 0
    for i in range(0, len(text), PAYLOAD):
        piece = text[i:i + PAYLOAD]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = c.compress(piece) + c.flush()
        total = 18 + len(comp) + 8
        parts.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + (total - 1).to_bytes(2, "little") + comp +
                     zlib.crc32(piece).to_bytes(4, "little") + len(piece).to_bytes(4, "little"))
        blocks.append((at + 18, len(comp), len(piece), out, zlib.crc32(piece), 0))
        at += total
        out += len(piece)
    return b"".join(parts), np.array(blocks, dtype=vafc.BGZF_BLOCK)


def spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30, help="text held by the members in HBM, at least")
    ap.add_argument("--chunk-members", type=int, default=64, help="members of the chunk that is repeated")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--legs", default="fastq_l1,fastq_l6,vcf1_l6,vcf100_l6")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bgzf_bench: no GPU; a rate is only measured on one")
    import vafc
    dev = torch.device("cuda", 0)
    z = vafc.BgzfInflater()
    n_chunk = a.chunk_members * PAYLOAD
    lines = []
    for leg in a.legs.split(","):
        shape, level = leg.rsplit("_l", 1)
        text = fastq_chunk(n_chunk) if shape == "fastq" else vcf_chunk(n_chunk, 1 if shape == "vcf1" else 100)
        raw, blocks = members_of(text, int(level))
        reps = max(1, -(-a.bytes // len(text)))
        all_blocks = np.tile(blocks, reps)
        rep_of = np.repeat(np.arange(reps, dtype=np.uint64), len(blocks))
        all_blocks["in_off"] += rep_of * np.uint64(len(raw))
        all_blocks["out_off"] += rep_of * np.uint64(len(text))
        d_raw = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev).repeat(reps)
        d_blk = torch.from_numpy(all_blocks.view(np.uint8).copy()).to(dev)
        n_text = len(text) * reps
        d_out = torch.zeros(n_text, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ms = []
        for step in range(a.warmup + a.steps):
            z.inflate_device(d_raw.data_ptr(), d_raw.numel(), d_blk.data_ptr(), len(all_blocks), d_out.data_ptr(), n_text)
            status, ok = z.status()
            if ok != len(all_blocks):
                sys.exit("bgzf_bench: block %d has status %d" % (ok, status[ok]))
            if step >= a.warmup:
                ms.append(z.kernel_ms())
        want = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)
        if not (torch.equal(d_out[:len(text)], want) and torch.equal(d_out[-len(text):], want)):
            sys.exit("bgzf_bench: the text differs from the input")
        # the host reader on the same members
        with tempfile.NamedTemporaryFile(suffix=".gz", dir=os.environ.get("TMPDIR")) as f:
            for _ in range(reps):
                f.write(raw)
            f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0\0\0\0\0\0\0\0\0")
            f.flush()
            host, out, st = [], np.empty(n_text + 1, np.uint8), np.zeros(6, np.uint64)
            for _ in range(3):
                t0 = time.perf_counter()
                got = vafc.lib().vc_gz_inflate_parallel(f.name.encode(), a.host_threads, 4 << 20, out.ctypes.data, n_text + 1,
                                                        st.ctypes.data)
                host.append(time.perf_counter() - t0)
                if got != n_text:
                    sys.exit("bgzf_bench: the host reader gave %d bytes of %d" % (got, n_text))
            del out
        med, lo, hi = spread(ms)
        line = dict(tool="bgzf_bench", leg=leg, members=len(all_blocks), text_bytes=n_text, compressed_bytes=int(d_raw.numel()),
                    ratio=round(n_text / d_raw.numel(), 3), steps=a.steps, warmup=a.warmup,
                    kernel_ms_median=round(med, 3), kernel_ms_min=round(lo, 3), kernel_ms_max=round(hi, 3),
                    text_GBps=round(n_text / med / 1e6, 2), text_GBps_min=round(n_text / hi / 1e6, 2),
                    text_GBps_max=round(n_text / lo / 1e6, 2), compressed_GBps=round(d_raw.numel() / med / 1e6, 2),
                    host_threads=a.host_threads, host_seconds_best=round(min(host), 3), host_seconds_all=[round(h, 3) for h in host],
                    host_text_GBps=round(n_text / min(host) / 1e9, 3))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del d_raw, d_blk, d_out, want
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    z.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The piece walk alone (vc_bam_scan_pieces_device, bam_piece_walk_kernel): HIP
events around single launches, on text resident in HBM; the sibling of
tools/bam_text_bench.py, whose text it uses.

The text: that tool's seeded chunk of whole 150-bp records, repeated until it
holds at least --bytes, cut into members where records end (at most 65,280
bytes apart).  Shapes of pieces:

    members   one piece per member, the whole text walked: the same work as
              the text scan's guess + link + emit
    panel     pieces of three members each, one behind the other, at most
              20,849 of them (the panel's size; a third of the members where
              the text holds fewer): what a seeking pass hands the kernel
    sparse    every eighth member as a piece of its own

One step = one vc_bam_scan_pieces_device call; --steps steps after --warmup,
the median of walk, check and count with min and max, one JSON line per
shape.  Every step must find exactly the records the pieces hold.

    python tools/bam_pieces_bench.py [--bytes 1073741824] [--out profiles/bam_pieces_bench_v1.jsonl]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmer-cnt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30, help="text in HBM, at least")
    ap.add_argument("--chunk-records", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="members,panel,sparse")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bam_pieces_bench: no GPU; a rate is only measured on one")
    import bam_bench as BB
    import bam_text_bench as TB
    import vafc
    dev = torch.device("cuda", 0)
    rows = BB.panel_rows(0)
    names = list(dict.fromkeys(r[0] for r in rows))
    records = TB.chunk_records(rows, names, a.chunk_records)
    chunk = b"".join(records)
    reps = max(1, -(-a.bytes // len(chunk)))
    n_text = len(chunk) * reps
    rec_starts = np.cumsum([0] + [len(r) for r in records[:-1]]).astype(np.uint64)
    starts = np.array(TB.member_starts(records, True), np.uint64)
    rep_of = np.repeat(np.arange(reps, dtype=np.uint64), starts.size) * np.uint64(len(chunk))
    edges = np.concatenate([np.tile(starts, reps) + rep_of, np.array([n_text], np.uint64)])     # every member's start, then the end
    recs_upto = np.concatenate([np.searchsorted(rec_starts, starts), [len(records)]])         # records before each member of a chunk
    per_member = np.tile(np.diff(recs_upto), reps)
    cum = np.concatenate([[0], np.cumsum(per_member)])
    n_members = edges.size - 1
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as tmp:
        pat = os.path.join(tmp, "p.txt")
        BB.write_patterns(rows, pat)
        db = vafc.load_patterns(pat)
        bc = vafc.BamCounter(db, names)
        d_text = torch.from_numpy(np.frombuffer(chunk, np.uint8).copy()).to(dev).repeat(reps)
        stream = torch.cuda.current_stream().cuda_stream
        lines = []
        for shape in a.shapes.split(","):
            if shape == "members":
                first, span = np.arange(n_members), 1
            elif shape == "panel":
                first, span = np.arange(0, n_members - 2, 3)[:len(rows)], 3
            elif shape == "sparse":
                first, span = np.arange(0, n_members, 8), 1
            else:
                sys.exit("bam_pieces_bench: no shape " + shape)
            first = np.unique(first)
            pieces = np.zeros(first.size, vafc.BAM_PIECE)
            pieces["entry"] = edges[first]
            pieces["stop"] = pieces["limit"] = edges[first + span]
            n_recs = int((cum[first + span] - cum[first]).sum())
            n_bytes = int((pieces["limit"] - pieces["entry"]).sum())
            d_pieces = torch.from_numpy(pieces.view(np.uint8).copy()).to(dev)
            torch.cuda.synchronize()
            walk, check, count = [], [], []
            for step in range(a.warmup + a.steps):
                bc.reset()
                bc.scan_pieces_device(d_text.data_ptr(), n_text, d_pieces.data_ptr(), pieces.size, stream)
                res, _status, _offs = bc.pieces_result()
                if (res.records, res.found, res.irregular, res.n_short, res.n_cut, res.n_noroom) != (n_recs, n_recs, 0, 0, 0, 0):
                    sys.exit("bam_pieces_bench: %s found %d of %d records (cut %d, short %d)" % (
                        shape, res.records, n_recs, res.n_cut, res.n_short))
                if step >= a.warmup:
                    w, c = bc.text_kernel_ms()
                    walk.append(w)
                    check.append(c)
                    count.append(bc.kernel_ms())
            got = bc.finish()

            def rates(ms):
                med, lo, hi = spread(ms)
                return dict(ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                            walked_GBps=round(n_bytes / med / 1e6, 2), records_per_s=round(n_recs / med * 1e3, 1))

            line = dict(tool="bam_pieces_bench", shape=shape, text_bytes=n_text, pieces=int(pieces.size),
                        members_per_piece=span, walked_bytes=n_bytes, records=n_recs, steps=a.steps, warmup=a.warmup,
                        walk=rates(walk), check=rates(check), count=rates(count),
                        counts_per_step=int(got.astype(np.uint64).sum()))
            print(json.dumps(line), flush=True)
            lines.append(line)
        bc.close()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

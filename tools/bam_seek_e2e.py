#!/usr/bin/env python3
"""End to end: bam-vaf-counter on one coordinate-sorted BGZF BAM beside a BAI,
reading by the index (VAFC_BAM_INDEX=seek) against the same build without the
variable and against the parent commit's binary, alternating in one call.

The file: a BAM header, then tools/bam_text_bench.chunk_records' seeded 150-bp
records over the GRCh38 panel in coordinate order, each written --repeat times
in a row (equal records are still in order), so that the file holds at least
--records records.  A record's copies are cut into members of 65,280 bytes of
text at level 6; the records straddle those members, and a member never holds
two different records, so the blocks compress in parallel.  The index is
tests/bam_seek_fixture.write_bai's over one entry per record and its copies
(they share position, bin and chunk).  The panel is all 20,849 rows.

Legs: parent (--parent, the parent commit's bam-vaf-counter built into a
directory of its own), branch (this tree's, no variable), seek (this tree's,
VAFC_BAM_INDEX=seek); one untimed run of each, then --runs timed, alternating,
all at -t --threads, a host clock around each process; every .vaf must be the
same.  One more run with VAFC_PHASES=1 reports the members the seek pass read,
against the members in the file.  One JSON object: the seconds of every run,
medians, spreads (max - min), members read and in the file.  No ratio is fixed
in advance: the expectation is the share of members read, above a floor of
about 0.3 s of process start.

    python tools/bam_seek_e2e.py --parent DIR/bam-vaf-counter [--records 24000000] [--out profiles/bam_seek_e2e.json]
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmer-cnt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PAYLOAD = 65280


def _block(arg):
    """The members of one record written `repeat` times: (bytes, [(size, isize)])."""
    import bam_text_bench as TB
    rec, repeat = arg
    text = rec * repeat
    parts, sizes = [], []
    for i in range(0, len(text), PAYLOAD):
        m, _n = TB.bgzf_member(text[i:i + PAYLOAD])
        parts.append(m)
        sizes.append((len(m), min(PAYLOAD, len(text) - i)))
    return b"".join(parts), sizes


def make_file(path, n_records, rows, names, chunk_records, procs):
    """The BAM and its .bai; (records, text bytes, file bytes, members)."""
    import struct
    import bam_fixture as F
    import bam_seek_fixture as S
    import bam_text_bench as TB
    records = TB.chunk_records(rows, names, chunk_records)
    repeat = max(1, -(-n_records // len(records)))
    refs = [(c, 250_000_000) for c in names]
    head = F.bgzf(F.header(refs), eof=False)
    members, recs, coff, n_members, text_bytes = [], [], len(head), 0, 0
    with open(path, "wb") as f, Pool(procs) as pool:
        f.write(head)
        for rec, (raw, sizes) in zip(records, pool.imap(_block, ((r, repeat) for r in records), chunksize=64)):
            _bl, tid, pos, l_qname, _mapq, _bin, n_cigar = struct.unpack_from("<iiiBBHH", rec, 0)
            words = struct.unpack_from("<%dI" % n_cigar, rec, 36 + l_qname)
            rlen = sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8))
            f.write(raw)
            end = coff + len(raw)
            # the copies begin at their first member's byte 0 and end where the next block begins
            recs.append(S.Rec(coff << 16, end << 16, 0, tid, pos, pos + (rlen or 1)))
            coff = end
            n_members += len(sizes)
            text_bytes += len(rec) * repeat
        f.write(F.EOF_BLOCK)
    d = S.Decoded(members, b"", 0, [c for c, _n in refs], recs, coff)
    with open(path + ".bai", "wb") as f:
        f.write(S.write_bai(d))
    return repeat * len(records), text_bytes, os.path.getsize(path), n_members + 1


def run(binary, seek, threads, patterns, bam, out, phases=False):
    env = dict(os.environ)
    for k in ("VAFC_BGZF", "VAFC_BAM_INDEX", "VAFC_PHASES", "VAFC_BATCH_BYTES"):
        env.pop(k, None)
    if seek:
        env["VAFC_BAM_INDEX"] = "seek"
    if phases:
        env["VAFC_PHASES"] = "1"
    t0 = time.perf_counter()
    p = subprocess.run([binary, "-p", patterns, "-o", out, "-t", str(threads), bam], capture_output=True, text=True, env=env,
                       timeout=900)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        sys.exit("bam_seek_e2e: %s failed: %s" % (binary, p.stderr[-1000:]))
    with open(out, "rb") as f:
        return dt, hashlib.sha256(f.read()).hexdigest(), p.stderr


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--branch", default=os.path.join(ROOT, "kmer-cnt_amd", "lib", "bam-vaf-counter"))
    ap.add_argument("--records", type=int, default=24_000_000)
    ap.add_argument("--chunk-records", type=int, default=40000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--procs", type=int, default=16, help="processes that compress the file")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import bam_bench as BB
    rows = BB.panel_rows(0)
    names = list(dict.fromkeys(r[0] for r in rows))
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as tmp:
        pat, bam = os.path.join(tmp, "p.txt"), os.path.join(tmp, "s.bam")
        BB.write_patterns(rows, pat)
        t0 = time.perf_counter()
        n_records, text_bytes, file_bytes, n_members = make_file(bam, a.records, rows, names, a.chunk_records, a.procs)
        print("bam_seek_e2e: %d records, %.2f GB of text, %.2f GB file, %d members, written in %.1f s" % (
            n_records, text_bytes / 1e9, file_bytes / 1e9, n_members, time.perf_counter() - t0), file=sys.stderr, flush=True)
        legs = [("parent", a.parent, False), ("branch", a.branch, False), ("seek", a.branch, True)]
        secs = {name: [] for name, _b, _s in legs}
        shas = set()
        for i in range(a.runs + 1):
            for name, binary, seek in legs:
                dt, sha, _err = run(binary, seek, a.threads, pat, bam, os.path.join(tmp, name + ".vaf"))
                shas.add(sha)
                if i:
                    secs[name].append(round(dt, 4))
        _dt, sha, err = run(a.branch, True, a.threads, pat, bam, os.path.join(tmp, "phases.vaf"), phases=True)
        shas.add(sha)
        if len(shas) != 1:
            sys.exit("bam_seek_e2e: the .vaf files differ")
    m = re.search(r"inflate host (\d+) device (\d+) members, (\d+) records, (\d+) bases, \S+ s, seek state (\d+) spans (\d+) "
                  r"members (\d+) rereads (\d+)", err)
    if not m:
        sys.exit("bam_seek_e2e: no seek figures in: " + err[-500:])
    host, device, recs_read, _bases, state, spans, members_read, rereads = (int(x) for x in m.groups())
    res = dict(tool="bam_seek_e2e", records=n_records, text_bytes=text_bytes, file_bytes=file_bytes, members_in_file=n_members,
               rows=len(rows), threads=a.threads, runs=a.runs, seconds=secs, median={k: median(v) for k, v in secs.items()},
               spread={k: round(max(v) - min(v), 4) for k, v in secs.items()}, vaf_sha256=shas.pop(), vaf_identical=True,
               seek=dict(state=state, spans=spans, members_read=members_read, rereads=rereads, records_read=recs_read,
                         members_share=round(members_read / n_members, 4), records_share=round(recs_read / n_records, 4)))
    res["seek_vs_branch"] = round(res["median"]["seek"] / res["median"]["branch"], 3)
    res["seek_faster_than_branch_beyond_spread"] = res["median"]["seek"] + res["spread"]["branch"] < res["median"]["branch"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

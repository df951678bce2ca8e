#!/usr/bin/env python3
"""End to end: bam-vaf-counter on one BGZF BAM of several million records, the
parent commit's binary against this tree's, alternating in one call.

The file: a BAM header, then a seeded chunk of whole 150-bp records
(tools/bam_text_bench.chunk_records, over the GRCh38 panel) as BGZF members of
65,280 bytes of text at level 6 (the records straddle the members), the
chunk's members repeated until the file holds at least --records records, then
the EOF member.  --parent is the parent commit's bam-vaf-counter (built from a
checkout of it into a directory of its own), --branch this tree's (default
lib/bam-vaf-counter, run with VAFC_BGZF=device; a second leg runs it with
VAFC_BGZF=host).  The runs alternate parent, branch, ... --runs times each
after one untimed run of each, all with -t --threads; the wall clock of each
process is taken with a host clock, and the .vaf files must be identical.  One
JSON object: the seconds of every run, the medians, the parent's own spread
(max - min) and the verdict of the rule that chooses the default: the device
path is the default for BGZF BAM only if the branch's median is not above the
parent's by more than that spread.

    python tools/bam_bgzf_e2e.py --parent DIR/bam-vaf-counter [--records 4000000] [--out profiles/bam_bgzf_e2e.json]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmer-cnt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PAYLOAD = 65280


def make_file(path, n_records, rows, names, chunk_records=40000):
    import bam_fixture as F
    import bam_text_bench as TB
    records = TB.chunk_records(rows, names, chunk_records)
    chunk = b"".join(records)
    # the chunk begins at a member border, so that its members can be repeated as they are
    body = b"".join(TB.bgzf_member(chunk[i:i + PAYLOAD])[0] for i in range(0, len(chunk), PAYLOAD))
    reps = max(1, -(-n_records // len(records)))
    with open(path, "wb") as f:
        f.write(F.bgzf(F.header([(c, 250_000_000) for c in names]), eof=False))
        for _ in range(reps):
            f.write(body)
        f.write(F.EOF_BLOCK)
    return reps * len(records), reps * len(chunk), os.path.getsize(path)


def run(binary, env_bgzf, threads, patterns, bam, out):
    env = dict(os.environ)
    env.pop("VAFC_BGZF", None)
    if env_bgzf:
        env["VAFC_BGZF"] = env_bgzf
    t0 = time.perf_counter()
    p = subprocess.run([binary, "-p", patterns, "-o", out, "-t", str(threads), bam], capture_output=True, text=True, env=env,
                       timeout=600)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        sys.exit("bam_bgzf_e2e: %s failed: %s" % (binary, p.stderr[-1000:]))
    with open(out, "rb") as f:
        return dt, hashlib.sha256(f.read()).hexdigest()


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--branch", default=os.path.join(ROOT, "kmer-cnt_amd", "lib", "bam-vaf-counter"))
    ap.add_argument("--records", type=int, default=4_000_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import bam_bench as BB
    rows = BB.panel_rows(0)
    names = list(dict.fromkeys(r[0] for r in rows))
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as tmp:
        pat, bam = os.path.join(tmp, "p.txt"), os.path.join(tmp, "s.bam")
        BB.write_patterns(rows, pat)
        n_records, text_bytes, file_bytes = make_file(bam, a.records, rows, names)
        legs = [("parent", a.parent, None), ("branch", a.branch, "device"), ("branch_host", a.branch, "host")]
        secs = {name: [] for name, _b, _e in legs}
        shas = set()
        for i in range(a.runs + 1):
            for name, binary, env in legs:
                dt, sha = run(binary, env, a.threads, pat, bam, os.path.join(tmp, name + ".vaf"))
                shas.add(sha)
                if i:
                    secs[name].append(round(dt, 4))
        if len(shas) != 1:
            sys.exit("bam_bgzf_e2e: the .vaf files differ")
    spread = max(secs["parent"]) - min(secs["parent"])
    res = dict(tool="bam_bgzf_e2e", records=n_records, text_bytes=text_bytes, file_bytes=file_bytes, threads=a.threads,
               runs=a.runs, seconds=secs, median={k: median(v) for k, v in secs.items()}, parent_spread=round(spread, 4),
               vaf_sha256=shas.pop(), vaf_identical=True)
    res["device_default"] = res["median"]["branch"] <= res["median"]["parent"] + spread
    res["host_within"] = res["median"]["branch_host"] <= res["median"]["parent"] + spread
    res["records_per_s"] = {k: round(n_records / v, 1) for k, v in res["median"].items()}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

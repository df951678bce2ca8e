#!/usr/bin/env python3
"""Golden fixtures for vcf-vaf-counter from the REAL reference binary.

Build the program by hand into a scratch directory.  The reference's own rule
links -lcurl -lcrypto -ldeflate; zlib alone is enough:

    cp -r <reference>/htslib <scratch>/htslib && cd <scratch>/htslib
    ./configure --disable-bz2 --disable-lzma --disable-libcurl --disable-gcs --disable-s3 --without-libdeflate
    make lib-static
    gcc -g -Wall -O2 -I<reference> -I<scratch>/htslib <reference>/vcf-vaf-counter.c \\
        <scratch>/htslib/libhts.a -lz -lm -lpthread -o <scratch>/vcf-vaf-counter

    python tests/golden/make_golden_vcf.py --ref-bin <scratch>/vcf-vaf-counter

Writes tests/golden/vcf/: the small inputs that tests/vcf_fixture.py builds
(inputs(): plain, gzip, BGZF and CRLF files, the panel p.txt with duplicate
rows, chr1 / chr10 / chr1_x, a row at start -1 and a chromosome no header
declares, and p_empty.txt) and manifest.json with, per case of
vcf_fixture.cases(), the argv, the exit code, the reference program's own
stderr lines (htslib's [E::..] / [W::..] lines are left out) and the .vaf it
wrote, kept as the md5 of its bytes, its first line and the "REF_COUNT
ALT_COUNT" pairs of its rows.  A .vaf that an earlier case (in name order)
already holds is stored as "=<that case>".  The cases run in a directory that
holds the inputs and an empty directory o/.

Every case that ends a file early (end_*, gt_int) has a row hit behind the
line that stops it: its counts stay 0 0 in the golden.
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vcf_fixture as F  # noqa: E402

OUT = os.path.join(HERE, "vcf")


def own_lines(stderr: str) -> str:
    """The reference program's own lines: htslib's start with [E:: or [W::."""
    return "".join(ln + "\n" for ln in stderr.splitlines() if not re.match(r"\[[EWIDT]::", ln))


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
    ap.add_argument("--ref-bin", required=True, help="the reference's vcf-vaf-counter, built as the docstring says")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref_bin)
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    for name, data in F.inputs().items():
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
    manifest, first = {}, {}
    with tempfile.TemporaryDirectory() as work:
        for name in os.listdir(OUT):
            shutil.copy(os.path.join(OUT, name), work)
        for name, argv in sorted(F.cases().items()):
            rc, err, vaf = run_case(ref, argv, work)
            manifest[name] = {"argv": argv, "rc": rc, "stderr": own_lines(err)}
            if vaf is not None:
                manifest[name]["vaf"] = "=" + first[vaf] if vaf in first else F.vaf_entry(vaf)
                first.setdefault(vaf, name)
            print("%-18s rc=%d %s" % (name, rc, str(manifest[name].get("vaf"))[:100]))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    sizes = {fn: os.path.getsize(os.path.join(OUT, fn)) for fn in sorted(os.listdir(OUT))}
    print("fixture bytes: %d (largest %s); manifest md5 %s" % (
        sum(sizes.values()), max(sizes.items(), key=lambda kv: kv[1]),
        hashlib.md5(open(os.path.join(OUT, "manifest.json"), "rb").read()).hexdigest()))


if __name__ == "__main__":
    main()

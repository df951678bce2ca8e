#!/bin/bash
# AddressSanitizer + UBSan run of the device's BAM text scan (host code only,
# no GPU, nothing loaded into Python): kmer-cnt_amd/csrc/vafc_bam_text.h
# compiled with a one-lane wave into the stand-alone tools/bam_text_check.cpp
# and run over every case file of a directory (default: every scan of every
# class of tests/bam_text_fixture.py).  Each scan is compared with what its
# file states; any difference and any sanitizer report fails the run.
#   tools/bam_text_asan.sh [casedir]
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/tools/bin"
CS=$ROOT/kmer-cnt_amd/csrc
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -I"$ROOT/include" -I"$CS" \
    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    "$ROOT/tools/bam_text_check.cpp" -o "$ROOT/tools/bin/bam_text_asan"
export ASAN_OPTIONS="detect_leaks=1" UBSAN_OPTIONS="print_stacktrace=1"
D=${1:-}
if [ -z "$D" ]; then
    D=$(mktemp -d)
    trap 'rm -rf "$D"' EXIT
    python3 "$ROOT/tests/bam_text_fixture.py" "$D"
fi
find "$D" -name '*.vbt' -print0 | sort -z | xargs -0 "$ROOT/tools/bin/bam_text_asan"
echo "bam_text_asan: all clean"

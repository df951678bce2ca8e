#!/bin/bash
# AddressSanitizer + UBSan run of the BAI reader, the seek planner and the
# device's piece walk (host code only, no GPU, nothing loaded into Python):
# kmer-cnt_amd/csrc/vafc_bam_index.cpp and vbt_piece_walk of vafc_bam_text.h
# compiled with a one-lane wave into the stand-alone tools/bam_index_check.cpp.
# The planner runs over every golden index, every prefix of each and seeded
# byte flips; the piece walk over every case file of a directory (default:
# every class of tests/bam_seek_fixture.py).  Any difference from a statement
# and any sanitizer report fails the run.
#   tools/bam_index_asan.sh [casedir]
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/tools/bin"
CS=$ROOT/kmer-cnt_amd/csrc
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -I"$ROOT/include" -I"$CS" \
    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    "$ROOT/tools/bam_index_check.cpp" -o "$ROOT/tools/bin/bam_index_asan"
export ASAN_OPTIONS="detect_leaks=1" UBSAN_OPTIONS="print_stacktrace=1"
D=${1:-}
if [ -z "$D" ]; then
    D=$(mktemp -d)
    trap 'rm -rf "$D"' EXIT
    python3 "$ROOT/tests/bam_seek_fixture.py" "$D"
fi
G=$ROOT/tests/golden/bam
"$ROOT/tools/bin/bam_index_asan" "$G/a.index" "$G/b.bam.bai" "$G/long.index"
find "$D" -name '*.vbp' -print0 | sort -z | xargs -0 "$ROOT/tools/bin/bam_index_asan"
echo "bam_index_asan: all clean"

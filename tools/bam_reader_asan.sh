#!/bin/bash
# AddressSanitizer + UBSan run of the BAM host reader (host code only, no GPU,
# nothing loaded into Python): kmer-cnt_amd/csrc/vafc_bam.cpp linked into the
# stand-alone tools/bam_reader_check.cpp and run over every golden BAM, the
# damaged ones included, with 1, 3 and 16 inflate threads; then the same
# program under ThreadSanitizer.  Any report fails the run.
#   tools/bam_reader_asan.sh [more.bam ...]
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/tools/bin"
CS=$ROOT/kmer-cnt_amd/csrc
COMMON="-std=c++17 -O1 -g -fno-omit-frame-pointer -pthread -I$ROOT/include -I$CS"
g++ $COMMON -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    "$ROOT/tools/bam_reader_check.cpp" "$CS/vafc_bam.cpp" -lz -o "$ROOT/tools/bin/bam_reader_asan"
g++ $COMMON -fsanitize=thread "$ROOT/tools/bam_reader_check.cpp" "$CS/vafc_bam.cpp" -lz -o "$ROOT/tools/bin/bam_reader_tsan"
export ASAN_OPTIONS="detect_leaks=1" UBSAN_OPTIONS="print_stacktrace=1" TSAN_OPTIONS="halt_on_error=1"
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
# the golden BAMs and the damaged files cut from them (tests/bam_fixture.py)
PYTHONPATH="$ROOT/tests" python3 -c 'import sys, bam_fixture; bam_fixture.derive(sys.argv[1], sys.argv[2])' \
    "$ROOT/tests/golden/bam" "$D"
"$ROOT/tools/bin/bam_reader_asan" -t 1,3,16 "$D"/*.bam "$@"
"$ROOT/tools/bin/bam_reader_tsan" -t 3,16 "$D"/*.bam "$@" > /dev/null
echo "bam_reader_asan: all clean"

#!/bin/bash
# AddressSanitizer + UBSan run of the device inflater's decode text (host code
# only, no GPU, nothing loaded into Python): kmer-cnt_amd/csrc/vafc_inflate.h
# compiled with a one-lane wave into the stand-alone
# tools/bgzf_inflate_check.cpp and run over every case file of a directory
# (default: the cases tests/bgzf_fixture.py writes, the malformed streams
# included).  Its lines go to stdout; any sanitizer report fails the run.
#   tools/bgzf_inflate_asan.sh [casedir]
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/tools/bin"
CS=$ROOT/kmer-cnt_amd/csrc
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -I"$ROOT/include" -I"$CS" \
    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    "$ROOT/tools/bgzf_inflate_check.cpp" -o "$ROOT/tools/bin/bgzf_inflate_asan"
export ASAN_OPTIONS="detect_leaks=1" UBSAN_OPTIONS="print_stacktrace=1"
D=${1:-}
if [ -z "$D" ]; then
    D=$(mktemp -d)
    trap 'rm -rf "$D"' EXIT
    python3 "$ROOT/tests/bgzf_fixture.py" "$D"
fi
"$ROOT/tools/bin/bgzf_inflate_asan" "$D"/*.bgzf
echo "bgzf_inflate_asan: all clean"

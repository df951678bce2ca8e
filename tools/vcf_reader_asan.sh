#!/bin/bash
# AddressSanitizer + UBSan run of the VCF host parser (host code only, no GPU,
# nothing loaded into Python): kmer-cnt_amd/csrc/vafc_vcf.cpp and the gzip
# inflater it reads through, linked into the stand-alone
# tools/vcf_reader_check.cpp and run over every golden input and over the
# truncations of each at every byte of its first 4 KB.  Any report fails the run.
#   tools/vcf_reader_asan.sh [more.vcf ...]
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/tools/bin"
CS=$ROOT/kmer-cnt_amd/csrc
COMMON="-std=c++17 -O1 -g -fno-omit-frame-pointer -pthread -I$ROOT/include -I$CS"
g++ $COMMON -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    "$ROOT/tools/vcf_reader_check.cpp" "$CS/vafc_vcf.cpp" "$CS/vafc_gzip.cpp" -lz -o "$ROOT/tools/bin/vcf_reader_asan"
export ASAN_OPTIONS="detect_leaks=1" UBSAN_OPTIONS="print_stacktrace=1"
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
"$ROOT/tools/bin/vcf_reader_asan" "$D" "$ROOT"/tests/golden/vcf/*.vcf "$ROOT"/tests/golden/vcf/*.vcf.gz "$@"
echo "vcf_reader_asan: all clean"

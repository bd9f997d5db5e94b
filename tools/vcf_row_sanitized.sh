#!/bin/bash
# usage: tools/vcf_row_sanitized.sh [cases] [seed]   (CPU only) the VCF reader's decision function under AddressSanitizer +
# UndefinedBehaviorSanitizer.  tools/vcf_row_fuzz.cpp (its own main) includes csrc/sg_vcf.h -- the code the device kernel
# runs, compiled for the host -- and is compiled with the sanitizers into one program; nothing else is linked, no GPU is
# touched.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/vcf_row_san; mkdir -p "$OUT"
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    "$ROOT/tools/vcf_row_fuzz.cpp" -o "$OUT/vcf_row_fuzz"
"$OUT/vcf_row_fuzz" "${1:-20000}" "${2:-12345}"

#!/bin/bash
# usage: tools/hap_check_sanitized.sh [lists] [seed]   (CPU only) the argument checks in front of the reference ingest and
# haplotype assembly kernels (simuscop_amd/csrc/sg_hap_check.h) under AddressSanitizer + UndefinedBehaviorSanitizer.
# tools/hap_check_fuzz.cpp (its own main) includes the header; nothing else is compiled or linked, no HIP header is
# reached (plain g++ would stop at one) and no GPU is touched.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/hap_check_san; mkdir -p "$OUT"
g++ -O1 -g -std=c++17 -Wall -Werror -I "$ROOT/include" -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    "$ROOT/tools/hap_check_fuzz.cpp" -o "$OUT/hap_check_fuzz"
"$OUT/hap_check_fuzz" "${1:-4000}" "${2:-12345}"

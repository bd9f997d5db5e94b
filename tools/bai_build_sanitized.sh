#!/bin/bash
# usage: tools/bai_build_sanitized.sh [cases] [seed]   (CPU only) the serialiser of --truth-index under AddressSanitizer +
# UndefinedBehaviorSanitizer.  tools/bai_build_fuzz.cpp (its own main) and host/truth_index.cpp are compiled with the
# sanitizers into one program; nothing else is linked, no GPU is touched.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/bai_build_san; mkdir -p "$OUT"
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    "$ROOT/tools/bai_build_fuzz.cpp" "$ROOT/simuscop_amd/csrc/host/truth_index.cpp" -o "$OUT/bai_build_fuzz"
"$OUT/bai_build_fuzz" "${1:-2000}" "${2:-12345}"

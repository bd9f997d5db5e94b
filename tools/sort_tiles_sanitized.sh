#!/bin/bash
# usage: tools/sort_tiles_sanitized.sh [run sets] [seed]   (CPU only) the tile cutter of --truth-sort under AddressSanitizer +
# UndefinedBehaviorSanitizer.  tools/sort_tiles_fuzz.cpp (its own main) and host/truth_sort_tiles.cpp are compiled with the
# sanitizers into one program; nothing else is linked, no GPU is touched.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/sort_tiles_san; mkdir -p "$OUT"
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    "$ROOT/tools/sort_tiles_fuzz.cpp" "$ROOT/simuscop_amd/csrc/host/truth_sort_tiles.cpp" -o "$OUT/sort_tiles_fuzz"
"$OUT/sort_tiles_fuzz" "${1:-3000}" "${2:-12345}"

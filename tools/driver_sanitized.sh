#!/bin/bash
# usage: tools/driver_sanitized.sh   (CPU only) the chunk pump of the FASTQ sink (host/fastq_sink.h) and the two cuts of a
# batch (host/batch_cut.h) under AddressSanitizer + UndefinedBehaviorSanitizer, then under ThreadSanitizer.
# tools/driver_check.cpp (its own main) includes the two headers; nothing else is linked, no GPU is touched.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/driver_san; mkdir -p "$OUT"
for san in address,undefined thread; do
  g++ -O1 -g -std=c++17 -Wall -pthread -fsanitize=$san -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
      "$ROOT/tools/driver_check.cpp" -o "$OUT/driver_check_${san%%,*}"
  "$OUT/driver_check_${san%%,*}" "$OUT"
done

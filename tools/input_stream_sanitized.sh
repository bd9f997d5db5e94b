#!/bin/bash
# usage: tools/input_stream_sanitized.sh   (CPU only) the batch reader and the read-ahead loop of seqToProfile and truthEval
# (host/input_stream.h) under AddressSanitizer + UndefinedBehaviorSanitizer, then under ThreadSanitizer.
# tools/input_stream_check.cpp (its own main) includes the header and the engine's member walk (sg_bgzf.h) and defines the
# engine calls the reader links against; nothing else is linked, no GPU is touched.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/input_stream_san; mkdir -p "$OUT"
for san in address,undefined thread; do
  g++ -O1 -g -std=c++17 -Wall -pthread -fsanitize=$san -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
      "$ROOT/tools/input_stream_check.cpp" -o "$OUT/input_stream_check_${san%%,*}"
  "$OUT/input_stream_check_${san%%,*}" "$OUT"
done

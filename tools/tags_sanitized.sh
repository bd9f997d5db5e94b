#!/bin/bash
# usage: tools/tags_sanitized.sh [records] [seed]   (CPU only) the host statement of the truth tags' rule under
# AddressSanitizer + UndefinedBehaviorSanitizer.  tools/tags_fuzz.cpp (its own main) and sg_api_truth_tags.cpp are compiled
# with the sanitizers on the host side into one program; nothing else is needed and no GPU is touched: sg_truth_tags
# needs no context.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/tags_san; mkdir -p "$OUT"
HIPCC=$(command -v hipcc || echo /opt/rocm/bin/hipcc)
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I "$ROOT/include" \
    -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -fno-sanitize-recover=undefined \
    -x hip "$ROOT/tools/tags_fuzz.cpp" "$ROOT/simuscop_amd/csrc/sg_api_truth_tags.cpp" \
    -fsanitize=address,undefined -o "$OUT/tags_fuzz"
"$OUT/tags_fuzz" "${1:-20000}" "${2:-12345}"

#!/bin/bash
# usage: tools/errtab_sanitized.sh [reads] [seed]   (CPU only) the host statement of the true error counts' rule under
# AddressSanitizer + UndefinedBehaviorSanitizer.  tools/errtab_fuzz.cpp (its own main) and sg_api_errors.cpp are compiled
# with the sanitizers on the host side into one program; everything else comes from the built libsimuscop_amd.so.  No GPU
# is touched: sg_errtab_observe needs no context.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/errtab_san; mkdir -p "$OUT"
HIPCC=$(command -v hipcc || echo /opt/rocm/bin/hipcc)
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I "$ROOT/include" \
    -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -fno-sanitize-recover=undefined \
    -x hip "$ROOT/tools/errtab_fuzz.cpp" "$ROOT/simuscop_amd/csrc/sg_api_errors.cpp" \
    -fsanitize=address,undefined -L "$ROOT/simuscop_amd/lib" -lsimuscop_amd -Wl,-rpath,"$ROOT/simuscop_amd/lib" -o "$OUT/errtab_fuzz"
"$OUT/errtab_fuzz" "${1:-20000}" "${2:-12345}"

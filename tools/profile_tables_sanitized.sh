#!/bin/bash
# usage: tools/profile_tables_sanitized.sh   (CPU only) the profile-table builder under AddressSanitizer +
# UndefinedBehaviorSanitizer.  tools/profile_tables_check.cpp (its own main), sg_profile_tables.cpp, sg_tables.cpp and
# host/profile.cpp are compiled with the sanitizers into one program; nothing else is linked, no GPU is touched.  Its
# lines must be those of tests/profile_tables_expected.txt.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/profile_tables_san; mkdir -p "$OUT"
C="$ROOT/simuscop_amd/csrc"
g++ -O1 -g -std=c++17 -ffp-contract=off -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    "$ROOT/tools/profile_tables_check.cpp" "$C/sg_profile_tables.cpp" "$C/sg_tables.cpp" "$C/host/profile.cpp" -o "$OUT/profile_tables_check"
"$OUT/profile_tables_check" "$ROOT/tests/golden/testData" > "$OUT/lines.txt"
diff "$OUT/lines.txt" "$ROOT/tests/profile_tables_expected.txt"
echo "$(wc -l < "$OUT/lines.txt") cases under the sanitizers, all as tests/profile_tables_expected.txt has them"

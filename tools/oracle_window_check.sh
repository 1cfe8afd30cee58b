#!/bin/bash
# Builds tools/oracle_window_check.c with oracle/relate_oracle.c under AddressSanitizer and UBSan and runs it on the
# CPU (test infrastructure only; no GPU, nothing loaded into Python).
#   tools/oracle_window_check.sh [work directory, default: a temporary one]
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
WORK="${1:-$(mktemp -d)}"
mkdir -p "$WORK"
${CC:-gcc} -O1 -g -std=gnu99 -ffp-contract=off -fno-omit-frame-pointer -fsanitize=address,undefined -Wall \
  -I"$ROOT/oracle" "$ROOT/tools/oracle_window_check.c" "$ROOT/oracle/relate_oracle.c" -lm -lpthread \
  -o "$WORK/oracle_window_check"
ASAN_OPTIONS=detect_leaks=1 "$WORK/oracle_window_check" "$WORK"

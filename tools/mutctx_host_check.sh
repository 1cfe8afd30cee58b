#!/bin/sh
# Builds tools/mutctx_host_check.cpp with mutctx.cpp, mutrate.cpp and tree_host.cpp, host code only, under
# AddressSanitizer and UBSan, writes the fixture cases' input files and runs the program on them -- on the CPU, as a
# program of its own (see the head of the .cpp).  Needs hipcc for the headers only; no GPU.
#   tools/mutctx_host_check.sh [work directory, default: a temporary one]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
WORK=${1:-$(mktemp -d)}
mkdir -p "$WORK"
CSRC="$ROOT/relate_amd/csrc"
FLAGS="-O1 -g -std=c++17 -ffp-contract=off -x hip --cuda-host-only -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$ROOT/include -I$CSRC"
for f in "$CSRC/mutctx.cpp" "$CSRC/mutrate.cpp" "$CSRC/tree_host.cpp" "$ROOT/tools/mutctx_host_check.cpp"; do
  $HIPCC $FLAGS -c "$f" -o "$WORK/$(basename "$f" .cpp).o" &
done
wait
$HIPCC -fsanitize=address,undefined "$WORK"/mutctx.o "$WORK"/mutrate.o "$WORK"/tree_host.o "$WORK"/mutctx_host_check.o -o "$WORK/mutctx_host_check"
python3 - "$ROOT" "$WORK" <<'EOF'
import sys
sys.path.insert(0, sys.argv[1] + "/tests")
import mutctx_cases as xc
for key in xc.CASES:
    xc.write_inputs(sys.argv[2], xc.CASES[key][0], xc.case_inputs(key)[0])
EOF
ASAN_OPTIONS=detect_leaks=1 "$WORK/mutctx_host_check" "$WORK" a a2 s::8 s::8:dist s:2,6.5,0.5:12.5

#!/bin/bash
# tools/build_variant.sh NAME "EXTRA FLAGS": relate_amd/variants/librelate_amd_NAME.so = the library with
# minmatch_worker.hip -- the unit that holds the tree-build kernel -- recompiled under EXTRA (experiments on that kernel,
# tools/bench_builder_variants.py)
set -e
cd "$(dirname "$0")/../relate_amd/csrc"
NAME=$1; EXTRA=$2
mkdir -p ../variants ../../build/variants
FLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -I../../include -I. -Wno-unused-result"
/opt/rocm/bin/hipcc $FLAGS $EXTRA -c minmatch_worker.hip -o ../../build/variants/minmatch_worker_$NAME.o
OBJS=$(ls ../../build/obj/*.o | grep -v minmatch_worker.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../variants/librelate_amd_$NAME.so $OBJS ../../build/variants/minmatch_worker_$NAME.o -lpthread -lz
echo built ../variants/librelate_amd_$NAME.so

#!/bin/bash
# Diagnostic build of libawsm_hip.so with in-kernel s_memrealtime stamps in the geometry kernels (-DAWSM_STAMP) -> build/variants/lib_STAMP.so
set -e
cd "$(dirname "$0")/../awsm-renderer_amd/csrc"
OUT=../../build/variants; mkdir -p $OUT
FLAGS="$(make -s print-CXXFLAGS) -DAWSM_STAMP"
OBJS=""
for f in $(make -s print-SRC); do
  /opt/rocm/bin/hipcc $FLAGS -c -o $OUT/stamp_${f%.*}.o $f 2>&1 | grep -v hip-link || true; OBJS="$OBJS $OUT/stamp_${f%.*}.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/lib_STAMP.so $OBJS && rm -f $OBJS && echo built $OUT/lib_STAMP.so

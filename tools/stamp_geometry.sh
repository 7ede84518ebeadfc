#!/bin/bash
# Diagnostic build of libawsm_hip.so with in-kernel s_memrealtime stamps in the geometry kernels (-DAWSM_STAMP) -> build/variants/lib_STAMP.so
set -e
cd "$(dirname "$0")/../awsm-renderer_amd/csrc"
OUT=../../build/variants; mkdir -p $OUT
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wno-unused-function -DAWSM_STAMP"
OBJS=""
for f in awsm_hip.cpp awsm_resources.cpp kernels_geometry.hip kernels_shade.hip kernels_post.hip kernels_env.hip kernels_texture.hip; do      # csrc/Makefile: SRC
  /opt/rocm/bin/hipcc $FLAGS -c -o $OUT/stamp_${f%.*}.o $f 2>&1 | grep -v hip-link || true; OBJS="$OBJS $OUT/stamp_${f%.*}.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/lib_STAMP.so $OBJS && rm -f $OBJS && echo built $OUT/lib_STAMP.so

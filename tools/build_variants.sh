#!/bin/bash
# A/B builds of libawsm_hip.so with extra -D flags for kernels_shade.hip, into build/variants/ (git-ignored; travels with gpurun).
# usage: tools/build_variants.sh NAME "-DFLAG=1 ..." [NAME2 "..."] ...   then on the GPU box: tools/ab_bench.sh build/variants/lib_NAME.so ...
# (a NAME that starts with g_ applies its flags to kernels_geometry.hip instead, one that starts with h_ to the two host files, awsm_hip.cpp and
#  awsm_resources.cpp, which see one AwsmHipCtx — e.g.
#  h_debug "-DAWSM_DEBUG_SWITCHES": the AWSM_DEBUG_KNOCKOUT / AWSM_SHADE_CU_MASK experiments, which the product library does not carry)
set -e
cd "$(dirname "$0")/../awsm-renderer_amd/csrc"
OUT=../../build/variants
mkdir -p $OUT
FLAGS="$(make -s print-CXXFLAGS)"; OBJ="$(make -s print-OBJ)"      # the Makefile's own flags and object list
make -s ../libawsm_hip.so >/dev/null
while [ $# -ge 2 ]; do
  NAME=$1; DEFS=$2; shift 2
  if [[ $NAME == g_* ]]; then SRC="kernels_geometry.hip"; elif [[ $NAME == h_* ]]; then SRC="awsm_hip.cpp awsm_resources.cpp"; else SRC="kernels_shade.hip"; fi
  ( VAR=""; OTHER=""
    for o in $OBJ; do case " $SRC " in *" ${o%.o}.cpp "*|*" ${o%.o}.hip "*) ;; *) OTHER="$OTHER $o";; esac; done
    for f in $SRC; do /opt/rocm/bin/hipcc $FLAGS $DEFS -c -o $OUT/var_${NAME}_${f%.*}.o $f 2>&1 | grep -v hip-link || true; VAR="$VAR $OUT/var_${NAME}_${f%.*}.o"; done
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/lib_$NAME.so $OTHER $VAR && rm -f $VAR && echo built $OUT/lib_$NAME.so ) &
  while [ $(jobs -r | wc -l) -ge 3 ]; do sleep 1; done
done
wait

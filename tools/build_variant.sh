#!/bin/bash
# build an A/B variant of the library: tools/build_variant.sh <name> <extra hipcc -D flags...>  ->  tools/_bin/libnereus_hip_<name>.so
# (only one unit is recompiled with the flags: the fp32 Muller context, or the one named by UNIT=<file without .hip>, e.g. UNIT=nrs_mesh;
# select the library with NEREUS_HIP_LIB=<path>)
set -e
cd "$(dirname "$0")/../nereus_amd/csrc"
NAME=$1; shift
UNIT=${UNIT:-nrs_inst_f32_muller}
mkdir -p build ../../tools/_bin
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -w "$@" -c -o build/var_$NAME.o $UNIT.hip
# the Makefile's object list with the variant in place of that unit; -z defs: an object missing from it fails the link
OBJS=$(make -s print-objs | sed "s#build/$UNIT.o#build/var_$NAME.o#")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -Wl,-z,defs -o ../../tools/_bin/libnereus_hip_$NAME.so $OBJS
echo built tools/_bin/libnereus_hip_$NAME.so

#!/bin/bash
# build an A/B variant of the library: tools/build_variant.sh <name> <extra hipcc -D flags...>  ->  tools/_bin/libnereus_hip_<name>.so
# (only the fp32 Muller unit is recompiled with the flags; select it with NEREUS_HIP_LIB=<path>)
set -e
cd "$(dirname "$0")/../nereus_amd/csrc"
NAME=$1; shift
mkdir -p build ../../tools/_bin
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -w "$@" -c -o build/var_$NAME.o nrs_inst_f32_muller.hip
# the Makefile's object list with the variant in place of the fp32 Muller unit; -z defs: an object missing from it fails the link
OBJS=$(make -s print-objs | sed "s#build/nrs_inst_f32_muller.o#build/var_$NAME.o#")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -Wl,-z,defs -o ../../tools/_bin/libnereus_hip_$NAME.so $OBJS
echo built tools/_bin/libnereus_hip_$NAME.so

#!/bin/bash
# Build an experimental variant of the convolution units into its own library:  tools/conv_variant.sh NAME "-DSOME_SWITCH=1 ..."
# (the experiment switches of rounds 1-5 -- stagger, set-priority, MFMAs in front of the hand-over, late issue, ablations -- are no
# longer in the shipped source: apply profiles/r06_experiments/conv_dead_switches.patch to get them back)
# -> swem_amd/libswem_hip_NAME.so (conv_presplit.hip compiled with -DSWEM_ISA_SUBSET: a fifth of the instantiations, about a
# minute; every other object as built).  Run with  SWEM_HIP_LIB=swem_amd/libswem_hip_NAME.so python tools/conv_bench.py --dominant
set -e
cd "$(dirname "$0")/.."
name=$1; shift
objs=""
for u in conv conv_f32 conv_presplit conv_t256; do
  subset=""; [ $u = conv_presplit ] && subset=-DSWEM_ISA_SUBSET
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $subset $@ \
    -c swem_amd/csrc/$u.hip -o /tmp/${u}_$name.o
  objs="$objs /tmp/${u}_$name.o"
done
for o in api bneck pointwise em match train train_conv; do objs="$objs swem_amd/csrc/$o.o"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o swem_amd/libswem_hip_$name.so $objs
echo swem_amd/libswem_hip_$name.so

#!/bin/bash
# Build a variant of librac_hip.so with extra compiler flags, for A/B runs on the GPU box:
#   bash tools/build_variant.sh <name> [extra hipcc flags ...]   ->  robot_aware_control_amd/variants/librac_<name>.so
#   RAC_HIP_LIB=robot_aware_control_amd/variants/librac_<name>.so python tools/bench_gemm.py ...
# Every csrc/*.hip is compiled with the Makefile's own compiler and flags plus the extra ones: the variant has every export.
set -eo pipefail
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
csrc=$root/robot_aware_control_amd/csrc
cc=$(make -s --no-print-directory -C "$csrc" --eval='print-cc: ; @echo $(HIPCC) $(CXXFLAGS)' print-cc)
obj=$(mktemp -d "/tmp/rac_variant_$name.XXXXXX"); mkdir -p "$root/robot_aware_control_amd/variants"
pids=()
for src in "$csrc"/*.hip; do
  $cc "$@" -c "$src" -o "$obj/$(basename "$src" .hip).o" &
  pids+=($!)
done
for pid in "${pids[@]}"; do wait "$pid"; done
${cc%% *} -shared -fPIC --offload-arch=gfx950 "$obj"/*.o -o "$root/robot_aware_control_amd/variants/librac_$name.so"
echo "built variants/librac_$name.so"

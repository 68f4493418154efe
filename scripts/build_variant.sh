#!/bin/bash
# diagnostic build of the library with extra hipcc flags into build/<name>/libldiff_hip.so (A/B runs on ONE box through LDIFF_LIB: boxes of the pool
# differ by more than most effects); never the product library.
#   scripts/build_variant.sh <name> <extra hipcc flags...>                     every file recompiled
#   scripts/build_variant.sh <name> --only <file.hip> <extra hipcc flags...>   that file of csrc/ recompiled, linked with the product objects (build/obj)
# e.g. the in-kernel stamps (csrc/stamps.h) of one kernel file: scripts/build_variant.sh stamps --only kernels_conv3x3p.hip -DLDIFF_STAMPS
set -e
cd "$(dirname "$0")/.."
name=$1; shift
only=; if [ "$1" = --only ]; then only=$(basename $2); shift 2; fi
mkdir -p build/$name
pids=()
for src in ldiffusion_amd/csrc/${only:-*.hip}; do
  obj=build/$name/$(basename ${src%.hip}).o
  hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -Wno-comment "$@" -c $src -o $obj &
  pids+=($!)
  if [ ${#pids[@]} -ge 4 ]; then wait ${pids[0]}; pids=("${pids[@]:1}"); fi
done
for p in "${pids[@]}"; do wait $p; done
objs=build/$name/*.o
if [ -n "$only" ]; then objs="build/$name/${only%.hip}.o $(ls build/obj/*.o | grep -v "/${only%.hip}.o")"; fi
hipcc --offload-arch=gfx950 -shared -fPIC -o build/$name/libldiff_hip.so $objs
echo built build/$name/libldiff_hip.so

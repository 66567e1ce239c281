#!/bin/bash
# Builds (if needed) and runs the broadcast micro-benchmark; its output is what profiles/bcast_factor_bench.txt holds.
#   tools/bcast/run.sh [build]        "build": compile only (cross-compiles without a GPU)
set -e
cd "$(dirname "$0")/../.."
B=tools/bcast/factor_bench
if [ ! -x $B ] || [ $B.hip -nt $B ] || [ tsid_control_amd/csrc/tsidb_tick.hpp -nt $B ] || [ tsid_control_amd/csrc/tsidb_common.hpp -nt $B ]; then
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -disable-machine-licm -ffp-contract=on -I tsid_control_amd/csrc -o $B $B.hip
fi
[ "$1" = build ] && exit 0
timeout -k 10 120 $B

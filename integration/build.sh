#!/usr/bin/env bash
# Builds the C++ multi-GPU batch driver into integration/_build/ (git-ignored).  The real-CompV plugin and its
# headless sample driver need the CompV sources: oracle/build_ref.sh builds them into oracle/_ref/.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(dirname "$HERE")"
OUT="$HERE/_build"
mkdir -p "$OUT"
# the C++ multi-GPU batch driver: C ABI + RCCL only, no CompV checkout needed
ROCM="${ROCM_PATH:-/opt/rocm}"
if [ -f "$ROCM/lib/librccl.so" ] && [ -f "$ROCM/lib/libamdhip64.so" ] && [ -f "$ROOT/compv_amd/lib/libcompv_hip.so" ]; then
  g++ -std=c++14 -O2 -w -D__HIP_PLATFORM_AMD__ -I"$ROCM/include" -o "$OUT/multi_gpu_batch" "$HERE/multi_gpu_batch.cxx" \
    -L"$ROOT/compv_amd/lib" -lcompv_hip -L"$ROCM/lib" -lamdhip64 -lrccl \
    -Wl,-rpath,'$ORIGIN/../../compv_amd/lib' -Wl,-rpath,"$ROCM/lib" -lpthread
  echo "integration/build.sh: OK -> $OUT/multi_gpu_batch"
else
  echo "integration/build.sh: no ROCm/RCCL or libcompv_hip.so not built yet -> multi_gpu_batch skipped"
fi

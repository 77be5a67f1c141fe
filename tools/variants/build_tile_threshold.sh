#!/bin/bash
# A throwaway build of the library with another row-path threshold in cm3_rows_tile (csrc/batch.hip, kTileRowMinBytes), for
# tools/checkers_phase_timing.py rows:   tools/variants/build_tile_threshold.sh <bytes> <name>
#   -> tools/variants/libcm3_hip_<name>.so   (load it with CM3_AMD_LIB; 16 = the row path wherever it applies, 2147483647 = never)
# Only batch.hip is compiled again, from a patched copy; the other objects are the product build's (run cm3_amd/csrc/build.sh first).
set -euo pipefail
BYTES="$1"; NAME="$2"
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
CSRC="${HERE}/../../cm3_amd/csrc"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
WORK="${HERE}/_${NAME}"
mkdir -p "${WORK}"
grep -q "constexpr uint32_t kTileRowMinBytes = [0-9]*;" "${CSRC}/batch.hip"
sed "s/constexpr uint32_t kTileRowMinBytes = [0-9]*;/constexpr uint32_t kTileRowMinBytes = ${BYTES};/" "${CSRC}/batch.hip" > "${WORK}/batch.hip"
"${HIPCC}" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function \
  -I"${CSRC}" -I"${HERE}/../../include" -DCM3_SOURCE_ID="\"variant-${NAME}\"" -c "${WORK}/batch.hip" -o "${WORK}/batch.o"
OBJS=()
for f in "${CSRC}"/_obj/*.o; do
  [ "$(basename "$f")" = "batch.o" ] || OBJS+=("$f")
done
"${HIPCC}" --offload-arch=gfx950 -shared -fPIC -o "${HERE}/libcm3_hip_${NAME}.so" "${WORK}/batch.o" "${OBJS[@]}"
echo "built ${HERE}/libcm3_hip_${NAME}.so"

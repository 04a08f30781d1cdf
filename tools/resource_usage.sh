# Per-kernel VGPR / SGPR / spill / LDS / occupancy of libmerging_hip's device code (hipcc's
# kernel-resource-usage remarks), for a source file (default: the product source).
# Usage: bash tools/resource_usage.sh [file.hip] > out.txt
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=${1:-$ROOT/merging-gym_amd/csrc/merging_hip.hip}
# build.py's flags without the two that only matter when linking the library
FLAGS=$(PYTHONPATH=$ROOT/merging-gym_amd python3 -c "from merging_gym import build; print(' '.join(f for f in build.HIPCC_FLAGS if f not in ('-shared', '-fPIC')))")
/opt/rocm/bin/hipcc $FLAGS --cuda-device-only -c \
  -I ${INC:-$ROOT/include} -Rpass-analysis=kernel-resource-usage -o /dev/null "$SRC" 2>&1 \
  | grep -E "Function Name|VGPRs:|AGPRs|ScratchSize|Occupancy|LDS Size|SGPRs Spill|VGPRs Spill" \
  | sed -E 's/^.*remark: //'

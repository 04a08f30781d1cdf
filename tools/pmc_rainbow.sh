# SQ compute-side counters of the Rainbow rollout kernels (tools/profile_rainbow.py), one pass per group and
# nothing traced beside them: VALU / SALU issue, the MFMA pipe, the instruction mix, the wave time split, LDS.
# Usage (on the GPU, from anywhere): bash tools/pmc_rainbow.sh OUTDIR
set -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
O=${1:?usage: bash tools/pmc_rainbow.sh OUTDIR}
mkdir -p $O
i=0
for set in "VALUBusy SALUBusy" "MfmaUtil SQ_INSTS_MFMA" "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES" \
           "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY" \
           "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU"; do
  i=$((i+1))
  timeout -s KILL 120 rocprofv3 --pmc $set --output-format csv -d $O/p$i -o p -- python tools/profile_rainbow.py > $O/p$i.log 2>&1 || { echo "pass $i ($set) failed"; tail -5 $O/p$i.log; exit 1; }
  echo "pass $i ok"
done

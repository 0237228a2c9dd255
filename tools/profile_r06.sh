# Round-6 measurement set:  bash tools/profile_r06.sh [tag] [output directory, default profile_out]
#   bench line (--full) -> rocprofv3 kernel stats -> separate PMC passes (never combined with tracing domains):
#   FETCH_SIZE, WRITE_SIZE, SQ_VALU_MFMA_BUSY_CYCLES + GRBM_GUI_ACTIVE (tools/pmc_summary.py), and the dynamic
#   instruction mix / wait cycles per kernel (tools/pmc_instmix.py: the executed counterpart of tools/issue_census.py).
# Copy <output directory>/<tag>_{bench.json,kernel_stats.csv,pmc_summary.json,instmix.json} into profiles/ afterwards.
set -e
T=${1:-r06}
cd "$(dirname "$0")/.."
O=${2:-profile_out}
mkdir -p "$O"
python bench.py --full > $O/${T}_bench.json 2> $O/${T}_bench.err
tail -c 400 $O/${T}_bench.json
P="--no-cpu-baseline --no-self-check --no-batch1"
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${T}_prof_stats -- python3 bench.py --steps 3 --warmup 3 $P > $O/${T}_prof_stats.log 2>&1
echo stats done
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --output-format csv --pmc $c -d $O/${T}_pmc_$c -- python3 bench.py --steps 2 --warmup 1 $P > $O/${T}_pmc_$c.log 2>&1
  echo pmc $c done
done
rocprofv3 --kernel-trace --output-format csv --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE -d $O/${T}_pmc_SQ -- python3 bench.py --steps 2 --warmup 1 $P > $O/${T}_pmc_SQ.log 2>&1
echo pmc sq done
python tools/pmc_summary.py $O/${T}_pmc_FETCH_SIZE $O/${T}_pmc_WRITE_SIZE $O/${T}_pmc_SQ > $O/${T}_pmc_summary.json
i=0
for group in "SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_SALU" \
             "SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_MUL_F32" \
             "SQ_INSTS_VALU_INT32 SQ_INSTS_VMEM SQ_INSTS_SMEM SQ_INSTS_VALU_CVT" \
             "SQ_BUSY_CU_CYCLES SQ_ACTIVE_INST_VALU SQ_VALU_MFMA_COEXEC_CYCLES SQ_ACTIVE_INST_LDS" \
             "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_WAIT_ANY" \
             "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_ANY SQ_INSTS_VALU_MFMA_MOPS_F32"; do
  i=$((i+1))
  rocprofv3 --kernel-trace --output-format csv --pmc $group -d $O/${T}_mix_$i -- python3 bench.py --steps 2 --warmup 1 $P > $O/${T}_mix_$i.log 2>&1 || { echo "mix pass $i failed"; tail -5 $O/${T}_mix_$i.log; }
  echo mix $i done
done
python tools/pmc_instmix.py $O/${T}_pmc_SQ $O/${T}_mix_* > $O/${T}_instmix.json
find $O/${T}_prof_stats -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/${T}_kernel_stats.csv
# keep the merged payload small
rm -rf $O/${T}_pmc_FETCH_SIZE $O/${T}_pmc_WRITE_SIZE $O/${T}_pmc_SQ $O/${T}_prof_stats $O/${T}_mix_[0-9]
ls -la "$O" | tail -12

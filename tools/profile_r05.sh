# Round-5 measurement set:  bash tools/profile_r05.sh [tag] [output directory, default profile_out]
#   bench line (--full) -> rocprofv3 kernel stats -> three separate PMC passes (FETCH_SIZE, WRITE_SIZE,
#   SQ_VALU_MFMA_BUSY_CYCLES + GRBM_GUI_ACTIVE; never combined with tracing domains) -> per-kernel summary JSON.
# Copy <output directory>/<tag>_{bench.json,kernel_stats.csv,pmc_summary.json} into profiles/ afterwards.
set -e
T=${1:-r05}
cd "$(dirname "$0")/.."
O=${2:-profile_out}
mkdir -p "$O"
python bench.py --full > $O/${T}_bench.json 2> $O/${T}_bench.err
tail -c 600 $O/${T}_bench.json
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
find $O/${T}_prof_stats -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/${T}_kernel_stats.csv
# keep the merged payload small
rm -rf $O/${T}_pmc_FETCH_SIZE $O/${T}_pmc_WRITE_SIZE $O/${T}_pmc_SQ $O/${T}_prof_stats
ls -la "$O" | tail -12

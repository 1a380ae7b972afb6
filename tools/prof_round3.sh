# Round-3 profiles (run on the GPU box from the repo root): tools/prof_round3.sh OUTDIR - kernel stats of the bench command,
# then separate --pmc passes (HBM FETCH_SIZE / WRITE_SIZE, MFMA busy) over a few single-stream L=2 closures, summarised
# into OUTDIR/r03_*.
set -o pipefail
O=$(mkdir -p "${1:?usage: tools/prof_round3.sh OUTDIR}" && cd "$1" && pwd)
R=$PWD
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_stats $O/pmc_fetch $O/pmc_write $O/pmc_mfma
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_stats -- python3 $R/bench.py --full --no-cpu-baseline --no-extras > $O/r03_bench_profiled.json 2> $O/bench_profiled.err; echo "stats rc $?"
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 $R/tools/pmc_run.py 3 2 > /dev/null 2>&1; echo "fetch rc $?"
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 $R/tools/pmc_run.py 3 2 > /dev/null 2>&1; echo "write rc $?"
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_WAIT_ANY --output-format csv -d $O/pmc_mfma -- python3 $R/tools/pmc_run.py 3 2 > /dev/null 2>&1; echo "mfma rc $?"
cd $R
cp $(find $O/prof_stats -name "*kernel_stats.csv" | head -1) $O/r03_bench_default_kernel_stats.csv
python tools/summarize_pmc.py traffic $O/pmc_fetch $O/pmc_write $O/r03_pmc_hbm_traffic_per_closure.txt $O/r03_pmc_hbm_traffic.json; echo "traffic rc $?"
python tools/summarize_pmc.py mfma $O/pmc_mfma $O/r03_pmc_mfma_util_conv.txt; echo "mfma summary rc $?"
rm -rf $O/prof_stats $O/pmc_fetch $O/pmc_write $O/pmc_mfma
python bench.py --full --steps 20 --warmup 5 > $O/r03_bench_default.json 2> $O/bench_default.err; echo "bench rc $?"

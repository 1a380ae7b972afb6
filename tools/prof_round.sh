# Round-2 profile passes (run on the GPU box from the repo root): tools/prof_round.sh OUTDIR
set -o pipefail
O=$(mkdir -p "${1:?usage: tools/prof_round.sh OUTDIR}" && cd "$1" && pwd)
export NST_TEST_REPORT=$O/parity_report.txt; rm -f $NST_TEST_REPORT
python -m pytest tests -m gpu -q > $O/gputest10.log 2>&1; echo "pytest rc $?"; tail -3 $O/gputest10.log
R=$PWD
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_stats -- python3 $R/bench.py --full --no-cpu-baseline --no-extras > $O/bench_profiled.json 2> $O/bench_profiled.err; echo "stats rc $?"
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 $R/tools/pmc_run.py 3 2 > /dev/null 2>&1; echo "fetch rc $?"
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 $R/tools/pmc_run.py 3 2 > /dev/null 2>&1; echo "write rc $?"
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_WAIT_ANY --output-format csv -d $O/pmc_mfma -- python3 $R/tools/pmc_run.py 3 2 > /dev/null 2>&1; echo "mfma rc $?"
cd $R
find $O/prof_stats -name "*kernel_stats.csv" | head -2
python bench.py --full --steps 20 --warmup 5 > $O/bench_r02b.json 2> $O/bench_r02b.err; echo "bench rc $?"

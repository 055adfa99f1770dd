# one gpurun call: GPU tests, bench line, kernel trace of the bench command, the three PMC passes of `bench.py --pmc-run`
# (SQ counters, FETCH_SIZE, WRITE_SIZE: separate passes, program directly after `--`), PMC pass of the sweeps.
# usage: bash tools/r03_measure.sh <tag> [notest]; every step stops the script when it fails.
set -o pipefail
V=${1:-r03_v1}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-measure_out}; mkdir -p "$OUT"  # where every output of this script goes
if [ "$2" != "notest" ]; then
timeout -k 10 900 python -m pytest tests -m gpu -q --durations=8 > $OUT/gputest_${V}.log 2>&1 || { tail -40 $OUT/gputest_${V}.log; exit 1; }; tail -4 $OUT/gputest_${V}.log
fi
timeout -k 10 600 python bench.py --full > $OUT/bench_${V}.json 2> $OUT/bench_${V}.err || { tail -5 $OUT/bench_${V}.err; exit 1; }
python3 tools/sweep_bench.py --shapes 1000000,128,1024 1000000,128,32 1000000,128,1 1250000,256,1024 1250000,256,32 1250000,256,1 3415,128,1024 --reps 20 > $OUT/sweep_bench_${V}.txt 2>&1 || { tail -5 $OUT/sweep_bench_${V}.txt; exit 1; }; cat $OUT/sweep_bench_${V}.txt
rm -rf $OUT/prof_bench $OUT/pmc_c2_sq $OUT/pmc_c2_fetch $OUT/pmc_c2_write $OUT/pmc_sweep3
rocprofv3 --kernel-trace --stats -d $OUT/prof_bench -- python3 bench.py --pmc-run --steps 5 --warmup 2 > $OUT/prof_bench.log 2>&1 || { tail -5 $OUT/prof_bench.log; exit 1; }
python3 tools/rocpd_kernels.py $(ls $OUT/prof_bench/*/*.db | head -1) k_path_step > $OUT/c2_b4096_kernels_${V}.txt 2>&1; head -14 $OUT/c2_b4096_kernels_${V}.txt
rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU --output-format csv -d $OUT/pmc_c2_sq -- python3 bench.py --pmc-run --steps 5 --warmup 2 > $OUT/pmc_c2_rows.json 2> $OUT/pmc_c2_sq.err || { tail -5 $OUT/pmc_c2_sq.err; exit 1; }
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_c2_fetch -- python3 bench.py --pmc-run --steps 5 --warmup 2 > $OUT/pmc_c2_fetch.log 2>&1 || { tail -5 $OUT/pmc_c2_fetch.log; exit 1; }
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_c2_write -- python3 bench.py --pmc-run --steps 5 --warmup 2 > $OUT/pmc_c2_write.log 2>&1 || { tail -5 $OUT/pmc_c2_write.log; exit 1; }
python3 tools/r03_pmc.py $OUT/pmc_c2_sq $OUT/pmc_c2_fetch $OUT/pmc_c2_write $OUT/pmc_c2_rows.json $OUT/c2_b4096_pmc_${V}.json || exit 1
rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d $OUT/pmc_sweep3 -- python3 tools/sweep_bench.py --shapes 1000000,128,1024 1250000,256,1024 --reps 3 > $OUT/pmc_run.log 2>&1 || { tail -5 $OUT/pmc_run.log; exit 1; }
python3 tools/pmc_summary.py $OUT/pmc_sweep3 k_sweep k_select k_refine k_prep > $OUT/sweep_pmc_${V}.txt; cat $OUT/sweep_pmc_${V}.txt

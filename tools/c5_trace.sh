# kernel trace of the bench's C4 / C5 legs only (small C2 part): which kernels make a C5 beam step; usage: bash tools/c5_trace.sh
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-measure_out}; mkdir -p "$OUT"  # where every output of this script goes
rm -rf $OUT/prof_c5
rocprofv3 --kernel-trace --stats -d $OUT/prof_c5 -- python3 bench.py --full --no-cpu-baseline --no-c3 --no-scoring --batch 64 --steps 2 --warmup 1 --c4-batch 64 --c4-steps 1 > $OUT/prof_c5.log 2>&1 || { tail -5 $OUT/prof_c5.log; exit 1; }
python3 tools/rocpd_kernels.py $(ls $OUT/prof_c5/*/*.db | head -1) k_beam_step > $OUT/c5_kernels.txt 2>&1; head -30 $OUT/c5_kernels.txt

#!/bin/bash
# The round's final measurement set (run on the MI355X box; copy $OUT/final/* into profiles/ as r<N>_final_*):
#   1. the driver's command with every leg (--full) -> final/bench_steps20.json
#   2. the default window, unprofiled              -> final/bench.json
#   3. the driver's command's timed path under rocprofv3 --kernel-trace --stats
#                                                  -> final/kernel_stats.csv, final/under_rocprof.json,
#                                                     final/spmv_working_dispatches.json
# OUT: the results directory (default bench_out, git-ignored), shared with scripts/prof_bench.sh
export OUT=${OUT:-bench_out}
mkdir -p $OUT/final
python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/final/bench_steps20.json 2> $OUT/final/bench_steps20.err || exit 1
python3 bench.py --main-only --no-cpu-baseline > $OUT/final/bench.json 2> $OUT/final/bench.err || exit 1
bash scripts/prof_bench.sh final --steps 20 --warmup 5 > $OUT/final/prof.txt 2>&1 || exit 1
cp $OUT/prof_bench/final_kernel_stats.csv $OUT/final/kernel_stats.csv
cp $OUT/prof_bench_final_line.json $OUT/final/under_rocprof.json
python3 scripts/rocprof_filtered_avg.py $OUT/prof_bench/final_kernel_trace.csv $OUT/final/spmv_working_dispatches.json
head -30 $OUT/final/prof.txt

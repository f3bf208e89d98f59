#!/bin/bash
# rocprofv3 --kernel-trace --stats of sim3opt_covariances on KITTI-00 (one loop / all loops; 1000 random pairs / one
# full block column; marginal_covariances next to them), one run each, no counters -> $OUT/cov_prof/<tag>_*.csv and
# the per-kernel medians in $OUT/covariances_kernel_medians.csv (OUT: default bench_out, git-ignored)
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT/cov_prof
for which in one all; do
  for what in pairs column marginals; do
    timeout -k 10 120 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/cov_prof -o ${which}_${what} -- \
      python3 scripts/gpu_cov_prof.py $which $what >> $OUT/cov_prof.log 2>&1 || { echo "run $which $what failed"; tail -5 $OUT/cov_prof.log; exit 1; }
  done
done
grep "wall median" $OUT/cov_prof.log
python3 scripts/gpu_cov_prof.py summarise $OUT/cov_prof $OUT/covariances_kernel_medians.csv

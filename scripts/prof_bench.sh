#!/bin/bash
# rocprofv3 --kernel-trace --stats of the timed path of bench.py -> $OUT/prof_bench/<tag>_kernel_stats.csv
# (OUT: the results directory, default bench_out, git-ignored)
TAG=${1:-bench}
shift
cd /tmp && export TMPDIR=/tmp && cd ${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-bench_out}
mkdir -p $OUT
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_bench -o $TAG -- python3 bench.py --main-only --no-cpu-baseline "$@" > $OUT/prof_bench_$TAG.log 2>&1
grep -m1 "^{\"metric\"" $OUT/prof_bench_$TAG.log > $OUT/prof_bench_${TAG}_line.json
python3 - <<PY
import csv
rows=list(csv.DictReader(open("$OUT/prof_bench/${TAG}_kernel_stats.csv")))
tot=sum(float(r["TotalDurationNs"]) for r in rows)
print("total kernel ms %.1f"%(tot/1e6))
for r in rows[:28]:
    print("%8.2f ms %6d x %8.1f us  %s"%(float(r["TotalDurationNs"])/1e6,int(r["Calls"]),float(r["AverageNs"])/1e3,r["Name"][:110]))
PY

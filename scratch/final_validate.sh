#!/bin/bash
# round-end validation on the GPU box: full GPU test suite, smoke, profiles of the default bench command and of the train step
#   bash scratch/final_validate.sh OUT_DIR      (run from anywhere; everything it writes goes to OUT_DIR)
# Every GPU step runs under its own time limit and the script stops at the first step that fails, faults or times out.
set -eo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${1:?usage: final_validate.sh OUT_DIR}" && cd "$1" && pwd)
cd $R
timeout -k 10 400 python -m pytest tests -q -m gpu 2>&1 | tail -3
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout -k 10 900 python bench.py --full 2>&1 | tail -1 > $OUT/bench_line_final.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d $OUT/prof_v9 -o bench -- python $R/bench.py --full --no-cpu-baseline > $OUT/prof_v9_bench.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_v9t -o train -- python $R/bench.py --mode train --steps 20 --warmup 3 > $OUT/prof_v9_train.log 2>&1
cd $R
python tools/rocprof_summary.py $OUT/prof_v9/bench_results.db $OUT/r1_bench_kernel_stats_v10.md "rocprofv3 --kernel-trace --stats -- python bench.py --full --no-cpu-baseline  (default workload: warm-up 5 + 50 timed steps on one stream)" first 55
python tools/rocprof_summary.py $OUT/prof_v9t/train_results.db $OUT/r1_train_kernel_stats_v10.md "rocprofv3 --kernel-trace --stats -- python bench.py --mode train --steps 20 --warmup 3  (train step: sample, solve, best-of-10 vs GT, MatchLoss, backward to the logits)"
tail -1 $OUT/prof_v9_bench.log | cut -c1-200
rm -rf $OUT/prof_v9 $OUT/prof_v9t

#!/bin/bash
# rocprofv3 kernel stats of the C3 bench under two environments: tools/prof_ab.sh "ENV_A" "ENV_B"
# (--full: the profile covers the fp32 companion and the roofline's eager step as well).
# Output goes to $BENCH_OUT (default: bench_out/ in the repository).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${BENCH_OUT:-$R/bench_out}; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
i=0
for E in "$@"; do
  i=$((i+1))
  env $E timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/pab_$i -o run -- \
    python $R/bench.py --steps 5 --warmup 2 --full --no-cpu-baseline > $OUT/pab_$i.log 2>&1 || exit 1
  echo "== $E"; python $R/tools/prof_summary.py $OUT/pab_$i 7 | head -16
done

#!/bin/bash
# bench.py lines of every BASELINE.json configuration (N = 1).  usage: r2_bench_configs.sh <output directory>
O=$(realpath "${1:?output directory}")
cd "$GRAFT_REPO_ROOT"
for c in 2 3 5; do
  echo "== config $c"
  timeout -k 10 500 python bench.py --full --config $c --steps 10 --warmup 2 2>$O/r2_bench_cfg$c.err | tee $O/r2_bench_cfg$c.json | cut -c1-1500
  tail -3 $O/r2_bench_cfg$c.err
done

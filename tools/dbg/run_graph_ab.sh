#!/bin/bash
# bench.py at 1000 images: eager launches against one HIP-graph replay per batch, alternating
O=${1:?usage: run_graph_ab.sh <out-dir>}
mkdir -p $O
for i in 1 2 3; do
  for g in off on; do
    python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --graph $g > $O/bench_$g.json 2> $O/bench_$g.err
    python - <<PY >> $O/ab.txt
import json
d=json.loads(open("$O/bench_$g.json").read().strip().splitlines()[-1])
print("graph $g", d["value"], d["ms_per_step"], d.get("value_synchronous"))
PY
  done
done
cat $O/ab.txt

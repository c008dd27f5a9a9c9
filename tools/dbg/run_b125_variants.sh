#!/bin/bash
# the 125-image step under process-wide kernel variants: usage run_b125_variants.sh <out-dir> <variant> <variant> ...
O=${1:?usage: run_b125_variants.sh <out-dir> <variant> ...}; shift
mkdir -p $O
for i in 1 2; do
  for v in "$@"; do
    I8IE_KERNEL_VARIANT=$v python bench.py --full --batch 125 --steps 100 --warmup 5 --no-cpu-baseline > $O/b_$v.json 2> $O/b_$v.err
    python - <<PY >> $O/ab.txt
import json
d=json.loads(open("$O/b_$v.json").read().strip().splitlines()[-1])
print("variant $v", d["value"], d["ms_per_step"], d["kernel_ms_per_step"])
PY
  done
done
cat $O/ab.txt

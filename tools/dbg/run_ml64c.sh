#!/bin/bash
# Linear / API tests, then the AlexNet step at shard sizes where the many-row Linear kernel's row tile matters
O=${1:?usage: run_ml64c.sh <out-dir>}
mkdir -p $O
timeout -k 10 600 python -m pytest tests/test_gpu_mlin.py tests/test_gpu_parity.py tests/test_gpu_api.py -m gpu -q -x > $O/tests.log 2>&1; echo "tests rc $?" >> $O/tests.log; tail -3 $O/tests.log
for b in 500 384 1000; do
  python bench.py --full --batch $b --steps 30 --warmup 5 --no-cpu-baseline > $O/b$b.json 2> $O/b$b.err
  python - <<PY
import json
d=json.loads(open("$O/b$b.json").read().strip().splitlines()[-1]); print($b, d["value"], d["ms_per_step"], d["kernel_ms_per_step"], d["parity"]["logits_bit_exact_vs_oracle"])
PY
done

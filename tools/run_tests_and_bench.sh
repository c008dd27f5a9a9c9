# the GPU suite, then the full bench line: usage run_tests_and_bench.sh <out-dir>
O=${1:?usage: run_tests_and_bench.sh <out-dir>}
mkdir -p $O
python -m pytest tests -m gpu -x -q > $O/tests.log 2>&1; echo "tests rc $?" >> $O/tests.log; tail -4 $O/tests.log
python bench.py --steps 20 --warmup 5 --full > $O/bench.json 2> $O/bench.err
python - <<PY
import json
d=json.loads(open("$O/bench.json").read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["kernel"], d["roofline"]["frac"]); print(d["kernel_ms_per_step"])
PY
tail -2 $O/bench.err

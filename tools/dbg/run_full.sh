O=${1:?usage: run_full.sh <out-dir>}
mkdir -p $O
python -m pytest tests -m gpu -q > $O/tests.log 2>&1; echo "tests rc $?" >> $O/tests.log; tail -6 $O/tests.log
timeout -k 10 300 python tools/calib_time.py device > $O/calib_time.txt 2>&1; tail -6 $O/calib_time.txt
python bench.py --full --steps 20 --warmup 5 > $O/bench.json 2> $O/bench.err
python - <<PY
import json
d=json.loads(open("$O/bench.json").read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["kernel"], d["roofline"]["frac"], d["fp32_engine_path"]["images_per_sec"], d["parity"]); print(d["kernel_ms_per_step"])
PY

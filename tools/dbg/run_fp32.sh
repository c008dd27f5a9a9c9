O=${1:?usage: run_fp32.sh <out-dir>}
mkdir -p $O
timeout -k 10 600 python -m pytest tests/test_gpu_api.py tests/test_gpu_calibration_device.py tests/test_gpu_serialization.py -m gpu -q > $O/tests_api.log 2>&1; echo "tests rc $?" >> $O/tests_api.log; tail -4 $O/tests_api.log
timeout -k 10 300 python tools/calib_time.py device > $O/calib_time.txt 2>&1; tail -12 $O/calib_time.txt
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $O/bench.json 2> $O/bench.err
python - <<PY
import json
d=json.loads(open("$O/bench.json").read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["kernel"], d["roofline"]["frac"], d["fp32_engine_path"]); print(d["kernel_ms_per_step"])
PY

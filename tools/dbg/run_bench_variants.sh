O=${1:?usage: run_bench_variants.sh <out-dir>}
mkdir -p $O
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $O/bench_v0.json 2> $O/bench_v0.err
I8IE_KERNEL_VARIANT=50 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $O/bench_v50.json 2> $O/bench_v50.err
python - <<PY
import json
for v in ("v0","v50"):
    d=json.loads(open("$O/bench_%s.json"%v).read().strip().splitlines()[-1])
    print(v, d["value"], d["ms_per_step"], d["roofline"]["kernel"], d["roofline"]["frac"]); print(d["kernel_ms_per_step"])
PY

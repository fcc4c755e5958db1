#!/bin/bash
# One perf iteration on the GPU box: GPU suite, C3 / C2 / bounds bench lines, stamps (bounds).
# usage (under gpurun): bash tools/perf_check.sh <tag>
set -u
TAG=${1:-dev}
O=${BENCH_OUT:-bench_out}
mkdir -p $O
bash tools/gpu_tests.sh $TAG || exit $?
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/b3_$TAG.json 2> $O/b3_$TAG.err || exit $?
timeout -k 10 300 python bench.py --full --no-cpu-baseline --continuous > $O/b2_$TAG.json 2> $O/b2_$TAG.err || exit $?
timeout -k 10 300 python bench.py --full --no-cpu-baseline --done-on-bounds --steps 200 > $O/bb_$TAG.json 2> $O/bb_$TAG.err || exit $?
if [ -f cartpoleplusplus_amd/libcartpole_hip_stamps.so ]; then
  CP_LIB_PATH=$PWD/cartpoleplusplus_amd/libcartpole_hip_stamps.so BOUNDS=1 STEPS=60 timeout -k 10 300 python tools/stamps.py > $O/stb_$TAG.json 2>/dev/null || exit $?
fi
python - "$TAG" "$O" <<'PY'
import json, sys
t, o = sys.argv[1:3]
for k in ("b3", "b2", "bb"):
    d = json.load(open(f"{o}/{k}_{t}.json"))
    print(k, "value", d["value"], "ms/step", d["ms_per_step"], "kernel", d["roofline"]["avg_launch_ms"],
          "reset", d["roofline"]["reset_kernel_avg_ms"], "steady", d["steady_state"]["value"])
try:
    s = json.load(open(f"{o}/stb_{t}.json"))["reset_kernel"]
    print("reset stamps", {k: round(v) for k, v in s["cycles_per_wave_substep"].items()}, "sweeps",
          round(s["sweeps_per_wave_substep"], 1), "cyc/sweep", round(s["cycles_per_sweep"]))
except Exception as e:
    print("no stamps", e)
PY

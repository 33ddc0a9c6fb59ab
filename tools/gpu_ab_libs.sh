#!/bin/bash
# gpu_ab_libs.sh TAG LIB... -- on the MI355X box: tools/time_fused.py (fused gradient, gradient + optimizer) with each library in turn, twice
# (LIB = a path under fly_bproject_amd/, e.g. libflyhip.so libflyhip_ab.so: A/B builds of one source tree, selected through FLYHIP_LIB)
# AB_BENCH=1: the benchmark line instead (bench.py --steps 20 --warmup 5, PPO only), AB_ROUNDS times each (default 3), alternating; one
# line per run with ms_per_step and the graph-replay time of the optimizer launch, the JSON lines kept beside the logs, under TAG
TAG=$1; shift
OUT=gpurun_out/$TAG
mkdir -p $OUT
if [ "${AB_BENCH:-0}" = 1 ]; then
  for i in $(seq 1 ${AB_ROUNDS:-3}); do
    for lib in "$@"; do
      f=$OUT/bench_${lib%.so}_$i
      FLYHIP_LIB=$PWD/fly_bproject_amd/$lib timeout -k 10 400 python bench.py --gpus 1 --steps 20 --warmup 5 --no_cpu_baseline --no_dqn --no_alt_gemm > $f.txt 2>&1 || { tail -5 $f.txt; exit 1; }
      grep -m1 '^{' $f.txt > $f.json
      python - $f.json "$lib $i" <<'PY' || exit 1
import json, sys
d = json.load(open(sys.argv[1]))
k = {e["kernel"].split(" ")[0]: e["avg_launch_us"] for e in d.get("kernels", []) if "avg_launch_us" in e}
r = d.get("roofline") or {}
print("%s: ms_per_step %.3f  adam_apply (graph replay) %.3f us  %s %s us" % (
    sys.argv[2], d["ms_per_step"], k.get("mlp_adam_apply_kernel", float("nan")), r.get("kernel", "?").split(" ")[0] + " + reduction",
    r.get("avg_launch_us", "?")))
PY
    done
  done
  echo "ab bench done"
  exit 0
fi
for i in 1 2; do
  for lib in "$@"; do
    FLYHIP_LIB=$PWD/fly_bproject_amd/$lib timeout -k 10 200 python tools/time_fused.py 40960 200 > $OUT/time_${lib%.so}_$i.txt 2>&1 || exit 1
    echo "$lib $i: $(grep -m1 f16x2 $OUT/time_${lib%.so}_$i.txt | cut -c1-90)"
  done
done
echo "ab libs done"

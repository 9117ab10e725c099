#!/bin/bash
# Interleaved A/B of library builds on the plain bench line (no --full), in one GPU call:
#   tools/ab_steps.sh label:libdir label:libdir ...   [REPS=3 STEPS=10 WARMUP=3 BENCH_ARGS="--scene random" SWAP=1]
# Runs the specs in order REPS times (P C P C P C); SWAP=1 reverses the order every other round, which
# separates a build's effect from the box's slow drifts.  A libdir is a directory under go-raytracing_amd/
# (RTGPU_LIB_DIR; tools/build_variant.sh builds a git revision into lib_<name>).  Prints per run: tag,
# Msamples/s, config.frame_sum, ms per step; every run's whole line stays in $BENCH_OUT.
set -o pipefail
OUT=${BENCH_OUT:-bench_out}
mkdir -p $OUT
specs=("$@")
for rep in $(seq 1 ${REPS:-3}); do
  order=("${specs[@]}")
  if [ -n "$SWAP" ] && [ $((rep % 2)) -eq 0 ]; then
    order=()
    for ((i = ${#specs[@]} - 1; i >= 0; i--)); do order+=("${specs[i]}"); done
  fi
  for spec in "${order[@]}"; do
    IFS=: read -r label lib <<< "$spec"
    tag=${label}_$rep
    RTGPU_LIB_DIR=${lib:-lib} timeout -k 10 300 python3 bench.py --gpus 1 --steps ${STEPS:-10} --warmup ${WARMUP:-3} $BENCH_ARGS \
      > $OUT/abs_$tag.json 2> $OUT/abs_$tag.err || { tail -20 $OUT/abs_$tag.err; exit 1; }
    python3 - "$tag" "$OUT" <<'PY'
import json, sys
tag, out = sys.argv[1:3]
d = json.loads(open(f"{out}/abs_{tag}.json").read().strip().splitlines()[-1])
print(tag, d["value"], d.get("unit"), "frame_sum", repr(d["config"].get("frame_sum")), "ms_per_step", d.get("ms_per_step"), flush=True)
PY
  done
done

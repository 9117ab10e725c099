#!/bin/bash
# Round-end refresh on one GPU box: GPU tests, the full bench line (with
# the CPU baseline), the rocprof kernel-trace + PMC traffic passes, the PMC
# counter passes and one bench line per BASELINE config.  Every GPU step has
# its own time limit; the script stops at the first failure.  Everything is
# written under $BENCH_OUT (default bench_out/).
set -o pipefail
OUT=${BENCH_OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python3 -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { tail -30 $OUT/gpu_tests.log; exit 1; }
tail -1 $OUT/gpu_tests.log
# the fp32-vs-fp64 tolerance figures per BASELINE config (printed by the test)
timeout -k 10 300 python3 -u -m pytest tests/test_gpu_parity.py -m gpu -k "fp64 or three_passes" -q -s --timeout 120 --timeout-method thread > $OUT/fp64_tolerance.log 2>&1 || { tail -30 $OUT/fp64_tolerance.log; exit 1; }
timeout -k 10 300 python3 bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 1; }
cat $OUT/bench.json
OUT=$OUT/prof bash tools/profile_round.sh || exit 1
OUT=$OUT/pmc bash tools/pmc_profile.sh || exit 1
bash tools/configs_round.sh || exit 1
echo refresh-done

#!/bin/bash
# GPU session: parity tests, then bench.py on every BASELINE config, then a
# kernel-trace of the general-path configs.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
OUT=${KCEP_OUT:-out}                     # where the logs go (KCEP_OUT overrides)
mkdir -p $OUT/prof
export TMPDIR=/tmp
TAG=${1:-run}
timeout -k 10 600 python -u -m pytest tests -m gpu -q -rf --timeout 120 --timeout-method thread > $OUT/pytest_gpu_$TAG.log 2>&1; rc=$?
tail -15 $OUT/pytest_gpu_$TAG.log
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit 1
for c in c2 c3 c4 c5; do
  timeout -k 10 300 python -u bench.py --full --config $c --steps 5 --warmup 1 > $OUT/bench_${c}_$TAG.log 2>&1 || { tail -20 $OUT/bench_${c}_$TAG.log; exit 1; }
  tail -1 $OUT/bench_${c}_$TAG.log
done
for c in c3 c5; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -T --output-format csv -d $OUT/prof/${TAG}_$c -o trace -- python3 bench.py --full --config $c --steps 2 --warmup 1 --no-cpu-baseline > $OUT/prof_${c}_$TAG.log 2>&1 || exit 1
done
echo done

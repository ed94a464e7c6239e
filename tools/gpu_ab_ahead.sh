#!/bin/bash
# DRA_VAR_TARGET_AHEAD A/B on one box: the bit-identity test, then interleaved driver-form / long runs of bench.py with the bit cleared and set.
# usage: gpurun -- 'bash tools/gpu_ab_ahead.sh <tag>'
TAG=${1:-ahead}; OUT=gpurun_out/$TAG; mkdir -p $OUT; export TMPDIR=/tmp
timeout 600 python -m pytest tests -q -m gpu -x -p no:cacheprovider -k "target_ahead" > $OUT/pytest.log 2>&1; tail -15 $OUT/pytest.log | cut -c1-300
DEF=$(python -c "from deeprl_amd import ops; print(ops.get_tuning() & ~ops.VAR_TARGET_AHEAD)")
ON=$(python -c "from deeprl_amd import ops; print(ops.get_tuning() | ops.VAR_TARGET_AHEAD)")
for rep in 1 2 3; do for V in $DEF $ON; do
  timeout 300 python bench.py --full --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --no-parity-check --variant $V 2>>$OUT/err.txt | python -c "
import sys,json
d=json.loads(sys.stdin.readline()); print(json.dumps({'variant': $V, 'driver_form': d['value'], 'long_run': d['long_run']['value'], 'host': d['host'].get('lane')}))" | tee -a $OUT/ab_ahead.jsonl | cut -c1-300
done; done
tail -3 $OUT/err.txt

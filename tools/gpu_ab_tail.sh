#!/bin/bash
# C4 pre-hash tail-wave count A/B (varlen_tail 1/2/3): varlen/c4 parity tests, then alternating bench runs.
OUT=${OUT:-build/ab_tail}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest -x -q --timeout 300 --timeout-method thread -m gpu tests/test_gpu_parity.py -k "varlen or c4 or prehash" > $OUT/tests.log 2>&1 || { tail -30 $OUT/tests.log; exit 1; }
tail -1 $OUT/tests.log
for r in 1 2 3; do for v in 1 2 3; do
  timeout -k 10 200 python bench.py --full --config c4 --steps 20 --warmup 3 --no-cpu-baseline --varlen-tail $v > $OUT/t$v.$r.json 2> $OUT/err || { tail $OUT/err; exit 1; }
  python3 -c "
import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(sys.argv[1].split('/')[-1], d['ms_per_step'], d.get('build_ms'), d.get('probe_ms'), d['parity'][:12])" $OUT/t$v.$r.json
done; done

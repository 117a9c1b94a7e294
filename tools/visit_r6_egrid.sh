#!/bin/bash
# bench line, same box, 3 drawings in flight: workgroups of the two one-wave-per-SIMD kernels of the NSR step
set -u
export PYTHONPATH=$(pwd) TMPDIR=/tmp
O=gpurun_out/${1:-r6_egrid2}; mkdir -p $O
for g in 256 128 96 64 160 128 256; do
  echo -n "onewave grid $g: " | tee -a $O/summary.txt
  timeout 900 python bench.py --full --steps 4 --warmup 1 --no-cpu-baseline --onewave-grid $g 2>/dev/null | tail -1 | python -c "import json,sys; j=json.loads(sys.stdin.read()); c=j['config']; print('value %.4f' % j['value'], 'latency %.2f' % c['latency_s']['mean'], {k: round(v,2) for k,v in c['stage_seconds_rank0'].items() if k in ('mv','nsr_fit','nsr_export','style','contour')})" | tee -a $O/summary.txt
done

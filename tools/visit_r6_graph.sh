#!/bin/bash
# bench line, same box, 3 drawings in flight: UNet evaluations as eager launches vs replayed HIP graphs
set -u
export PYTHONPATH=$(pwd) TMPDIR=/tmp
O=gpurun_out/${1:-r6_graph}; mkdir -p $O
for g in 0 1 0 1; do
  echo -n "DSU_MV_GRAPH=$g: " | tee -a $O/summary.txt
  DSU_MV_GRAPH=$g timeout 900 python bench.py --full --steps 4 --warmup 1 --no-cpu-baseline 2>$O/err_$g.txt | tail -1 | python -c "import json,sys; j=json.loads(sys.stdin.read()); c=j['config']; print('value %.4f' % j['value'], 'latency %.2f' % c['latency_s']['mean'], {k: round(v,2) for k,v in c['stage_seconds_rank0'].items() if k in ('mv','nsr_fit','nsr_export','style','contour')})" | tee -a $O/summary.txt
done
tail -3 $O/err_1.txt

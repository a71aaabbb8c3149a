# A/B of the dissection's separator absorption on one box: bash scripts/ab_absorb.sh
run() { python bench.py --full --workload $1 --steps 15 --warmup 3 --no-cpu-baseline --no-past-l3 --no-other-configs --sustained-seconds 0 2>/dev/null | python -c "
import sys, json
for l in sys.stdin:
    if l.startswith('{'):
        d=json.loads(l); p=d.get('phases_us_per_lm_step') or {}; print('$1 $2', d['value'], 'factor', p.get('factor'), 'backsolve', p.get('backsolve'))
"; }
for rep in 1 2; do
for w in c2 c3; do
  for a in 0 1; do BSGPU_DIM_ABSORB=$a run $w absorb=$a; done
done
done
for a in 0 1; do echo absorb=$a; BSGPU_DIM_ABSORB=$a python scripts/small_window.py | tail -4; done

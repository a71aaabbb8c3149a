#!/bin/bash
# C2 with the full (BSGPU_COMPACT_J=0) / the compact pose part of the reprojection Jacobian: kernel-trace averages + bench value, 0 / 1 / 0 / 1 on one box,
# then a window of the reference's size (20 KF x 500, below the band rule: full layout either way) both ways.  Every step under its own time limit; a failed
# step ends the call.   bash scripts/ab_compact_j.sh
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
set -e -o pipefail
line() {
  python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); p=d.get('phases_us_per_lm_step') or {}
print('value', d['value'], 'eval_reproj', p.get('eval_reproj'), 'pairs', p.get('pairs'), 'backsub', p.get('backsub'), 'cost %.12e' % d['config']['final_cost'])"
}
for v in 0 1 0 1; do
  echo "== BSGPU_COMPACT_J=$v"
  BSGPU_COMPACT_J=$v timeout -k 10 330 bash "$ROOT/scripts/kstats.sh" c2 14 2>&1 | grep -i "chol_\|landmark\|backsub\|pairs_band\|visual_imu_eval\|value"
  cd "$ROOT"; BSGPU_COMPACT_J=$v timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-other-configs --no-past-l3 --sustained-seconds 0 --steps 30 2>/dev/null | line
done
for v in 0 1 0 1; do
  echo "== 20 KF x 500, BSGPU_COMPACT_J=$v"
  cd "$ROOT"; BSGPU_COMPACT_J=$v timeout -k 10 300 python bench.py --full --n-kf 20 --n-lm 500 --no-cpu-baseline --no-other-configs --no-past-l3 --sustained-seconds 0 --steps 30 2>/dev/null | line
done

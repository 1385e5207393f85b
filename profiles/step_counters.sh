#!/bin/bash
# Issue counters and a kernel trace of the fused 32-step launch (profiles/step_fused.py), one library per call:
#   bash profiles/step_counters.sh <name> <out dir> [library]      (library: BLE_HIP_LIB; default: the in-tree one)
# Counters in a rocprofv3 --pmc pass of their own (kernel trace only), the trace with --stats in another.  Prints, per kernel whose name
# holds "ble_step", the counters per launch and per 64 environments and agent step, and the trace's statistics.
set -u -o pipefail
NAME=$1; OUT=$2; LIB=${3:-}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
[ -n "$LIB" ] && export BLE_HIP_LIB=$LIB
rm -rf $OUT/${NAME}_pmc $OUT/${NAME}_trace; mkdir -p $OUT
timeout -k 10 240 rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAIT_ANY \
    --output-format csv -d $OUT/${NAME}_pmc -o x -- python $ROOT/profiles/step_fused.py > $OUT/${NAME}_pmc.log 2>&1 || { echo "$NAME: counter pass failed"; tail -5 $OUT/${NAME}_pmc.log; exit 1; }
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${NAME}_trace -o x -- python $ROOT/profiles/step_fused.py > $OUT/${NAME}_trace.log 2>&1 || { echo "$NAME: trace pass failed"; tail -5 $OUT/${NAME}_trace.log; exit 1; }
grep "form of this launch" $OUT/${NAME}_pmc.log
python - "$NAME" "$OUT" <<'PY'
import collections, csv, glob, re, sys
short = lambda full: (re.search(r'ble_step\w*', full).group(0) + ('<noise>' if '<true' in full else ''))      # (names carry "(anonymous namespace)")
name, out = sys.argv[1], sys.argv[2]
by = collections.defaultdict(lambda: collections.defaultdict(list))
for p in glob.glob(f'{out}/{name}_pmc/**/*counter_collection.csv', recursive=True):
  for r in csv.DictReader(open(p)):
    if 'ble_step' in r['Kernel_Name']:
      by[short(r['Kernel_Name'])][r['Counter_Name']].append(float(r['Counter_Value']))
groups, steps = 65536 / 64, 32
for k, c in by.items():
  m = {q: sum(v[-8:]) / len(v[-8:]) for q, v in c.items()}           # the 8 launches after the warm-up
  print(f'{name} {k}: launches {len(next(iter(c.values())))}, waves per launch {m.get("SQ_WAVES", 0):.0f}')
  for q in ('SQ_INSTS_VALU', 'SQ_INSTS_SALU', 'SQ_WAVE_CYCLES', 'SQ_ACTIVE_INST_VALU', 'SQ_ACTIVE_INST_ANY', 'SQ_WAIT_ANY'):
    if q in m:
      print(f'  {q}: {m[q]:.4g} per launch, {m[q] / groups / steps:.1f} per 64 environments and agent step')
  if m.get('SQ_WAVE_CYCLES'):
    print(f'  valu_issue_frac {m["SQ_ACTIVE_INST_VALU"] / m["SQ_WAVE_CYCLES"]:.3f}  wait_frac {m["SQ_WAIT_ANY"] / m["SQ_WAVE_CYCLES"]:.3f}  '
          f'wave_issue_utilisation {m["SQ_ACTIVE_INST_ANY"] / m["SQ_WAVE_CYCLES"]:.3f}')
for p in glob.glob(f'{out}/{name}_trace/**/*kernel_stats.csv', recursive=True):
  for r in csv.DictReader(open(p)):
    if 'ble_step' in r['Name']:
      print(f'{name} trace: {short(r["Name"])}  calls {r["Calls"]}  average {float(r["AverageNs"]) / 1e3:.1f} us  min {float(r["MinNs"]) / 1e3:.1f}  max {float(r["MaxNs"]) / 1e3:.1f}')
PY

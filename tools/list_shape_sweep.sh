#!/bin/bash
# The sweep behind the list launches' defaults: lanes {rule, all 64, all 16} x workgroup target of the 16-lane
# launches {1,024, 2,048, 4,096} at the headline shape, three timed steps each, one rocprofv3 --kernel-trace --stats run per
# setting (the target does not touch 64-lane launches, so "all 64" runs once).  From the repository root, on a GPU box:
#   tools/list_shape_sweep.sh <output dir>  > profiles/rNN_list_shape_sweep.txt
# The per-launch traces (tens of MB a setting) are deleted once their phase table is printed: keep the printed output, the
# tables cannot be made again without a new run.  The run's JSON and rocprofv3's kernel_stats.csv stay in the output dir.
set -o pipefail
R="$(pwd)"
out="${1:-$R/build/list_shape_sweep}"
mkdir -p "$out"
echo "# tools/list_shape_sweep.sh: tools/list_shape_run.py --lanes L --target W --steps 3 --warmup 1 (10M x 2,504, select all) under rocprofv3 --kernel-trace --stats,"
echo "# one run per setting; wall ms per step are under the profiler (every launch traced); phases: tools/list_phases.py on the run's trace, ms per step"
for setting in "0 1024" "0 2048" "0 4096" "16 1024" "16 2048" "16 4096" "64 0"; do
  set -- $setting
  tag="lanes$1_wgs$2"
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/$tag" -- python3 "$R/tools/list_shape_run.py" --lanes "$1" --target "$2" --steps 3 --warmup 1 > "$out/$tag.json" 2> "$out/$tag.err"
  rc=$?
  if [ $rc -ne 0 ]; then echo "setting $setting: exit $rc"; tail -5 "$out/$tag.err"; exit $rc; fi
  python3 - "$out/$tag.json" "$1" "$2" <<'EOF'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().split("\n")[-1])
ms = d["ms_per_step"]
print(f"## lanes {sys.argv[2] if sys.argv[2] != '0' else 'rule'}, target {sys.argv[3] if sys.argv[3] != '0' else 'default'}: wall ms per step {' '.join('%.2f' % x for x in ms)} (median {sorted(ms)[len(ms) // 2]:.2f})")
EOF
  python3 "$R/tools/list_phases.py" "$out/$tag" "$out/$tag.json" "$tag" || exit 1
  find "$out/$tag" -name "*kernel_trace.csv" -delete
done

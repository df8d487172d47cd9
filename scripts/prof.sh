#!/bin/bash
# rocprofv3 kernel trace of bench.py --full; writes a compact per-kernel table to $RESULTS/prof_<tag>.txt (default results/)
cd "$(dirname "$0")/.." || exit 1
TAG=${1:-run}; shift
export RESULTS=${RESULTS:-results}
mkdir -p "$RESULTS"
export TMPDIR=/tmp
REPO=$PWD
(cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $REPO/$RESULTS/prof_$TAG -o p -- python $REPO/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-roofline --no-exact --no-graph "$@" > $REPO/$RESULTS/prof_$TAG.log 2>&1)
f=$(find "$RESULTS"/prof_$TAG -name "*kernel_stats.csv" | head -1)
python - "$f" "$TAG" <<'PY'
import csv, os, sys
f, tag = sys.argv[1], sys.argv[2]
rows = list(csv.DictReader(open(f)))
out = open(f"{os.environ['RESULTS']}/prof_{tag}.txt", "w")
out.write(f"{'calls':>6} {'total_us':>12} {'avg_us':>10} {'pct':>6}  name\n")
for r in rows[:45]:
    n = r["Name"].replace("(anonymous namespace)::", "")
    if len(n) > 100: n = n[:97] + "..."
    out.write(f"{int(r['Calls']):6d} {float(r['TotalDurationNs'])/1e3:12.1f} {float(r['AverageNs'])/1e3:10.1f} {float(r['Percentage']):6.2f}  {n}\n")
out.close()
print(open(f"{os.environ['RESULTS']}/prof_{tag}.txt").read())
PY
tail -1 "$RESULTS"/prof_$TAG.log

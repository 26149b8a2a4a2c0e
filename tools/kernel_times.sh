#!/bin/bash
# per-kernel average times of a bench run under rocprofv3 for a given library.  usage: tools/kernel_times.sh lib.so
# Output: $PROF_OUT/kst_<lib> (PROF_OUT: an absolute path, default prof_out/ in the repository).
L=$1
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${PROF_OUT:-$ROOT/prof_out}/kst_$L
cd /tmp && export TMPDIR=/tmp
TANGENCY_LIB=$ROOT/incorporating_different_sources_amd/$L rocprofv3 --kernel-trace --stats -f csv -d "$OUT" -- python3 "$ROOT/bench.py" --full --steps 20 --warmup 3 --no-cpu-baseline --no-end-to-end > /dev/null 2>&1
python3 - <<PY
import csv,glob
f=glob.glob("$OUT/**/*kernel_stats.csv", recursive=True)[0]
print("$L", [(r["Name"].split("::")[-1][:22], round(float(r["AverageNs"])/1e3,1)) for r in csv.DictReader(open(f))])
PY

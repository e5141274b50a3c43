#!/bin/bash
# usage: tools/pmc.sh <tag> "<counters>" <out dir> -- collects PMC counters for bench.py kernels (separate pass per call)
tag=$1; ctrs=$2; R=$(cd "$(dirname "$0")/.." && pwd); O=$(realpath -m "${3:?usage: tools/pmc.sh <tag> \"<counters>\" <out dir>}")/pmc_$tag; mkdir -p "${O%/*}"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --pmc $ctrs --output-format csv -d $O -- python3 $R/bench.py --full --no-cpu-baseline --no-extras --no-pmc --steps 3 --warmup 1 > $O.log 2>&1
python3 - <<PY
import csv, glob, collections
f = glob.glob("$O/*/*counter_collection.csv")
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for fn in f:
    for r in csv.DictReader(open(fn)):
        k = r["Kernel_Name"].split("(")[0][:40]
        acc[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, d in acc.items():
    print(k, {c: round(sum(v)/len(v), 1) for c, v in d.items()}, "n=", len(next(iter(d.values()))))
PY

"""Medians of a rocprofv3 --kernel-trace of host-landed headline steps (tools/host_lab/early_ab.py --steps-only): product rows /
fp64 SpMM / finish kernel durations, GPU span of a step (first kernel's start to the finish kernel's end) and GPU idle between
steps (finish kernel's end to the next step's first start), over steps 50 .. end, in us.
python tools/host_lab/trace_medians.py <dir with *_kernel_trace.csv> [label]"""
import csv, glob, sys
import numpy as np

f = sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True))[0]
rows = list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
steps, cur = [], None
for r in rows:
    name, s, e = r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    if "k_s1d_feature_rows" in name:
        cur = {"rows": (s, e)}
    elif cur is not None and "k_spmm_f64" in name:
        cur["spmm"] = (s, e)
    elif cur is not None and "k_delta_probe_finish" in name:
        cur["fin"] = (s, e)
        if len(cur) == 3:
            steps.append(cur)
        cur = None
steps = steps[50:]
d = lambda k: np.median([(s[k][1] - s[k][0]) / 1e3 for s in steps])
span = np.median([(s["fin"][1] - s["rows"][0]) / 1e3 for s in steps])
idle = np.median([(b["rows"][0] - a["fin"][1]) / 1e3 for a, b in zip(steps, steps[1:])])
print(f"{sys.argv[2] if len(sys.argv) > 2 else f}: {len(steps)} steps: {d('rows'):.1f} / {d('spmm'):.1f} / {d('fin'):.1f} / {span:.1f} / {idle:.1f}")

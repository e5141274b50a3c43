#!/usr/bin/env python3
"""The launch sequence of both GPU trainers, for comparing two builds of the library: two plain and two validated epochs
(keep_best) of one case per model -- train_cases B (several slices of dW1) and boundary_cases.train_case3 (hub rows: the segmented
launches), the cases "B" and "hub3" of tests/test_train_bits_gpu.py -- under rocprofv3, then one line per launch of the library (torch's own kernels and the runtime's copies are left out).

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/train_trace.py [--lib path/to/liblinkteller_hip.so]
    python tools/train_trace.py --reduce OUT listing.txt        # kernel, grid and block in threads, LDS bytes, in start order

Two listings are equal up to kernel names when two builds issue the same launches (profiles/train_core_trace_*.txt)."""
import csv
import glob
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def reduce(trace_dir, out):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {trace_dir}"
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows = sorted((r for r in rows if r["Kernel_Name"].replace("void ", "").startswith("k_")), key=lambda r: int(r["Start_Timestamp"]))
    with open(out, "w") as fh:
        for r in rows:
            name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "")
            grid, block = ([int(r[f"{k}_Size_{a}"]) for a in "XYZ"] for k in ("Grid", "Workgroup"))
            fh.write(f"{name}\tgrid={grid}\tblock={block}\tlds={r['LDS_Block_Size']}\n")
    print(out, len(rows), "launches")


def main():
    if "--lib" in sys.argv:
        from linkteller_amd import _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import numpy as np
    import torch
    import boundary_cases
    import train_cases as K
    from linkteller_amd import engine

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    for cls, case in ((engine.GCN2Trainer, K.make("B")), (engine.GCN3Trainer, boundary_cases.train_case3())):
        def trainer():
            return cls(case["adj"], dev(case["x"]), dev(case["y"]), *[dev(p.copy()) for p in case["params"]], lr=K.LR,
                       weight_decay=K.DECAY, dropout=case["p"], seed=K.SEED)
        trainer().run(2)
        tr = trainer()
        tr.attach_validation(case["adj"], dev(case["x"]), dev(case["y"]), keep_best=True, patience=0)
        tr.run_validated(2)
        torch.cuda.synchronize()


if __name__ == "__main__":
    if "--reduce" in sys.argv:
        reduce(*sys.argv[sys.argv.index("--reduce") + 1:][:2])
    else:
        main()

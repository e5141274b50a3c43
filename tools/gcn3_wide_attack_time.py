#!/usr/bin/env python3
"""ms per influence matrix of attacking a 3-layer GCN3 with a wide class layer (9 .. 256 classes), on the two synthetic graphs of
tools/train3_wide_time.py (ppi's shape with C = 121; the flickr-sized graph with F = 602, C = 41), H1 = 256, H2 = 64,
n_test = 500 random nodes, influence = 1e-4.

  primitive  Attacker.influence_matrix() in the default mode `delta`: engine.Baseline3 through lt_baseline3_create_wide, the
             rows widened and landed on the host (refresh of the fp64 baseline included, as every attack pays it)
  loop       the same nodes through Attacker._rows_generic (what a 9 .. 256-class GCN3 took before, and still takes for `sparse` /
             `full`) + the same landing.  The loop costs the same per probe whatever the probe, so it runs on the first
             --loop-probes (default 100) of the 500 probes against all 500 observed nodes and its time is scaled by
             500 / loop_probes; `loop_probes` is in the output.

Both are wall clock around work that ends in a device synchronise, in alternating blocks inside one process after one warm-up of
each; a block of the primitive is --prim-reps (default 20) matrices back to back, reported per matrix (one matrix is too short a
window), a block of the loop one pass; the figures are block medians with their min and max.  `gate` = the primitive's slowest block is faster than the loop's
fastest (scaled) block.  `probes_per_chunk` is read off lt_influence3_workspace_bytes (the level-2 tables of a wide handle are
sized by n rows per probe: a large graph gets small chunks).  `max_abs_diff_over_max` compares the two routes' rows on the loop's
probes (delta against the loop's fp32 finite difference: the reference's fp32 noise, not rounding).

Each shape runs in a child process of its own under a time limit; a child that fails ends the run (nothing is started behind it).

    python tools/gcn3_wide_attack_time.py [--shapes ppi reddit] [--blocks 5] [--out profiles/gcn3_wide_attack_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ("ppi", "reddit")
H1, H2, N_TEST, DELTA = 256, 64, 500, 1e-4


def child(name, blocks, loop_probes, prim_reps):
    import types

    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import train_wide_time as W2
    from linkteller_amd import _lib, engine, graph
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN3

    dev = torch.device("cuda:0")
    p = W2.problem(name, dev)
    n, nf, c = p["n"], p["nf"], p["c"]
    torch.manual_seed(4)
    model = GCN3(nf, H1, H2, c, 0.5).to(dev).eval()
    worker = types.SimpleNamespace(features=p["x"], adj_ori=p["adj_full"], n_nodes=n,
                                   adj_full=graph.sparse_mx_to_torch_sparse_tensor(p["adj_full"]).to(dev))
    args = argparse.Namespace(dataset=name, sample_type="unbalanced", n_test=N_TEST, sample_seed=42, influence=DELTA,
                              mode="vanilla-clean", attack_mode="efficient")
    atk = Attacker(args, model, worker)
    nodes = np.sort(np.random.RandomState(5).choice(n, N_TEST, replace=False)).astype(np.int64)
    atk.test_nodes = nodes
    assert atk._walk()[0] == "gcn3w" and atk._mode() == "delta"
    k = min(loop_probes, N_TEST)

    def primitive(reps=1):
        for _ in range(reps):
            out = atk.influence_matrix()
        return out

    def loop():
        return engine.export_rows_f64(atk._rows_generic(nodes[:k], nodes))

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    _, m_prim = wall(primitive)         # warm-up of both (code objects, the baseline's buffers, the workspace)
    _, m_loop = wall(loop)
    base = atk.baseline3()
    assert base.wide
    ws = [_lib.lib().lt_influence3_workspace_bytes(base._h, q, N_TEST) for q in range(N_TEST + 1)]
    chunk = max([q for q in range(1, N_TEST + 1) if ws[q] - ws[q - 1] > 4096] or [1])
    samples = {"primitive": [], "loop": []}
    for _ in range(blocks):
        samples["primitive"].append(wall(lambda: primitive(prim_reps))[0] / prim_reps)
        samples["loop"].append(wall(loop)[0] * N_TEST / k)
    row = {"shape": name, "n": n, "entries_per_row": p["entries_per_row"], "F": nf, "H1": H1, "H2": H2, "C": c, "n_test": N_TEST,
           "loop_probes": k, "prim_reps": prim_reps, "blocks": blocks, "probes_per_chunk": chunk, "chunks": -(-N_TEST // chunk),
           "workspace_mib": round(ws[N_TEST] / 2 ** 20, 1)}
    for key, v in samples.items():
        row[f"{key}_ms"] = round(float(np.median(v)), 3)
        row[f"{key}_min_ms"], row[f"{key}_max_ms"] = round(float(min(v)), 3), round(float(max(v)), 3)
        row[f"{key}_blocks_ms"] = [round(float(t), 3) for t in v]
    row["gate"] = bool(max(samples["primitive"]) < min(samples["loop"]))
    row["speedup"] = round(row["loop_ms"] / row["primitive_ms"], 2)
    row["max_abs_diff_over_max"] = float(np.abs(m_prim[:k] - m_loop).max() / m_loop.max())
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--loop-probes", type=int, default=100)
    ap.add_argument("--prim-reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape")
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.blocks, a.loop_probes, a.prim_reps)
    rows = []
    for name in a.shapes:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", name, "--blocks", str(a.blocks),
               "--loop-probes", str(a.loop_probes), "--prim-reps", str(a.prim_reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; nothing more is started", flush=True)
            return r.returncode
        rows += [json.loads(line[4:]) for line in r.stdout.splitlines() if line.startswith("ROW ")]
    if a.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"hidden1": H1, "hidden2": H2, "n_test": N_TEST, "influence": DELTA, "rows": rows}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

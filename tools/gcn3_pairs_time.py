#!/usr/bin/env python3
"""ms per scoring pass of `balanced-full` on a 3-layer GCN3: the pair list (lt_influence3_pairs) against the rectangle, on two
synthetic graphs (linkteller_amd/synth.py; nothing is read from a dataset):

  twitch   twitch-RU's shape (synth.twitch_like_problem: 4 385 nodes, 37 304 edges, F = 3170), the narrow GCN3 3170-256-64-2
  ppi      ppi's shape of tools/train_wide_time.py (14 755 nodes, 103 285 edges, F = 50), H1, H2 = 256, 64 and C = 121: the wide handle

What is timed is the scoring part of the attack (attacker.py:250-284): every edge plus as many non-edges
(sampling.construct_balanced_edge_sets, seed 82), from the first launch to the float64 scores of every pair on the host, mode
`delta`, influence = 1e-4; no sklearn, no file.

  pairs      Attacker.pair_scores: engine.group_pairs + ONE Baseline3.influence_pairs call + one copy of n_pairs floats
  rectangle  Attacker._balanced_scores_rect: 1024 starting nodes x every node through _rows per chunk, each block copied to the host,
             widened and read at the listed cells -- what `balanced-full` took for these models before the pair list, and still the
             fallback of the models without one

Both are wall clock around work that ends on the host (the scores are host arrays: the copy is the wait), in ALTERNATING blocks
inside one process after one warm-up pass of each, during which the two score arrays are asserted equal, value for value.  A block
is --reps passes (default 1 for the rectangle, 3 for the list: one rectangle pass is seconds), reported per pass; the figures are
block medians with their min, max and spread.  `gate` = the list's slowest block is faster than the rectangle's fastest.  Recorded
per route for ONE call: the workspace bytes (lt_influence3_pairs_workspace_bytes for the whole list; lt_influence3_workspace_bytes
for one 1024 x N chunk) and the bytes copied to the host (4 x n_pairs; 4 x 1024 x N per chunk, summed over the chunks of a pass).

Each shape runs in a child process of its own under a time limit; a child that fails ends the run (nothing is started behind it).

    python tools/gcn3_pairs_time.py [--shapes twitch ppi] [--blocks 5] [--out profiles/gcn3_pairs_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ("twitch", "ppi")
H1, H2, DELTA, CHUNK, SEED = 256, 64, 1e-4, 1024, 82


def problem(name, dev):
    """(raw adjacency, features on the device, classes)"""
    import torch
    from linkteller_amd import synth
    if name == "twitch":
        adj, x, _ = synth.twitch_like_problem("twitch-RU", hidden=H1, n_classes=2, seed=0)
        return adj, torch.from_numpy(x).to(dev), 2
    import train_wide_time as W2
    n, e, nf, c = W2.SHAPES["ppi"][:4]
    return synth.erdos_renyi_graph(n, e, seed=1), torch.from_numpy(synth.gaussian_features(n, nf, seed=2)).to(dev), c


def child(name, blocks, reps_pairs, reps_rect):
    import types

    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    from linkteller_amd import _lib, graph, sampling
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN3

    dev = torch.device("cuda:0")
    adj, x, c = problem(name, dev)
    n, nf = int(x.shape[0]), int(x.shape[1])
    torch.manual_seed(4)
    model = GCN3(nf, H1, H2, c, 0.5).to(dev).eval()
    worker = types.SimpleNamespace(features_2=x, adj_ori=adj, n_nodes=n,
                                   adj_2=graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(adj)).to(dev))
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="balanced-full", n_test=n, sample_seed=SEED, influence=DELTA,
                              mode="vanilla-clean", attack_mode="efficient", influence_mode="delta")
    atk = Attacker(args, model, worker)
    np.random.seed(SEED)
    (ex, nex), _ = sampling.construct_balanced_edge_sets("twitch/ES/RU", "balanced-full", adj, n)
    ex, nex = np.asarray(ex, dtype=np.int64).reshape(-1, 2), np.asarray(nex, dtype=np.int64).reshape(-1, 2)
    probe, observed = np.concatenate([ex[:, 0], nex[:, 0]]), np.concatenate([ex[:, 1], nex[:, 1]])
    kind = atk._walk()[0]
    assert kind == ("gcn3" if c <= 8 else "gcn3w") and atk._mode() == "delta" and atk._pair_route() is not None

    def pairs(reps=1):
        for _ in range(reps):
            out = atk.pair_scores(probe, observed)
        return out

    def rect(reps=1):
        for _ in range(reps):
            s_ex, s_nex = atk._balanced_scores_rect(ex, nex, np.empty(len(ex)), np.empty(len(nex)), CHUNK)
        return np.concatenate([s_ex, s_nex])

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    _, s_pairs = wall(pairs)            # warm-up of both (code objects, the baseline's buffers, the workspaces) ...
    _, s_rect = wall(rect)
    assert s_pairs.dtype == s_rect.dtype == np.float64 and np.array_equal(s_pairs, s_rect), np.abs(s_pairs - s_rect).max()
    assert s_pairs.max() > 0            # ... and the same scores, value for value
    samples = {"pairs": [], "rectangle": []}
    for _ in range(blocks):
        samples["pairs"].append(wall(lambda: pairs(reps_pairs))[0] / reps_pairs)
        samples["rectangle"].append(wall(lambda: rect(reps_rect))[0] / reps_rect)
    base = atk.baseline3()
    n_probe = int(len(np.union1d(ex[:, 0], nex[:, 0])))
    chunks = -(-n_probe // CHUNK)
    lib = _lib.lib()
    row = {"shape": name, "model": kind, "n": n, "edges": int(len(ex)), "F": nf, "H1": H1, "H2": H2, "C": c, "mode": "delta",
           "n_pairs": int(len(probe)), "n_probes": n_probe, "rectangle_chunk": CHUNK, "rectangle_chunks": chunks, "blocks": blocks,
           "reps_per_block": {"pairs": reps_pairs, "rectangle": reps_rect}, "scores_equal": True,
           "nonzero_share": round(float((s_pairs > 0).mean()), 3),
           "workspace_bytes": {"pairs": int(lib.lt_influence3_pairs_workspace_bytes(base._h, n_probe, len(probe))),
                               "rectangle": int(lib.lt_influence3_workspace_bytes(base._h, min(CHUNK, n_probe), n))},
           "bytes_to_host": {"pairs": 4 * int(len(probe)), "rectangle_per_chunk": 4 * min(CHUNK, n_probe) * n,
                             "rectangle_per_pass": 4 * n_probe * n}}
    for key, v in samples.items():
        row[f"{key}_ms"] = round(float(np.median(v)), 3)
        row[f"{key}_min_ms"], row[f"{key}_max_ms"] = round(float(min(v)), 3), round(float(max(v)), 3)
        row[f"{key}_spread_ms"] = round(float(max(v) - min(v)), 3)
        row[f"{key}_blocks_ms"] = [round(float(t), 3) for t in v]
    row["gate"] = bool(max(samples["pairs"]) < min(samples["rectangle"]))
    row["faster_in_every_block"] = bool(all(p < r for p, r in zip(samples["pairs"], samples["rectangle"])))
    row["speedup"] = round(row["rectangle_ms"] / row["pairs_ms"], 2)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps-pairs", type=int, default=3)
    ap.add_argument("--reps-rect", type=int, default=1)
    ap.add_argument("--limit", type=int, default=280, help="seconds per shape")
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.blocks, a.reps_pairs, a.reps_rect)
    rows = []
    for name in a.shapes:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", name, "--blocks", str(a.blocks),
               "--reps-pairs", str(a.reps_pairs), "--reps-rect", str(a.reps_rect)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; nothing more is started", flush=True)
            return r.returncode
        rows += [json.loads(line[4:]) for line in r.stdout.splitlines() if line.startswith("ROW ")]
    if a.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"hidden1": H1, "hidden2": H2, "influence": DELTA, "sample_seed": SEED, "rows": rows}, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

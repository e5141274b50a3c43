#!/usr/bin/env python3
"""ms per training epoch of the 3-layer GCN3 at twitch-ES shape (synthetic ER graph, N = 4648, E = 59 382, F = 3170, C = 2,
dropout 0.5): the HIP trainer (engine.GCN3Trainer) against stock torch on the same GPU doing the same epoch on a plain-torch
GCN3 of the same shapes (torch.sparse.mm, autograd, F.dropout, F.cross_entropy, foreach Adam).  After --warmup epochs of
each, --blocks blocks of --epochs epochs are timed with device events, HIP and torch alternating; the medians are reported,
beside the 2-layer ratios of profiles/train_time.json.

    python tools/train3_time.py [--widths 16x16 256x64] [--epochs 200] [--blocks 7] [--warmup 20] [--hip-only]
                                [--out profiles/train3_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from linkteller_amd import engine, graph, synth  # noqa: E402
from train3_cases import init_params  # noqa: E402  (the tests' init law: one RandomState, W1, b1, W2, b2, W3, b3)

N, E, NF, C = 4648, 59382, 3170, 2


def timed(fn, epochs):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn(epochs)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / epochs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", nargs="+", default=["16x16", "256x64"])
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    adj = graph.first_order_gcn(synth.erdos_renyi_graph(N, E, seed=1))
    x = torch.from_numpy(synth.twitch_like_features(N, NF, seed=2)).to(dev)
    y = torch.from_numpy(np.random.RandomState(3).randint(0, C, N)).to(dev)
    coo = adj.tocoo()
    a_t = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]), coo.data.astype(np.float32), adj.shape).coalesce().to(dev)
    rows = []
    for wd in a.widths:
        h1, h2 = (int(v) for v in wd.split("x"))
        init = init_params(NF, h1, h2, C, seed=4)
        tr = engine.GCN3Trainer(adj, x, y, *[torch.from_numpy(p).to(dev) for p in init], lr=0.01, weight_decay=5e-4,
                                dropout=0.5, seed=42)
        ps = [torch.from_numpy(p).to(dev).requires_grad_() for p in init]
        opt = torch.optim.Adam(ps, lr=0.01, weight_decay=5e-4, foreach=True)

        def torch_epochs(k):
            for _ in range(k):
                opt.zero_grad()
                h = F.dropout(torch.relu(torch.sparse.mm(a_t, x @ ps[0]) + ps[1]), 0.5, training=True)
                h = F.dropout(torch.relu(torch.sparse.mm(a_t, h @ ps[2]) + ps[3]), 0.5, training=True)
                loss = F.cross_entropy(torch.sparse.mm(a_t, h @ ps[4]) + ps[5], y)
                loss.backward()
                opt.step()

        tr.run_async(a.warmup)
        if not a.hip_only:
            torch_epochs(a.warmup)
        torch.cuda.synchronize()
        hip, ref = [], []
        for _ in range(a.blocks):
            hip.append(timed(tr.run_async, a.epochs))
            if not a.hip_only:
                ref.append(timed(torch_epochs, a.epochs))
        row = {"hidden1": h1, "hidden2": h2, "epochs": a.epochs, "blocks": a.blocks,
               "hip_ms_per_epoch": round(float(np.median(hip)), 4),
               "hip_ms_min_max": [round(min(hip), 4), round(max(hip), 4)]}
        if ref:
            row.update(torch_ms_per_epoch=round(float(np.median(ref)), 4),
                       torch_ms_min_max=[round(min(ref), 4), round(max(ref), 4)],
                       speedup=round(float(np.median(ref) / np.median(hip)), 2))
        print(json.dumps(row), flush=True)
        rows.append(row)
    two = {}
    try:
        with open(os.path.join(REPO, "profiles", "train_time.json")) as fh:
            two = {str(r["hidden"]): r.get("speedup") for r in json.load(fh)["rows"]}
    except OSError:
        pass
    print("2-layer speedups (profiles/train_time.json):", json.dumps(two), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"shape": {"N": N, "E": E, "F": NF, "C": C, "dropout": 0.5}, "rows": rows,
                       "two_layer_speedups": two}, fh, indent=1)


if __name__ == "__main__":
    main()

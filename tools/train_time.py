#!/usr/bin/env python3
"""ms per training epoch of the 2-layer GCN at twitch-ES shape (synthetic ER graph, N = 4648, E = 59 382, F = 3170, C = 2,
dropout 0.5): the HIP trainer (engine.GCN2Trainer) against stock torch on the same GPU doing the same epoch
(torch.sparse.mm, autograd, F.dropout, F.cross_entropy, foreach Adam).  Both are timed with device events over --epochs
epochs after --warmup epochs.

    python tools/train_time.py [--hidden 16 256] [--epochs 500] [--warmup 20] [--hip-only] [--out profiles/train_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linkteller_amd import engine, graph, synth  # noqa: E402

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
    ap.add_argument("--hidden", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--epochs", type=int, default=500)
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
    for h in a.hidden:
        w = synth.gcn_weights(NF, h, C, seed=4)
        params = [torch.from_numpy(w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")]
        tr = engine.GCN2Trainer(adj, x, y, *params, lr=0.01, weight_decay=5e-4, dropout=0.5, seed=42)
        tr.run_async(a.warmup)
        torch.cuda.synchronize()
        hip_ms = timed(tr.run_async, a.epochs)
        row = {"hidden": h, "epochs": a.epochs, "hip_ms_per_epoch": round(hip_ms, 4)}
        if not a.hip_only:
            ps = [torch.from_numpy(w[k]).to(dev).requires_grad_() for k in ("W1", "b1", "W2", "b2")]
            opt = torch.optim.Adam(ps, lr=0.01, weight_decay=5e-4, foreach=True)

            def torch_epochs(k):
                for _ in range(k):
                    opt.zero_grad()
                    hh = F.dropout(torch.relu(torch.sparse.mm(a_t, x @ ps[0]) + ps[1]), 0.5, training=True)
                    loss = F.cross_entropy(torch.sparse.mm(a_t, hh @ ps[2]) + ps[3], y)
                    loss.backward()
                    opt.step()

            torch_epochs(a.warmup)
            torch.cuda.synchronize()
            t_ms = timed(torch_epochs, a.epochs)
            row.update(torch_ms_per_epoch=round(t_ms, 4), speedup=round(t_ms / hip_ms, 2))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"shape": {"N": N, "E": E, "F": NF, "C": C, "dropout": 0.5}, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

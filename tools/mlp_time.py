#!/usr/bin/env python3
"""ms per training epoch of the feature-only MLP baselines: the HIP trainer (engine.MLPTrainer, a whole run enqueued by one
library call) against stock torch running the reference's loop in the same process (DataLoader(shuffle=True) over GPU tensors,
autograd, F.dropout, optim.Adam).  Shapes: twitch-ES training shape (n = 4648, F = 3170, C = 2 ce; depth 2 with H = 16 and 256,
and depth 1), ppi's training shape (n = 9716, F = 50, C = 121 bce, H = 256).  Batch 256, p = 0.5.  Each side is timed with device
events over --epochs epochs per block, in --blocks alternating blocks after --warmup epochs; the medians and min-max go to
--out, every block's figure with them.

    python tools/mlp_time.py [--epochs 20] [--blocks 5] [--warmup 3] [--out profiles/mlp_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, TensorDataset

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linkteller_amd import engine, synth  # noqa: E402

BATCH, P = 256, 0.5
SHAPES = [
    dict(name="twitch-ES depth 2 H=16", n=4648, f=3170, h=16, c=2, loss="ce"),
    dict(name="twitch-ES depth 2 H=256", n=4648, f=3170, h=256, c=2, loss="ce"),
    dict(name="twitch-ES depth 1", n=4648, f=3170, h=0, c=2, loss="ce"),
    dict(name="ppi depth 2 H=256", n=9716, f=50, h=256, c=121, loss="bce"),
]


def timed(fn, epochs):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn(epochs)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / epochs


def init(s, dev):
    rng = np.random.RandomState(4)
    dims = [s["f"], s["h"], s["c"]] if s["h"] else [s["f"], s["c"]]
    out = []
    for a, b in zip(dims[:-1], dims[1:]):
        k = 1.0 / np.sqrt(a)
        out += [rng.uniform(-k, k, (a, b)).astype(np.float32), rng.uniform(-k, k, b).astype(np.float32)]
    return [torch.from_numpy(p).to(dev) for p in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for s in SHAPES:
        n, f, h, c = s["n"], s["f"], s["h"], s["c"]
        if f == 3170:
            x = torch.from_numpy(synth.twitch_like_features(n, f, seed=2)).to(dev)
        else:
            x = torch.from_numpy(np.random.RandomState(2).standard_normal((n, f)).astype(np.float32)).to(dev)
        rng = np.random.RandomState(3)
        y = torch.from_numpy(rng.randint(0, 2, (n, c)) if s["loss"] == "bce" else rng.randint(0, c, n)).to(dev)
        depth = 2 if h else 1
        tr = engine.MLPTrainer(x, y, *init(s, dev), depth=depth, batch_size=BATCH, lr=0.01, weight_decay=5e-6, dropout=P, seed=42,
                               loss=s["loss"])
        ps = [p.clone().requires_grad_() for p in init(s, dev)]
        opt = torch.optim.Adam(ps, lr=0.01, weight_decay=5e-6)
        yt = y.float() if s["loss"] == "bce" else y
        loader = DataLoader(TensorDataset(x, yt), batch_size=BATCH, shuffle=True)

        def torch_epochs(k):
            for _ in range(k):
                for xb, yb in loader:
                    z = xb @ ps[0] + ps[1]
                    if depth == 2:
                        z = F.dropout(torch.relu(z), P, training=True) @ ps[2] + ps[3]
                    loss = F.binary_cross_entropy_with_logits(z, yb) if s["loss"] == "bce" else F.cross_entropy(z, yb)
                    opt.zero_grad()
                    loss.backward()
                    opt.step()

        tr.run_async(a.warmup)
        torch_epochs(a.warmup)
        torch.cuda.synchronize()
        hip, stock = [], []
        for _ in range(a.blocks):
            hip.append(timed(tr.run_async, a.epochs))
            stock.append(timed(torch_epochs, a.epochs))
        row = dict(shape=s["name"], n=n, F=f, H=h, C=c, loss=s["loss"], batch=BATCH, dropout=P, steps_per_epoch=tr.steps_per_epoch,
                   epochs_per_block=a.epochs, hip_ms_per_epoch=[round(v, 4) for v in hip],
                   torch_ms_per_epoch=[round(v, 4) for v in stock], hip_median=round(float(np.median(hip)), 4),
                   hip_min_max=[round(min(hip), 4), round(max(hip), 4)], torch_median=round(float(np.median(stock)), 4),
                   torch_min_max=[round(min(stock), 4), round(max(stock), 4)],
                   hip_faster_in_every_block=bool(all(u < v for u, v in zip(hip, stock))))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ms per epoch of training the 3-layer GCN3 with the wide head (engine.GCN3Trainer(head="wide")) on the synthetic graphs of
tools/train_wide_time.py (its ``ppi`` and ``reddit`` shapes, its split, features and labels), H1 = 256, H2 = 64, dropout 0.5.

The model trains on the induced training subgraph and is validated on the rows ``idx_val`` of the full graph.

  plain      run_async(k)                                             the training launches alone
  validated  run_validated(k, chunk = 10), keep_best, rows = idx_val  + forward on the full graph, the head over the list, state,
                                                                      snapshot; one state read per 10 epochs, wall clock
  torch      stock torch on the same GPU doing the same epoch (torch.sparse.mm, autograd, two F.dropout, the loss, foreach Adam)

The variants are timed in alternating blocks inside one process, each block --epochs epochs after --warmup warm-up epochs; the
figure is the median over --blocks blocks, ``spread`` the (max - min) / median of the plain blocks, and ``faster_in_every_block``
says whether the plain epoch beat torch's in each block (the blocks' values are kept).

    python tools/train3_wide_time.py [--shapes ppi reddit] [--epochs 50] [--blocks 5] [--out profiles/train3_wide_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/train3_wide_time.py --trace
        (--trace: 20 plain and 20 validated epochs per shape, no torch route: the per-kernel averages)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_wide_time as W2  # noqa: E402  (the shapes, the problem and the two clocks)
from linkteller_amd import engine  # noqa: E402

H1, H2, CHUNK = 256, 64, W2.CHUNK


def init_params(nf, c, seed=4):
    """The init law of gcn.GraphConvolution, U(-1 / sqrt(out), 1 / sqrt(out)), for the three layers."""
    rng = np.random.RandomState(seed)
    out = []
    for fan_in, fan_out in ((nf, H1), (H1, H2), (H2, c)):
        bound = 1.0 / np.sqrt(fan_out)
        out.append(rng.uniform(-bound, bound, (fan_in, fan_out)).astype(np.float32))
        out.append(rng.uniform(-bound, bound, fan_out).astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(W2.SHAPES))
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name in a.shapes:
        p = W2.problem(name, dev)
        c, loss = p["c"], p["loss"]
        g_train, g_full = engine.as_hip_graph(p["adj_train"]), engine.as_hip_graph(p["adj_full"])
        init = init_params(p["nf"], c)

        def make(validated):
            tr = engine.GCN3Trainer(g_train, p["x_train"], p["y_train"], *[torch.from_numpy(t.copy()).to(dev) for t in init], lr=0.01,
                                    weight_decay=5e-4, dropout=0.5, seed=42, head="wide", loss=loss)
            if validated:
                tr.attach_validation(g_full, p["x"], p["y"], rows=p["idx_val"], keep_best=True, patience=1 << 30)
            return tr
        plain, validated = make(False), make(True)
        if a.trace:
            plain.run_async(20)
            validated.run_validated(20, chunk=CHUNK)
            torch.cuda.synchronize()
            continue

        t_train = p["y_train"].float() if loss == "bce" else p["y_train"]
        loss_fn = F.binary_cross_entropy_with_logits if loss == "bce" else F.cross_entropy
        a_train = W2.sparse_tensor(p["adj_train"], dev)
        ps = [torch.from_numpy(t.copy()).to(dev).requires_grad_() for t in init]
        opt = torch.optim.Adam(ps, lr=0.01, weight_decay=5e-4, foreach=True)

        def torch_epochs(k):
            for _ in range(k):
                opt.zero_grad()
                h = F.dropout(torch.relu(torch.sparse.mm(a_train, p["x_train"] @ ps[0]) + ps[1]), 0.5, training=True)
                h = F.dropout(torch.relu(torch.sparse.mm(a_train, h @ ps[2]) + ps[3]), 0.5, training=True)
                loss_fn(torch.sparse.mm(a_train, h @ ps[4]) + ps[5], t_train).backward()
                opt.step()

        variants = {
            "plain": lambda: W2.event_ms(plain.run_async, a.epochs),
            "validated": lambda: W2.wall_ms(lambda k: validated.run_validated(k, chunk=CHUNK), a.epochs),
            "torch": lambda: W2.event_ms(torch_epochs, a.epochs),
        }
        plain.run_async(a.warmup)
        validated.run_validated(a.warmup, chunk=CHUNK)
        torch_epochs(a.warmup)
        torch.cuda.synchronize()
        samples = {k: [] for k in variants}
        for _ in range(a.blocks):
            for k, fn in variants.items():
                samples[k].append(fn())
        row = {"shape": name, "n_full": p["n"], "n_train": int(p["x_train"].shape[0]), "entries_per_row": p["entries_per_row"],
               "F": p["nf"], "H1": H1, "H2": H2, "C": c, "loss": loss, "rows_val": len(p["idx_val"]), "epochs": a.epochs,
               "blocks": a.blocks}
        for k, v in samples.items():
            row[f"{k}_ms"] = round(float(np.median(v)), 4)
            row[f"{k}_blocks_ms"] = [round(float(t), 4) for t in v]
        row["plain_spread"] = round(float((max(samples["plain"]) - min(samples["plain"])) / np.median(samples["plain"])), 4)
        row["faster_in_every_block"] = bool(all(x < t for x, t in zip(samples["plain"], samples["torch"])))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"hidden1": H1, "hidden2": H2, "dropout": 0.5, "chunk": CHUNK, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

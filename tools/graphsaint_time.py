#!/usr/bin/env python3
"""ms per epoch of training a dataset with one graph and a split of its nodes, at flickr's shape (synthetic ER graph, N = 89 250,
899 756 undirected edges, F = 500, C = 7, split 50 / 25 / 25, dropout 0.5): the 2-layer model with H = 256 and the 3-layer
model with 256 / 64.  The model trains on the induced training subgraph and is validated on the rows ``idx_val`` of the full
graph.

  plain      run_async(k)                                               the training launches alone
  validated  run_validated(k, chunk = 10), keep_best, rows = idx_val    + forward on the full graph, the head over the list, state,
                                                                        snapshot; one 32-byte state read per 10 epochs, wall clock
  host       the reference's way: run(1), then per epoch a synchronise, the eval-mode forward of the full graph through the
             library, F.cross_entropy(out[idx_val], ...) read back, and a deepcopy of the parameters when it improved

and the test-time head over ``idx_test`` of the full graph's logits:

  head_device   eval_head(logits, labels, rows = idx_test) + f1_from_confusion (one read of the 7 x 7 counts and the loss)
  head_host     softmax / argmax / cross_entropy on the gathered rows, the predictions read back, three sklearn f1_score calls

The variants are timed in alternating blocks inside one process, each block --epochs epochs (head: --head-reps calls); the
figure is the median over --blocks blocks and ``spread`` the (max - min) / median of the plain blocks.

    python tools/graphsaint_time.py [--epochs 50] [--blocks 5] [--out profiles/graphsaint_time.json]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linkteller_amd import engine, graph, synth  # noqa: E402

N, E, NF, C = 89250, 899756, 500, 7
CHUNK = 10


def event_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn(reps)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn(reps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--head-reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1)
    full = synth.erdos_renyi_graph(N, E, seed=1)
    perm = rng.permutation(N)
    idx_train, idx_val, idx_test = (np.sort(p) for p in (perm[:N // 2], perm[N // 2:3 * N // 4], perm[3 * N // 4:]))
    adj_full = graph.first_order_gcn(full)
    adj_train = graph.first_order_gcn(full[idx_train, :][:, idx_train])
    x = torch.from_numpy(synth.gaussian_features(N, NF, seed=2)).to(dev)
    y = torch.from_numpy(rng.randint(0, C, N)).to(dev)
    x_train, y_train = x[torch.from_numpy(idx_train).to(dev)].contiguous(), y[torch.from_numpy(idx_train).to(dev)]
    val_dev, test_dev = torch.from_numpy(idx_val).to(dev), torch.from_numpy(idx_test).to(dev)
    g_train, g_full = engine.as_hip_graph(adj_train), engine.as_hip_graph(adj_full)
    rows = []
    for family, hidden in (("gcn2", (256,)), ("gcn3", (256, 64))):
        def make(validated=False):
            w = synth.gcn_weights(NF, hidden[0], hidden[1] if family == "gcn3" else C, seed=4)
            params = [torch.from_numpy(w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")]
            if family == "gcn3":
                w3 = synth.gcn_weights(hidden[1], C, C, seed=8)
                params += [torch.from_numpy(w3["W1"]).to(dev), torch.from_numpy(w3["b1"]).to(dev)]
            cls = engine.GCN3Trainer if family == "gcn3" else engine.GCN2Trainer
            tr = cls(g_train, x_train, y_train, *params, lr=0.01, weight_decay=5e-4, dropout=0.5, seed=42)
            if validated:       # a patience no block exhausts: every block times all of its epochs, in chunks of CHUNK
                tr.attach_validation(g_full, x, y, keep_best=True, patience=1 << 30, rows=idx_val)
            return tr
        plain, validated, host = make(), make(True), make()

        def forward(tr):
            p = tr.params
            if family == "gcn2":
                return engine.gcn2_forward(g_full, x, *p)
            h1 = engine.spmm(g_full, engine.gemm(x, p[0]), p[1], relu=True)
            h2 = engine.spmm(g_full, engine.gemm(h1, p[2]), p[3], relu=True)
            return engine.spmm(g_full, engine.gemm(h2, p[4]), p[5])
        kept = {"loss": float("inf"), "model": None}

        def host_epochs(k):
            for _ in range(k):
                host.run(1)                                            # synchronises: the record is read
                out = forward(host)
                loss = float(torch.nn.functional.cross_entropy(out[val_dev], y[val_dev]))
                if not loss > kept["loss"]:
                    kept["loss"], kept["model"] = loss, copy.deepcopy([p.cpu() for p in host.params])
        logits = forward(plain)

        def head_device(k):
            for _ in range(k):
                loss, conf = engine.eval_head(logits, y, rows=test_dev)
                float(loss), engine.f1_from_confusion(conf)

        def head_host(k):
            from sklearn.metrics import f1_score
            for _ in range(k):
                out, target = logits[test_dev], y[test_dev]
                float(torch.nn.functional.cross_entropy(out, target))
                pred = torch.nn.functional.softmax(out, dim=1).max(1)[1].cpu()
                t = target.cpu()
                [f1_score(t, pred, average=kind) for kind in ("micro", "macro", "weighted")]
        host_k = max(a.epochs // 5, 1)
        variants = {
            "plain": lambda: event_ms(lambda k: plain.run_async(k), a.epochs),
            "validated": lambda: wall_ms(lambda k: validated.run_validated(k, chunk=CHUNK), a.epochs),
            "host": lambda: wall_ms(host_epochs, host_k),
            "head_device": lambda: wall_ms(head_device, a.head_reps),
            "head_host": lambda: wall_ms(head_host, a.head_reps),
        }
        plain.run_async(a.warmup)
        validated.run_validated(a.warmup, chunk=CHUNK)
        host_epochs(2)
        head_device(2)
        head_host(2)
        torch.cuda.synchronize()
        samples = {k: [] for k in variants}
        for _ in range(a.blocks):
            for name, fn in variants.items():
                samples[name].append(fn())
        row = {"family": family, "hidden": list(hidden), "epochs": a.epochs, "blocks": a.blocks, "head_reps": a.head_reps}
        for name, v in samples.items():
            unit = "ms_per_call" if name.startswith("head") else "ms_per_epoch"
            row[f"{name}_{unit}"] = round(float(np.median(v)), 4)
        row["plain_spread"] = round(float((max(samples["plain"]) - min(samples["plain"])) / np.median(samples["plain"])), 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"shape": {"N": N, "E": E, "F": NF, "C": C, "n_train": int(idx_train.size), "n_val": int(idx_val.size),
                                 "n_test": int(idx_test.size), "dropout": 0.5}, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

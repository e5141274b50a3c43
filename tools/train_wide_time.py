#!/usr/bin/env python3
"""ms per epoch of training with the wide head (engine.GCN2Trainer(head="wide")) on synthetic graphs, H = 256, dropout 0.5:

  ppi     ppi's training shape: 14 755 nodes with about 15 entries per row, split 9 716 / 1 825 / 3 214, F = 50, C = 121 labels
          per node, binary cross-entropy with logits
  reddit  reddit's class shape on a graph of the size tools/graphsaint_time.py gives flickr (N = 89 250, 899 756 undirected
          edges, split 50 / 25 / 25 -- NOT reddit's 232 965 nodes and 11.6 M edges): F = 602, C = 41, cross-entropy

The model trains on the induced training subgraph and is validated on the rows ``idx_val`` of the full graph.

  plain            run_async(k)                                             the training launches alone
  validated        run_validated(k, chunk = 10), keep_best, rows = idx_val  + forward on the full graph, the head over the list,
                                                                            state, snapshot; one state read per 10 epochs, wall clock
  torch            stock torch on the same GPU doing the same epoch (torch.sparse.mm, autograd, F.dropout, the loss, foreach Adam)
  torch_validated  the same, then per epoch the eval-mode forward of the full graph in torch, the loss over out[idx_val] read
                   back, and a deepcopy of the parameters when it improved; wall clock
  head_device      eval_head_wide(logits, labels, rows = idx_test) + f1_from_counts (one read of the [C, 3] counts and the loss)
  head_host        the reference's way: the loss on the gathered rows, the predictions read back, three sklearn f1_score calls

The variants are timed in alternating blocks inside one process, each block --epochs epochs (head: --head-reps calls); the
figure is the median over --blocks blocks and ``spread`` the (max - min) / median of the plain blocks.

    python tools/train_wide_time.py [--shapes ppi reddit] [--epochs 50] [--blocks 5] [--out profiles/train_wide_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/train_wide_time.py --trace
        (--trace: 20 plain and 20 validated epochs and 5 head calls per shape, no torch route: the per-kernel averages)
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linkteller_amd import engine, graph, synth  # noqa: E402

H, CHUNK = 256, 10
#            N, undirected edges, F, C, loss, (train, val, test)
SHAPES = {
    "ppi": (14755, 103285, 50, 121, "bce", (9716, 1825, 3214)),
    "reddit": (89250, 899756, 602, 41, "ce", (44625, 22312, 22313)),
}


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


def sparse_tensor(adj, dev):
    coo = adj.tocoo()
    return torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]), coo.data.astype(np.float32), adj.shape).coalesce().to(dev)


def problem(name, dev):
    n, e, nf, c, loss, split = SHAPES[name]
    rng = np.random.RandomState(11)
    raw = synth.erdos_renyi_graph(n, e, seed=1)
    perm = rng.permutation(n)
    idx_train = np.sort(perm[:split[0]])
    idx_val, idx_test = perm[split[0]:split[0] + split[1]], perm[split[0] + split[1]:]
    adj_full = graph.first_order_gcn(raw)
    adj_train = graph.first_order_gcn(sp.csr_matrix(raw)[idx_train][:, idx_train])
    x = torch.from_numpy(synth.gaussian_features(n, nf, seed=2)).to(dev)
    if loss == "bce":
        y = torch.from_numpy((rng.uniform(size=(n, c)) < 0.3).astype(np.int64)).to(dev)
    else:
        y = torch.from_numpy(rng.randint(0, c, n)).to(dev)
    tr_idx = torch.from_numpy(idx_train).to(dev)
    return dict(name=name, n=n, nf=nf, c=c, loss=loss, adj_full=adj_full, adj_train=adj_train, x=x, y=y, x_train=x[tr_idx].contiguous(),
                y_train=y[tr_idx].contiguous(), idx_val=idx_val, idx_test=idx_test, entries_per_row=round(adj_full.nnz / n, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--head-reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name in a.shapes:
        p = problem(name, dev)
        c, loss = p["c"], p["loss"]
        g_train, g_full = engine.as_hip_graph(p["adj_train"]), engine.as_hip_graph(p["adj_full"])
        w = synth.gcn_weights(p["nf"], H, c, seed=4)
        init = [w[k] for k in ("W1", "b1", "W2", "b2")]

        def make(validated):
            tr = engine.GCN2Trainer(g_train, p["x_train"], p["y_train"], *[torch.from_numpy(t.copy()).to(dev) for t in init], lr=0.01,
                                    weight_decay=5e-4, dropout=0.5, seed=42, head="wide", loss=loss)
            if validated:
                tr.attach_validation(g_full, p["x"], p["y"], rows=p["idx_val"], keep_best=True, patience=1 << 30)
            return tr
        plain, validated = make(False), make(True)
        val_dev, test_dev = torch.from_numpy(p["idx_val"]).to(dev), torch.from_numpy(p["idx_test"]).to(dev)
        t_train, t_full = (p["y_train"].float(), p["y"].float()) if loss == "bce" else (p["y_train"], p["y"])
        loss_fn = F.binary_cross_entropy_with_logits if loss == "bce" else F.cross_entropy

        def head_device(reps):
            for _ in range(reps):
                l, counts = engine.eval_head_wide(logits, p["y"], rows=test_dev, loss=loss)
                float(l)
                engine.f1_from_counts(counts, present_only=loss == "ce")

        def head_host(reps):
            from sklearn.metrics import f1_score
            for _ in range(reps):
                out, target = logits[test_dev], p["y"][test_dev]
                if loss == "bce":
                    F.binary_cross_entropy_with_logits(out, target.float()).item()
                    preds = torch.sigmoid(out) > 0.5
                else:
                    F.cross_entropy(out, target).item()
                    preds = out.max(1)[1]
                t, q = target.cpu(), preds.cpu()
                for k in ("micro", "macro", "weighted"):
                    f1_score(t, q, average=k, zero_division=0)

        if a.trace:
            plain.run_async(20)
            validated.run_validated(20, chunk=CHUNK)
            logits = validated.val_logits()
            head_device(5)
            torch.cuda.synchronize()
            continue

        a_train, a_full = sparse_tensor(p["adj_train"], dev), sparse_tensor(p["adj_full"], dev)
        ps = [torch.from_numpy(t.copy()).to(dev).requires_grad_() for t in init]
        opt = torch.optim.Adam(ps, lr=0.01, weight_decay=5e-4, foreach=True)
        kept = {"loss": float("inf"), "model": None}

        def torch_epoch():
            opt.zero_grad()
            h = F.dropout(torch.relu(torch.sparse.mm(a_train, p["x_train"] @ ps[0]) + ps[1]), 0.5, training=True)
            loss_fn(torch.sparse.mm(a_train, h @ ps[2]) + ps[3], t_train).backward()
            opt.step()

        def torch_epochs(k):
            for _ in range(k):
                torch_epoch()

        def torch_validated(k):
            for _ in range(k):
                torch_epoch()
                with torch.no_grad():
                    h = torch.relu(torch.sparse.mm(a_full, p["x"] @ ps[0]) + ps[1])
                    out = torch.sparse.mm(a_full, h @ ps[2]) + ps[3]
                    lv = float(loss_fn(out[val_dev], t_full[val_dev]))
                if not lv > kept["loss"]:
                    kept["loss"], kept["model"] = lv, copy.deepcopy([t.detach() for t in ps])

        variants = {
            "plain": lambda: event_ms(plain.run_async, a.epochs),
            "validated": lambda: wall_ms(lambda k: validated.run_validated(k, chunk=CHUNK), a.epochs),
            "torch": lambda: event_ms(torch_epochs, a.epochs),
            "torch_validated": lambda: wall_ms(torch_validated, a.epochs),
            "head_device": lambda: wall_ms(head_device, a.head_reps),
            "head_host": lambda: wall_ms(head_host, a.head_reps),
        }
        plain.run_async(a.warmup)
        validated.run_validated(a.warmup, chunk=CHUNK)
        torch_validated(a.warmup)
        logits = validated.val_logits()
        head_device(1)
        head_host(1)
        torch.cuda.synchronize()
        samples = {k: [] for k in variants}
        for _ in range(a.blocks):
            for k, fn in variants.items():
                samples[k].append(fn())
        row = {"shape": name, "n_full": p["n"], "n_train": int(p["x_train"].shape[0]), "entries_per_row": p["entries_per_row"],
               "F": p["nf"], "H": H, "C": c, "loss": loss, "rows_val": len(p["idx_val"]), "rows_test": len(p["idx_test"]),
               "epochs": a.epochs, "blocks": a.blocks}
        for k, v in samples.items():
            row[f"{k}_ms"] = round(float(np.median(v)), 4)
        row["plain_spread"] = round(float((max(samples["plain"]) - min(samples["plain"])) / np.median(samples["plain"])), 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"hidden": H, "dropout": 0.5, "chunk": CHUNK, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

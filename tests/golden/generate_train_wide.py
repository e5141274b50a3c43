#!/usr/bin/env python3
"""Generate ``train_wide.npz``: 40 training epochs of the REFERENCE's 2-layer GCN with a class layer wider than 8, in fp32 and
in fp64 -- one single-label case (9 classes, ``F.cross_entropy``) and one multi-label case (12 labels per node,
``F.binary_cross_entropy_with_logits``), the two losses of the reference's gcn_trainer.py:27-28, 41-45.

Runs only in the build container (needs the read-only reference tree); the ``.npz`` is committed.  As generate_train.py, it
follows ``train_one_epoch`` step by step with the reference's own ``gcn.models.GCN`` and ``optim.Adam(lr, weight_decay)``
(``gcn_trainer.py`` itself imports TensorBoard, which is not installed); the normalised adjacency is the reference's
``fetch_normalization`` + ``sparse_mx_to_torch_sparse_tensor``.  Dropout is 0 (torch's generator cannot be reproduced on the
GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_train_wide.py

The archive is written with fixed zip timestamps, so two runs give the same bytes.
"""
import copy
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn.functional as F
import torch.optim as optim

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import generate_train as G         # noqa: E402  (sets up the reference's path; quiet, save, normalised)
from generate_train import GCN, synth   # noqa: E402

N, E, NF, H = 300, 1200, 40, 16
EPOCHS, LR, DECAY, SEED, NORM = 40, 0.01, 5e-4, 42, "FirstOrderGCN"
CASES = {"ce9": ("ce", 9), "bce12": ("bce", 12)}
TINY = 1e-4          # an fp64 argmax margin (ce) or logit magnitude (bce) below this makes a prediction fragile


def counts(out, y, loss):
    """(tp summed over the classes, fragile predictions) of one epoch's train-mode logits."""
    out = out.detach()
    if loss == "ce":
        top2 = torch.topk(out, 2, dim=1).values
        return int((out.max(1)[1] == y).sum()), int(((top2[:, 0] - top2[:, 1]).abs() < TINY).sum())
    return int(((out > 0) & (y > 0.5)).sum()), int((out.abs() < TINY).sum())


def train(model, x, a, y, loss):
    opt = optim.Adam(model.parameters(), lr=LR, weight_decay=DECAY)
    fn = F.cross_entropy if loss == "ce" else F.binary_cross_entropy_with_logits
    losses, tps, tiny = [], [], []
    for _ in range(EPOCHS):
        model.train()
        opt.zero_grad()
        out = model(x, a)
        lt = fn(out, y)
        losses.append(lt.item())
        tp, fragile = counts(out, y, loss)
        tps.append(tp)
        tiny.append(fragile)
        lt.backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        logits = model(x, a)
    return np.array(losses), np.array(tps), np.array(tiny), logits.numpy()


def main():
    adj = synth.erdos_renyi_graph(N, E, seed=21)
    x = synth.gaussian_features(N, NF, seed=22)
    t, m = G.normalised(adj, NORM)
    out = dict(x=x, epochs=np.int64(EPOCHS), lr=np.float64(LR), decay=np.float64(DECAY), tiny=np.float64(TINY))
    out["adj.indptr"], out["adj.indices"] = m.indptr.astype(np.int64), m.indices.astype(np.int64)
    out["adj.data"] = m.data.astype(np.float32)
    X = torch.from_numpy(x)
    rng = np.random.RandomState(23)
    for key, (loss, c) in CASES.items():
        centres = rng.standard_normal((NF, c)).astype(np.float32)
        score = x @ centres
        y = score.argmax(axis=1).astype(np.int64) if loss == "ce" else (score > np.quantile(score, 0.7)).astype(np.uint8)
        out[f"{key}.y"] = y
        torch.manual_seed(SEED)
        model = G.quiet(GCN, nfeat=NF, nhid=H, nclass=c, dropout=0.0)
        model64 = copy.deepcopy(model).double()
        for name, p in model.state_dict().items():
            out[f"{key}.init.{name}"] = p.numpy().copy()
        y32 = torch.from_numpy(y) if loss == "ce" else torch.from_numpy(y).float()
        y64 = y32 if loss == "ce" else y32.double()
        l32, tp32, _, z32 = train(model, X, t, y32, loss)
        l64, tp64, tiny64, z64 = train(model64, X.double(), t.double(), y64, loss)
        out.update({f"{key}.loss32": l32, f"{key}.loss64": l64, f"{key}.tp32": tp32, f"{key}.tp64": tp64, f"{key}.tiny64": tiny64,
                    f"{key}.logits32": z32, f"{key}.logits64": z64})
        print(f"{key}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, tp {tp64[0]} -> {tp64[-1]}, |loss32 - loss64| max "
              f"{np.abs(l32 - l64).max():.2e}, fragile {int(tiny64.max())}")
    G.save("train_wide.npz", out)


if __name__ == "__main__":
    main()

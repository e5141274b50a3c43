#!/usr/bin/env python3
"""Generate ``mlp_train.npz``: minibatch training of the REFERENCE's feature-only baselines, in fp32 and in fp64.

Runs only in the build container (needs the read-only reference tree); the ``.npz`` is committed.  The reference's
``mlp_trainer.py`` imports TensorBoard, which is not installed, so its ``train_one_epoch`` (mlp_trainer.py:97-122, the
``--batch`` branch) is followed step by step with the reference's own ``gcn.models.OneLayerMLP`` / ``SingleHiddenLayerMLP``,
``F.cross_entropy`` / ``F.binary_cross_entropy_with_logits`` and ``optim.Adam(lr, weight_decay)``.  Dropout is 0 (torch's
generator cannot be reproduced on the GPU); each epoch's row order is recorded in the archive instead of being drawn by a
``DataLoader``, and the batches are its consecutive stretches of 64 rows (the last one 44: ``drop_last=False``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_mlp_train.py

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

from generate_train import REF, quiet, save  # noqa: E402,F401  (puts the repository and the reference on sys.path)

from linkteller_amd import synth  # noqa: E402

from gcn.models import OneLayerMLP, SingleHiddenLayerMLP  # noqa: E402  reference models

torch.set_num_threads(1)

N, NF, BATCH = 300, 160, 64
EPOCHS, LR, DECAY, SEED = 5, 0.01, 5e-4, 42
TINY = 1e-4          # an fp64 margin below this makes a row's (an element's) prediction fragile
# key: (depth, hidden, classes, loss)
CASES = {"d2.h16": (2, 16, 2, "ce"), "d2.h64": (2, 64, 2, "ce"), "d2.h16.ml5": (2, 16, 5, "bce"), "d1": (1, 0, 2, "ce")}


def train(model, x, y, orders, loss_kind):
    """mlp_trainer.py:104-113 over the recorded orders: per-step loss, tp count and the count of fragile predictions."""
    opt = optim.Adam(model.parameters(), lr=LR, weight_decay=DECAY)
    loss, count, tiny = [], [], []
    model.train()
    for order in orders:
        for o in range(0, N, BATCH):
            rows = torch.from_numpy(order[o:o + BATCH])
            out = model(x[rows])
            if loss_kind == "ce":
                lt = F.cross_entropy(out, y[rows])
                count.append(int((out.max(1)[1] == y[rows]).sum()))
                top2 = torch.topk(out.detach(), 2, dim=1).values
                tiny.append(int(((top2[:, 0] - top2[:, 1]).abs() < TINY).sum()))
            else:
                lt = F.binary_cross_entropy_with_logits(out, y[rows].to(out.dtype))
                count.append(int(((out > 0) & (y[rows] != 0)).sum()))
                tiny.append(int(((out.detach().abs() < TINY) & (y[rows] != 0)).sum()))
            loss.append(lt.item())
            opt.zero_grad()
            lt.backward()
            opt.step()
    return np.array(loss), np.array(count), np.array(tiny)


def main():
    x = synth.twitch_like_features(N, NF, seed=13, density=0.05)
    rng = np.random.RandomState(15)
    r = rng.standard_normal(NF).astype(np.float32)
    y2 = (x @ r > np.median(x @ r)).astype(np.int64)
    r5 = rng.standard_normal((NF, 5)).astype(np.float32)
    y5 = (x @ r5 > np.median(x @ r5, axis=0)).astype(np.uint8)
    orders = np.stack([np.random.RandomState(100 + e).permutation(N) for e in range(EPOCHS)]).astype(np.int64)
    out = dict(x=x, y2=y2, y5=y5, orders=orders, batch=np.int64(BATCH), lr=np.float64(LR), decay=np.float64(DECAY),
               tiny=np.float64(TINY))
    X = torch.from_numpy(x)
    for key, (depth, h, c, loss_kind) in CASES.items():
        torch.manual_seed(SEED)
        model = quiet(OneLayerMLP, nfeat=NF, nclass=c) if depth == 1 else \
            quiet(SingleHiddenLayerMLP, nfeat=NF, nhid=h, nclass=c, dropout=0.0)
        model64 = copy.deepcopy(model).double()
        y = torch.from_numpy(y2 if loss_kind == "ce" else y5)
        for name, p in model.state_dict().items():
            out[f"{key}.init.{name}"] = p.numpy().copy()
        l32, c32, _ = train(model, X, y, orders, loss_kind)
        l64, c64, tiny64 = train(model64, X.double(), y, orders, loss_kind)
        for name, p in model.state_dict().items():
            out[f"{key}.final32.{name}"] = p.numpy().copy()
        for name, p in model64.state_dict().items():
            out[f"{key}.final64.{name}"] = p.numpy().copy()
        out.update({f"{key}.loss32": l32, f"{key}.loss64": l64, f"{key}.count32": c32, f"{key}.count64": c64,
                    f"{key}.tiny64": tiny64})
        print(f"{key}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, |loss32 - loss64| max {np.abs(l32 - l64).max():.2e}")
    save("mlp_train.npz", out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate ``validate.npz``: 40 epochs of the REFERENCE's GCN and GCN3 with the validation of every epoch, in fp32 and fp64.

Runs only in the build container (needs the read-only reference tree); the ``.npz`` is committed.  Graphs, features, labels
and initial weights are those of ``train.npz`` / ``train3.npz`` and are read from there, not stored again.  As in
generate_train.py the reference's ``train_one_epoch`` on a transfer dataset is followed step by step; after each optimiser
step the model is switched to eval mode, forwarded on the held-out graph and ``loss_val`` / the predictions are taken
(gcn_trainer.py:167-174), and the loss goes to the reference's own ``utils.early_stopping.EarlyStopping`` (as
gcn_trainer.py:195-196 does), one instance per patience.  An instance is not called again once it has stopped
(gcn_trainer.py:235-238 breaks out of the loop there); the 40 epochs run on, so one training serves both patiences.

Per row ``<norm>.h<H>`` (GCN) / ``<norm>.h<H1>_<H2>`` (GCN3):
  loss_val64, loss_val32 [40]      the validation loss after each epoch's update
  counts64, counts32 [40, C, C]    confusion counts (true class, predicted class) of the same forward
  tiny_val64 [40]                  held-out rows whose fp64 logit margin is below ``tiny`` (their argmax is fragile)
  p3, p10 [2]                      (best epoch, stop epoch), 0-based, of EarlyStopping(patience) on loss_val64; the fp32 run
                                   is asserted to give the same pairs
  best64.e<epoch>.<name>, best32.e<epoch>.<name>    the state_dict of ``EarlyStopping.best_model`` (stored once per epoch)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_validate.py

``EarlyStopping.__init__`` reads ``np.Inf``, which numpy 2 no longer has: the name is put back before the class is used.
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

import generate_train as G                              # noqa: E402  (puts the repository and the reference on sys.path)
import generate_train3 as G3                            # noqa: E402
from gcn.models import GCN, GCN3                        # noqa: E402  reference models
if not hasattr(np, "Inf"):
    np.Inf = np.inf
from utils.early_stopping import EarlyStopping          # noqa: E402  reference helper

torch.set_num_threads(1)

PATIENCES = (3, 10)
# the table of the pull request that introduced this fixture: row -> ((best, stop) for patience 3, for patience 10)
EXPECTED = {
    "FirstOrderGCN.h16": ((17, 20), (17, 27)), "FirstOrderGCN.h64": ((3, 6), (3, 13)),
    "AugRWalk.h16": ((15, 18), (15, 25)), "AugRWalk.h64": ((5, 8), (5, 15)),
    "FirstOrderGCN.h16_16": ((3, 6), (14, 24)), "FirstOrderGCN.h64_32": ((7, 10), (12, 22)),
    "AugRWalk.h16_16": ((4, 7), (12, 22)), "AugRWalk.h64_32": ((7, 10), (7, 17)),
}


def confusion(out, y, c):
    pred = out.max(1)[1]
    return np.bincount((y * c + pred).numpy(), minlength=c * c).reshape(c, c).astype(np.int64)


def train_validated(model, x1, a1, y1, x2, a2, y2, c):
    opt = optim.Adam(model.parameters(), lr=G.LR, weight_decay=G.DECAY)
    stoppers = {p: EarlyStopping(patience=p) for p in PATIENCES}
    best = {p: -1 for p in PATIENCES}
    stop = {p: -1 for p in PATIENCES}
    kept = {}
    loss_val, counts, tiny = [], [], []
    for epoch in range(G.EPOCHS):
        model.train()
        opt.zero_grad()
        F.cross_entropy(model(x1, a1), y1).backward()
        opt.step()
        model.eval()
        with torch.no_grad():
            out = model(x2, a2)
            lv = F.cross_entropy(out, y2)
        loss_val.append(lv.item())
        counts.append(confusion(out, y2, c))
        top2 = torch.topk(out, 2, dim=1).values
        tiny.append(int(((top2[:, 0] - top2[:, 1]).abs() < G.TINY).sum()))
        for p, es in stoppers.items():
            if stop[p] >= 0:
                continue
            before = es.best_model
            es(lv, model)
            if es.best_model is not before:
                best[p] = epoch
            if es.early_stop:
                stop[p] = epoch
    for p, es in stoppers.items():
        kept[best[p]] = {k: v.numpy().copy() for k, v in es.best_model.state_dict().items()}
    return np.array(loss_val), np.stack(counts), np.array(tiny), {p: (best[p], stop[p]) for p in PATIENCES}, kept


def main():
    g, g3 = np.load(os.path.join(HERE, "train.npz")), np.load(os.path.join(HERE, "train3.npz"))
    x1, x2, y1, y2 = g["x1"], g["x2"], g["y1"], g["y2"]
    nf, c = x1.shape[1], int(y1.max()) + 1
    X1, X2, Y1, Y2 = (torch.from_numpy(a) for a in (x1, x2, y1, y2))
    out = dict(epochs=np.int64(G.EPOCHS), lr=np.float64(G.LR), decay=np.float64(G.DECAY), tiny=np.float64(G.TINY),
               patiences=np.array(PATIENCES, dtype=np.int64))
    rows, wrong = [], []
    for norm in G.NORMS:
        t1, t2 = G3.stored(g, norm, "adj1")[0], G3.stored(g, norm, "adj2")[0]
        cases = [(f"{norm}.h{h}", g, lambda h=h: G.quiet(GCN, nfeat=nf, nhid=h, nclass=c, dropout=0.0)) for h in G.HIDDEN]
        cases += [(f"{norm}.h{h1}_{h2}", g3, lambda h1=h1, h2=h2: G.quiet(GCN3, nfeat=nf, nhid1=h1, nhid2=h2, nclass=c,
                                                                        dropout=0.0)) for h1, h2 in G3.WIDTHS]
        for key, src, make in cases:
            model = make()
            model.load_state_dict({k: torch.from_numpy(src[f"{key}.init.{k}"].copy()) for k in model.state_dict()})
            model64 = copy.deepcopy(model).double()
            l32, c32, _, d32, kept32 = train_validated(model, X1, t1, Y1, X2, t2, Y2, c)
            l64, c64, tiny64, d64, kept64 = train_validated(model64, X1.double(), t1.double(), Y1, X2.double(), t2.double(), Y2, c)
            assert d32 == d64, (key, d32, d64)
            out.update({f"{key}.loss_val64": l64, f"{key}.loss_val32": l32, f"{key}.counts64": c64, f"{key}.counts32": c32,
                        f"{key}.tiny_val64": tiny64})
            for p in PATIENCES:
                out[f"{key}.p{p}"] = np.array(d64[p], dtype=np.int64)
            for tag, kept in (("best64", kept64), ("best32", kept32)):
                for e, sd in kept.items():
                    for name, a in sd.items():
                        out[f"{key}.{tag}.e{e}.{name}"] = a
            rows.append(key)
            got = tuple(d64[p] for p in PATIENCES)
            if got != EXPECTED[key]:
                wrong.append((key, got, EXPECTED[key]))
            last = max(s for _, s in got)
            gap = np.abs(np.diff(l64[:last + 1])).min()
            print(f"{key}: (best, stop) {got}, loss_val {l64[0]:.4f} -> min {l64.min():.4f}, smallest gap up to the stop "
                  f"{gap:.2e}, |32 - 64| max {np.abs(l32 - l64).max():.2e}")
    out["rows"] = np.array(rows)
    G.save("validate.npz", out)
    assert not wrong, f"the issue's table is wrong in these rows (row, generated, table): {wrong}"


if __name__ == "__main__":
    main()

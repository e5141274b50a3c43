#!/usr/bin/env python3
"""Generate ``train3.npz``: 40 training epochs of the REFERENCE's 3-layer GCN3, in fp32 and in fp64.

Runs only in the build container (needs the read-only reference tree); the ``.npz`` is committed.  The graphs, features and
labels are those of ``train.npz`` and are read from it, not stored again; the stored normalised adjacencies are checked
against the reference's ``fetch_normalization`` on the same synthetic graphs.  As in generate_train.py, ``train_one_epoch``
on a transfer dataset (gcn_trainer.py:144-170) is followed step by step with the reference's own ``gcn.models.GCN3``,
``F.cross_entropy`` and ``optim.Adam(lr, weight_decay)``.  Dropout is 0 (torch's generator cannot be reproduced on the GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_train3.py

The archive is written with fixed zip timestamps, so two runs give the same bytes.
"""
import copy
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import generate_train as G         # noqa: E402  (puts the repository and the reference on sys.path)
from gcn.models import GCN3        # noqa: E402  reference model

from linkteller_amd import synth   # noqa: E402

torch.set_num_threads(1)

WIDTHS = ((16, 16), (64, 32))


def stored(g, norm, tag):
    n = g[f"{norm}.{tag}.indptr"].shape[0] - 1
    m = sp.csr_matrix((g[f"{norm}.{tag}.data"], g[f"{norm}.{tag}.indices"], g[f"{norm}.{tag}.indptr"]), shape=(n, n))
    coo = m.tocoo()
    t = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]), coo.data, m.shape).coalesce()
    return t, m


def main():
    g = np.load(os.path.join(HERE, "train.npz"))
    x1, x2, y1 = g["x1"], g["x2"], g["y1"]
    nf, c = x1.shape[1], int(y1.max()) + 1
    assert int(g["epochs"]) == G.EPOCHS and float(g["lr"]) == G.LR and float(g["decay"]) == G.DECAY
    X1, X2, Y1 = torch.from_numpy(x1), torch.from_numpy(x2), torch.from_numpy(y1)
    raw = {"adj1": synth.erdos_renyi_graph(G.N1, G.E1, seed=11), "adj2": synth.erdos_renyi_graph(G.N2, G.E2, seed=12)}
    out = dict(epochs=np.int64(G.EPOCHS), lr=np.float64(G.LR), decay=np.float64(G.DECAY), tiny=np.float64(G.TINY))
    for norm in G.NORMS:
        ts = {}
        for tag in ("adj1", "adj2"):
            ts[tag], m = stored(g, norm, tag)
            _, ref = G.normalised(raw[tag], norm)       # the reference's normaliser gives the stored matrix
            assert (m != ref).nnz == 0 and np.array_equal(m.data, ref.data), (norm, tag)
        for h1, h2 in WIDTHS:
            key = f"{norm}.h{h1}_{h2}"
            torch.manual_seed(G.SEED)
            model = G.quiet(GCN3, nfeat=nf, nhid1=h1, nhid2=h2, nclass=c, dropout=0.0)
            model64 = copy.deepcopy(model).double()
            for name, p in model.state_dict().items():
                out[f"{key}.init.{name}"] = p.numpy().copy()
            l32, _, _, z32 = G.train(model, X1, ts["adj1"], Y1, X2, ts["adj2"])
            l64, c64, tiny64, z64 = G.train(model64, X1.double(), ts["adj1"].double(), Y1, X2.double(), ts["adj2"].double())
            out.update({f"{key}.loss32": l32, f"{key}.loss64": l64, f"{key}.correct64": c64, f"{key}.tiny64": tiny64,
                        f"{key}.logits2_32": z32, f"{key}.logits2_64": z64})
            print(f"{key}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, acc {c64[-1] / x1.shape[0]:.3f}, "
                  f"|loss32 - loss64| max {np.abs(l32 - l64).max():.2e}")
    G.save("train3.npz", out)


if __name__ == "__main__":
    main()

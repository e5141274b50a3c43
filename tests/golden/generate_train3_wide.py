#!/usr/bin/env python3
"""Generate ``train3_wide.npz``: 40 training epochs of the REFERENCE's 3-layer GCN3 with a class layer wider than 8, in fp32
and in fp64 -- one single-label case (9 classes, ``F.cross_entropy``) and one multi-label case (12 labels per node,
``F.binary_cross_entropy_with_logits``), the two losses of the reference's gcn_trainer.py:27-28, 41-45 on the model it builds
for ``--n-layer 3`` (gcn_trainer.py:81-86).

Runs only in the build container (needs the read-only reference tree); the ``.npz`` is committed.  As generate_train_wide.py,
whose graph, features, labels and epoch loop it shares, it follows ``train_one_epoch`` step by step with the reference's own
``gcn.models.GCN3`` and ``optim.Adam(lr, weight_decay)``.  Dropout is 0 (torch's generator cannot be reproduced on the GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_train3_wide.py

The archive is written with fixed zip timestamps, so two runs give the same bytes.
"""
import copy
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import generate_train as G            # noqa: E402  (sets up the reference's path; quiet, save, normalised)
import generate_train_wide as GW      # noqa: E402  (sizes, cases, the epoch loop)
from generate_train import synth      # noqa: E402
from gcn.models import GCN3           # noqa: E402  reference model

H1, H2 = 16, 12


def main():
    adj = synth.erdos_renyi_graph(GW.N, GW.E, seed=21)
    x = synth.gaussian_features(GW.N, GW.NF, seed=22)
    t, m = G.normalised(adj, GW.NORM)
    out = dict(x=x, epochs=np.int64(GW.EPOCHS), lr=np.float64(GW.LR), decay=np.float64(GW.DECAY), tiny=np.float64(GW.TINY))
    out["adj.indptr"], out["adj.indices"] = m.indptr.astype(np.int64), m.indices.astype(np.int64)
    out["adj.data"] = m.data.astype(np.float32)
    X = torch.from_numpy(x)
    rng = np.random.RandomState(23)
    for key, (loss, c) in GW.CASES.items():
        centres = rng.standard_normal((GW.NF, c)).astype(np.float32)
        score = x @ centres
        y = score.argmax(axis=1).astype(np.int64) if loss == "ce" else (score > np.quantile(score, 0.7)).astype(np.uint8)
        out[f"{key}.y"] = y
        torch.manual_seed(GW.SEED)
        model = G.quiet(GCN3, nfeat=GW.NF, nhid1=H1, nhid2=H2, nclass=c, dropout=0.0)
        model64 = copy.deepcopy(model).double()
        for name, p in model.state_dict().items():
            out[f"{key}.init.{name}"] = p.numpy().copy()
        y32 = torch.from_numpy(y) if loss == "ce" else torch.from_numpy(y).float()
        y64 = y32 if loss == "ce" else y32.double()
        l32, tp32, _, z32 = GW.train(model, X, t, y32, loss)
        l64, tp64, tiny64, z64 = GW.train(model64, X.double(), t.double(), y64, loss)
        out.update({f"{key}.loss32": l32, f"{key}.loss64": l64, f"{key}.tp32": tp32, f"{key}.tp64": tp64, f"{key}.tiny64": tiny64,
                    f"{key}.logits32": z32, f"{key}.logits64": z64})
        print(f"{key}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, tp {tp64[0]} -> {tp64[-1]}, |loss32 - loss64| max "
              f"{np.abs(l32 - l64).max():.2e}, fragile {int(tiny64.max())}")
    G.save("train3_wide.npz", out)


if __name__ == "__main__":
    main()

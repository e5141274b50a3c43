#!/usr/bin/env python3
"""Generate ``train.npz``: 40 training epochs of the REFERENCE's 2-layer GCN, in fp32 and in fp64.

Runs only in the build container (needs the read-only reference tree); the ``.npz`` is committed.  The reference's
``gcn_trainer.py`` imports TensorBoard, which is not installed, so ``train_one_epoch`` on a transfer dataset
(gcn_trainer.py:144-170) is followed step by step with the reference's own ``gcn.models.GCN``, ``F.cross_entropy`` and
``optim.Adam(lr, weight_decay)``; the normalised adjacency is the reference's ``fetch_normalization`` +
``sparse_mx_to_torch_sparse_tensor``.  Dropout is 0 (torch's generator cannot be reproduced on the GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_train.py

The archive is written with fixed zip timestamps, so two runs give the same bytes.
"""
import contextlib
import copy
import io
import os
import sys
import zipfile

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F
import torch.optim as optim

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("LT_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

from linkteller_amd import synth  # noqa: E402

import utils as ref_utils          # noqa: E402  reference utils (normalisation, sparse conversion)
from gcn.models import GCN         # noqa: E402  reference model

torch.set_num_threads(1)

N1, N2, E1, E2, NF, C = 300, 250, 1200, 1000, 160, 2
EPOCHS, LR, DECAY, SEED = 40, 0.01, 5e-4, 42
NORMS = ("FirstOrderGCN", "AugRWalk")
HIDDEN = (16, 64)
TINY = 1e-4          # an fp64 logit margin below this makes a row's argmax fragile


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*a, **k)


def save(name, arrays):
    """np.savez_compressed with fixed member timestamps (byte-stable)."""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[key])
            np.lib.format.write_array(buf, a if a.ndim == 0 else np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print(f"wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB")


def normalised(adj, norm):
    t = quiet(ref_utils.sparse_mx_to_torch_sparse_tensor, ref_utils.fetch_normalization(norm)(adj)).coalesce()
    idx = t.indices().numpy()
    m = sp.csr_matrix((t.values().numpy(), (idx[0], idx[1])), shape=tuple(t.shape))
    m.sort_indices()
    return t, m


def train(model, x1, a1, y1, x2, a2):
    """gcn_trainer.py:144-170 (transfer branch) for EPOCHS epochs, then the eval-mode logits on graph 2."""
    opt = optim.Adam(model.parameters(), lr=LR, weight_decay=DECAY)
    loss, correct, tiny = [], [], []
    for _ in range(EPOCHS):
        model.train()
        opt.zero_grad()
        out = model(x1, a1)
        lt = F.cross_entropy(out, y1)
        loss.append(lt.item())
        correct.append(int((out.max(1)[1] == y1).sum()))
        top2 = torch.topk(out.detach(), 2, dim=1).values
        tiny.append(int(((top2[:, 0] - top2[:, 1]).abs() < TINY).sum()))
        lt.backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        logits2 = model(x2, a2)
    return np.array(loss), np.array(correct), np.array(tiny), logits2.numpy()


def main():
    adj1 = synth.erdos_renyi_graph(N1, E1, seed=11)
    adj2 = synth.erdos_renyi_graph(N2, E2, seed=12)
    x1 = synth.twitch_like_features(N1, NF, seed=13, density=0.05)
    x2 = synth.twitch_like_features(N2, NF, seed=14, density=0.05)
    rng = np.random.RandomState(15)
    r = rng.standard_normal(NF).astype(np.float32)
    y1 = (x1 @ r > np.median(x1 @ r)).astype(np.int64)
    y2 = (x2 @ r > np.median(x2 @ r)).astype(np.int64)
    out = dict(x1=x1, x2=x2, y1=y1, y2=y2, epochs=np.int64(EPOCHS), lr=np.float64(LR), decay=np.float64(DECAY),
               tiny=np.float64(TINY))
    X1, X2, Y1 = torch.from_numpy(x1), torch.from_numpy(x2), torch.from_numpy(y1)
    for norm in NORMS:
        t1, m1 = normalised(adj1, norm)
        t2, m2 = normalised(adj2, norm)
        for tag, m in (("adj1", m1), ("adj2", m2)):
            out[f"{norm}.{tag}.indptr"] = m.indptr.astype(np.int64)
            out[f"{norm}.{tag}.indices"] = m.indices.astype(np.int64)
            out[f"{norm}.{tag}.data"] = m.data.astype(np.float32)
        for h in HIDDEN:
            key = f"{norm}.h{h}"
            torch.manual_seed(SEED)
            model = quiet(GCN, nfeat=NF, nhid=h, nclass=C, dropout=0.0)
            model64 = copy.deepcopy(model).double()
            for name, p in model.state_dict().items():
                out[f"{key}.init.{name}"] = p.numpy().copy()
            l32, c32, _, z32 = train(model, X1, t1, Y1, X2, t2)
            l64, c64, tiny64, z64 = train(model64, X1.double(), t1.double(), Y1, X2.double(), t2.double())
            for name, p in model.state_dict().items():
                out[f"{key}.final32.{name}"] = p.numpy().copy()
            for name, p in model64.state_dict().items():
                out[f"{key}.final64.{name}"] = p.numpy().copy()
            out.update({f"{key}.loss32": l32, f"{key}.loss64": l64, f"{key}.correct32": c32, f"{key}.correct64": c64,
                        f"{key}.tiny64": tiny64, f"{key}.logits2_32": z32, f"{key}.logits2_64": z64})
            print(f"{key}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, acc {c64[-1] / N1:.3f}, "
                  f"|loss32 - loss64| max {np.abs(l32 - l64).max():.2e}")
    save("train.npz", out)


if __name__ == "__main__":
    main()

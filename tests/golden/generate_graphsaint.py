#!/usr/bin/env python3
"""Generate ``graphsaint_loader.npz`` by running the REFERENCE's own loader and ``Worker`` on two tiny synthetic datasets in the
GraphSAINT layout (``role.json``, ``feats.npy``, ``class_map.json``, ``adj_full.npz``), written under the names the reference
expects (``./data/flickr``, ``./data/ppi`` of a temporary working directory).

Runs only where the reference tree is available (``LT_REFERENCE`` names its directory); the resulting file is committed and is
the only thing that travels.  No reference source is copied: its modules are imported from where they lie.

    LT_REFERENCE=<reference tree> PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_graphsaint.py

  flickr   n = 60, F = 12, 7 classes (single label), class 6 absent from the training rows, two training nodes isolated in the
           training subgraph
  ppi      the same graph, features and split with 5 binary labels per node

The fixture stores the input arrays next to the reference's outputs: the test rebuilds the files from the inputs with
``synth.write_graphsaint_dataset`` and compares ``linkteller_amd.worker.Worker`` with the stored outputs bit for bit.
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("LT_REFERENCE")
if not REF or not os.path.isdir(REF):
    sys.exit("set LT_REFERENCE to the directory of the reference implementation")
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

from linkteller_amd import synth  # noqa: E402

import worker as ref_worker        # noqa: E402  the reference's worker.py

torch.set_num_threads(1)
N, NF, NC, NL = 60, 12, 7, 5


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*a, **k)


def csr_parts(a):
    a = sp.csr_matrix(a)
    a.sort_indices()
    return dict(indptr=a.indptr.astype(np.int64), indices=a.indices.astype(np.int64), data=np.asarray(a.data),
                shape=np.asarray(a.shape, dtype=np.int64), dtype=np.array(str(a.dtype)))


def inputs():
    rng = np.random.RandomState(71)
    perm = rng.permutation(N)
    roles = {"tr": perm[:30].tolist(), "va": perm[30:45].tolist(), "te": perm[45:].tolist()}     # unsorted on purpose
    adj = synth.erdos_renyi_graph(N, 150, seed=72).tolil()
    train = set(roles["tr"])
    for u in roles["tr"][:2]:              # two training nodes keep only their edges to nodes outside the training set
        for v in list(adj.rows[u]):
            if v in train:
                adj[u, v] = 0
                adj[v, u] = 0
    adj = sp.csr_matrix(adj)
    adj.eliminate_zeros()
    adj = adj.astype(np.float64)           # adj_full.npz of the published datasets stores float64 data
    sub = adj[sorted(roles["tr"]), :][:, sorted(roles["tr"])]
    assert int((np.diff(sub.indptr) == 0).sum()) >= 2
    feats = rng.standard_normal((N, NF)) * rng.uniform(0.5, 3.0, NF) + rng.uniform(-2, 2, NF)
    feats[:, 3] = 1.25                     # a zero-variance column: StandardScaler leaves its scale at 1
    single = rng.randint(0, NC - 1, N)
    single[roles["va"][0]] = NC - 1        # class 6 only outside the training rows
    single[roles["te"][0]] = NC - 1
    assert NC - 1 not in set(single[roles["tr"]]) and single.max() == NC - 1
    multi = (rng.random_sample((N, NL)) < 0.4).astype(np.int64)
    return roles, adj, feats, single, multi


def main():
    roles, adj, feats, single, multi = inputs()
    out = {"in.feats": feats, "in.labels.flickr": single, "in.labels.ppi": multi}
    for k in ("tr", "va", "te"):
        out[f"in.role.{k}"] = np.asarray(roles[k], dtype=np.int64)
    for k, v in csr_parts(adj).items():
        out[f"in.adj.{k}"] = v
    cwd = os.getcwd()
    cuda_was = torch.cuda.is_available
    torch.cuda.is_available = lambda: False
    try:
        with tempfile.TemporaryDirectory() as td:
            for name, labels in (("flickr", single), ("ppi", multi)):
                synth.write_graphsaint_dataset(os.path.join(td, "data"), name, adj, feats, labels, roles)
            os.chdir(td)
            for name in ("flickr", "ppi"):
                args = argparse.Namespace(mode="vanilla-clean", norm="FirstOrderGCN", scale="small", train_ratio=0.5,
                                          feature_size=-1, perturb_type="continuous", epsilon=5.0, noise_seed=42,
                                          noise_type="laplace", delta=1e-5)
                w = quiet(ref_worker.Worker, args, dataset=name, mode="vanilla-clean")
                assert not w.transfer
                out[f"{name}.features"] = w.features.numpy()
                out[f"{name}.features_train"] = w.features_train.numpy()
                out[f"{name}.labels"] = w.labels.numpy()
                for k in ("idx_train", "idx_val", "idx_test"):
                    out[f"{name}.{k}"] = np.asarray(getattr(w, k))
                out[f"{name}.sizes"] = np.array([w.n_nodes, w.n_features, w.n_classes, w.multi_label], dtype=np.int64)
                for k, v in csr_parts(w.adj_ori).items():
                    out[f"{name}.adj_ori.{k}"] = v
                # the unnormalised adj_train / adj_full: what the reference's load_data holds when it calls prepare_data
                prepare = ref_worker.Worker.prepare_data
                ref_worker.Worker.prepare_data = lambda self: None
                try:
                    raw = quiet(ref_worker.Worker, args, dataset=name, mode="vanilla-clean")
                finally:
                    ref_worker.Worker.prepare_data = prepare
                for which in ("adj_train", "adj_full"):
                    for k, v in csr_parts(getattr(raw, which)).items():
                        out[f"{name}.{which}_raw.{k}"] = v
                for which in ("adj_train", "adj_full"):
                    t = getattr(w, which).coalesce()
                    out[f"{name}.clean.{which}.indices"] = t.indices().numpy()
                    out[f"{name}.clean.{which}.values"] = t.values().numpy()
                    out[f"{name}.clean.{which}.shape"] = np.array(t.shape, dtype=np.int64)
    finally:
        torch.cuda.is_available = cuda_was
        os.chdir(cwd)
    path = os.path.join(HERE, "graphsaint_loader.npz")
    np.savez_compressed(path, **out)
    print(f"wrote graphsaint_loader.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ms per epoch of transductive training -- the whole graph forwarded, the loss over m listed rows
(lt_gcn2_trainer_set_train_rows) -- on synthetic graphs at three shapes, 2-layer GCN, dropout 0.5:

  shape    n       stored entries (self loops included)   F      C   H     m
  cora     2 708   13 264                                 1 433  7   16    140
  pubmed   19 717  108 365                                500    3   16    60
  flickr   89 250  2 x 899 756 + 89 250                   500    7   256   44 625

  listed        this library, the list set                                          (a)
  torch         stock torch on the same GPU running the reference's loop: autograd,
                F.cross_entropy(out[idx], y[idx]), optim.Adam, F.dropout               (b)
  all_rows      this library, no list: the epoch every earlier build ran              (c)
  all_rows_2    a second trainer of this library, no list: the control -- what two
                instances of ONE build differ by (their buffers lie elsewhere)
  parent        --parent-lib PATH: the same all-rows epoch through another build of the
                library (the parent commit's), loaded beside this one                 (c)

The three library variants go through the C entry points directly (one host path for both builds).  The variants are timed in
alternating blocks inside one process, each block --epochs epochs between two events after --warmup warm-up epochs; the
figure is the median over --blocks blocks with the blocks' minimum and maximum.  No time is fixed in advance; two things are
read off the blocks and written next to them:

  all_rows_inside_parent_spread   this build's all-rows median lies inside [min, max] of the parent's blocks
  listed_within_parent_spread     the listed median is at most the parent's all-rows median + (max - min) of its blocks

  control_difference_ms           |all_rows - all_rows_2| of the medians: differences below it say nothing about the code

    python tools/train_rows_time.py [--parent-lib PATH] [--shapes cora pubmed flickr] [--out profiles/train_rows_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/train_rows_time.py --trace
        (--trace: 20 listed and 20 all-rows epochs per shape and nothing else: the per-kernel averages; the listed head's
         kernels are the <.., true> instantiations)
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_wide_time as W2  # noqa: E402  (the event clock, the sparse tensor)
from linkteller_amd import _lib, graph, synth  # noqa: E402

#          n,     undirected edges, F,    C, H,   m
SHAPES = {"cora": (2708, 5278, 1433, 7, 16, 140),
          "pubmed": (19717, 44324, 500, 3, 16, 60),
          "flickr": (89250, 899756, 500, 7, 256, 44625)}
LR, DECAY, DROPOUT, SEED = 0.01, 5e-4, 0.5, 42


def load(path):
    """Another build of the library beside the one linkteller_amd loaded: the signatures of the entry points it has."""
    handle = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(handle, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return handle


class RawTrainer:
    """lt_gcn2_trainer_* of one build of the library, with its own lt_graph."""

    def __init__(self, lib, adj, x, y, init, rows=None):
        self.lib, dev = lib, x.device
        _, rowptr, col, val = graph.csr_arrays(adj)
        self.g, self.h = C.c_void_p(), C.c_void_p()
        self._ok(lib.lt_graph_create(adj.shape[0], int(col.shape[0]), rowptr.ctypes.data, col.ctypes.data, val.ctypes.data,
                                     C.byref(self.g)))
        self.keep = (x, y.to(torch.int32).contiguous(), [torch.from_numpy(t.copy()).to(dev) for t in init])
        n, f = x.shape
        self._ok(lib.lt_gcn2_trainer_create(self.g, x.data_ptr(), f, f, self.keep[1].data_ptr(), init[0].shape[1], init[2].shape[1],
                                            *[t.data_ptr() for t in self.keep[2]], LR, DECAY, DROPOUT, SEED, self._stream(),
                                            C.byref(self.h)))
        if rows is not None:
            host = np.ascontiguousarray(rows, dtype=np.int32)
            self._ok(lib.lt_gcn2_trainer_set_train_rows(self.h, host.ctypes.data, len(host), self._stream()))
        self.record = torch.empty((1 << 12, 2), dtype=torch.float32, device=dev)

    @staticmethod
    def _stream():
        return torch.cuda.current_stream().cuda_stream

    def _ok(self, status):
        if status != 0:
            raise RuntimeError(self.lib.lt_last_error().decode("utf-8", "replace"))

    def run(self, k):
        self._ok(self.lib.lt_gcn2_trainer_run(self.h, k, self.record.data_ptr(), self._stream()))

    def close(self):
        torch.cuda.synchronize()
        self._ok(self.lib.lt_gcn2_trainer_destroy(self.h))
        self._ok(self.lib.lt_graph_destroy(self.g))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.epochs <= 1 << 12 and a.warmup <= 1 << 12
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    this = _lib.lib()
    parent = load(a.parent_lib) if a.parent_lib else None
    out_rows = []
    for name in a.shapes:
        n, e, nf, c, h, m = SHAPES[name]
        rng = np.random.RandomState(11)
        adj = graph.first_order_gcn(synth.erdos_renyi_graph(n, e, seed=1))
        x = torch.from_numpy(synth.gaussian_features(n, nf, seed=2)).to(dev)
        y = torch.from_numpy(rng.randint(0, c, n)).to(dev)
        idx = np.sort(rng.permutation(n)[:m])
        w = synth.gcn_weights(nf, h, c, seed=4)
        init = [w[k] for k in ("W1", "b1", "W2", "b2")]

        trainers = {"listed": RawTrainer(this, adj, x, y, init, rows=idx), "all_rows": RawTrainer(this, adj, x, y, init)}
        if a.trace:
            for t in trainers.values():
                t.run(20)
                t.close()
            continue
        trainers["all_rows_2"] = RawTrainer(this, adj, x, y, init)
        if parent is not None:
            trainers["parent"] = RawTrainer(parent, adj, x, y, init)
        a_t = W2.sparse_tensor(adj, dev)
        idx_t = torch.from_numpy(idx).to(dev)
        ps = [torch.from_numpy(t.copy()).to(dev).requires_grad_() for t in init]
        opt = torch.optim.Adam(ps, lr=LR, weight_decay=DECAY)

        def torch_epochs(k):
            for _ in range(k):
                opt.zero_grad()
                hid = F.dropout(torch.relu(torch.sparse.mm(a_t, x @ ps[0]) + ps[1]), DROPOUT, training=True)
                out = torch.sparse.mm(a_t, hid @ ps[2]) + ps[3]
                F.cross_entropy(out[idx_t], y[idx_t]).backward()
                opt.step()

        variants = {k: (lambda t: lambda: W2.event_ms(t.run, a.epochs))(t) for k, t in trainers.items()}
        variants["torch"] = lambda: W2.event_ms(torch_epochs, a.epochs)
        for t in trainers.values():
            t.run(a.warmup)
        torch_epochs(a.warmup)
        torch.cuda.synchronize()
        samples = {k: [] for k in variants}
        for _ in range(a.blocks):
            for k, fn in variants.items():
                samples[k].append(fn())
        row = {"shape": name, "n": n, "stored_entries": int(adj.nnz), "F": nf, "C": c, "H": h, "m": m, "epochs": a.epochs,
               "blocks": a.blocks}
        for k, v in samples.items():
            row[f"{k}_ms"] = round(float(np.median(v)), 4)
            row[f"{k}_min_ms"], row[f"{k}_max_ms"] = round(float(min(v)), 4), round(float(max(v)), 4)
            row[f"{k}_blocks_ms"] = [round(float(t), 4) for t in v]
        row["torch_over_listed"] = round(row["torch_ms"] / row["listed_ms"], 2)
        row["control_difference_ms"] = round(abs(row["all_rows_ms"] - row["all_rows_2_ms"]), 4)
        if parent is not None:
            lo, hi, med = min(samples["parent"]), max(samples["parent"]), float(np.median(samples["parent"]))
            row["all_rows_inside_parent_spread"] = bool(lo <= np.median(samples["all_rows"]) <= hi)
            row["listed_within_parent_spread"] = bool(np.median(samples["listed"]) <= med + (hi - lo))
        print(json.dumps(row), flush=True)
        out_rows.append(row)
        for t in trainers.values():
            t.close()
    if a.out and out_rows:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"dropout": DROPOUT, "lr": LR, "weight_decay": DECAY, "parent_lib": bool(parent is not None), "rows": out_rows},
                      fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ms per epoch of training with validation every epoch, at twitch-ES shape for both graphs (synthetic ER graphs, N = 4648,
E = 59 382, F = 3170, C = 2, dropout 0.5), H = 16 and 256, both model families (GCN3: hidden2 = 16):

  plain   run_async(k)                                                  the training launches alone
  log     run_validated_async(k), nothing kept                         + forward on the held-out graph, head, state
  best    run_validated_async(k), keep_best                            + the predicated snapshot launch
  early   run_validated(k, chunk = 10), keep_best                      + one 32-byte state read per 10 epochs and the records'
                                                                        read-back at the end, wall clock (the patience is set
                                                                        so large that no block stops: every block times all
                                                                        of its epochs)
  host    the reference's way: run(1), then per epoch a synchronisation, the eval-mode forward through the module's own
          kernels, the loss read back, and a deepcopy of the parameters to the host when it improved

The variants are timed in alternating blocks inside one process (plain, log, best, early, host, plain, ...), each block
--epochs epochs behind device events (host: wall clock around a synchronise); the figure is the median over --blocks blocks
and ``spread`` the (max - min) / median of the plain blocks, the run-to-run noise against which "plain is unchanged" is read.

    python tools/validate_time.py [--hidden 16 256] [--epochs 200] [--blocks 5] [--out profiles/validate_time.json]
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

N, E, NF, C, H2 = 4648, 59382, 3170, 2, 16
CHUNK = 10      # epochs per state read of the `early` variant: the default chunk at the command line's default --patience


def event_ms(fn, epochs):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    done = fn(epochs)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / (done or epochs)


def wall_ms(fn, epochs):
    torch.cuda.synchronize()
    t = time.perf_counter()
    done = fn(epochs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / (done or epochs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    adj1 = graph.first_order_gcn(synth.erdos_renyi_graph(N, E, seed=1))
    adj2 = graph.first_order_gcn(synth.erdos_renyi_graph(N, E, seed=5))
    x1 = torch.from_numpy(synth.twitch_like_features(N, NF, seed=2)).to(dev)
    x2 = torch.from_numpy(synth.twitch_like_features(N, NF, seed=6)).to(dev)
    y1 = torch.from_numpy(np.random.RandomState(3).randint(0, C, N)).to(dev)
    y2 = torch.from_numpy(np.random.RandomState(7).randint(0, C, N)).to(dev)
    g1, g2 = engine.as_hip_graph(adj1), engine.as_hip_graph(adj2)
    rows = []
    for family in ("gcn2", "gcn3"):
        for h in a.hidden:
            def make(keep_best=None, patience=0):
                w = synth.gcn_weights(NF, h, H2 if family == "gcn3" else C, seed=4)
                params = [torch.from_numpy(w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")]
                if family == "gcn3":
                    w3 = synth.gcn_weights(H2, C, C, seed=8)
                    params += [torch.from_numpy(w3["W1"]).to(dev), torch.from_numpy(w3["b1"]).to(dev)]
                cls = engine.GCN3Trainer if family == "gcn3" else engine.GCN2Trainer
                tr = cls(g1, x1, y1, *params, lr=0.01, weight_decay=5e-4, dropout=0.5, seed=42)
                if keep_best is not None:
                    tr.attach_validation(g2, x2, y2, keep_best=keep_best, patience=patience)
                return tr
            plain, log, best = make(), make(False), make(True)
            host = make()
            early = make(True, 1 << 30)      # never exhausted: every block runs all its epochs, in chunks of CHUNK

            def host_forward():
                p = host.params
                if family == "gcn2":
                    return engine.gcn2_forward(g2, x2, *p)
                h1 = engine.spmm(g2, engine.gemm(x2, p[0]), p[1], relu=True)
                h2 = engine.spmm(g2, engine.gemm(h1, p[2]), p[3], relu=True)
                return engine.spmm(g2, engine.gemm(h2, p[4]), p[5])
            kept = {"loss": float("inf"), "model": None}

            def host_epochs(k):
                for _ in range(k):
                    host.run(1)                                            # synchronises: the record is read
                    loss = float(torch.nn.functional.cross_entropy(host_forward(), y2))
                    if not loss > kept["loss"]:
                        kept["loss"], kept["model"] = loss, copy.deepcopy([p.cpu() for p in host.params])
                return k
            variants = {
                "plain": lambda: event_ms(lambda k: plain.run_async(k) is None and None, a.epochs),
                "log": lambda: event_ms(lambda k: log.run_validated_async(k) is None and None, a.epochs),
                "best": lambda: event_ms(lambda k: best.run_validated_async(k) is None and None, a.epochs),
                "early": lambda: wall_ms(lambda k: len(early.run_validated(k, chunk=CHUNK)["loss"]), a.epochs),
                "host": lambda: wall_ms(host_epochs, max(a.epochs // 4, 1)),
            }
            for tr in (plain, log, best):
                tr.run_async(a.warmup)
            log.run_validated_async(a.warmup)
            best.run_validated_async(a.warmup)
            host_epochs(3)
            torch.cuda.synchronize()
            samples = {k: [] for k in variants}
            for _ in range(a.blocks):
                for name, fn in variants.items():
                    samples[name].append(fn())
            row = {"family": family, "hidden": h, "epochs": a.epochs, "blocks": a.blocks}
            for name, v in samples.items():
                row[f"{name}_ms_per_epoch"] = round(float(np.median(v)), 4)
            row["plain_spread"] = round(float((max(samples["plain"]) - min(samples["plain"])) / np.median(samples["plain"])), 4)
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"shape": {"N": N, "E": E, "F": NF, "C": C, "hidden2": H2, "dropout": 0.5}, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

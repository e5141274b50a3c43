"""Edge-DP graph generation: the numpy noise stream (an N x N draw on the host) against the Philox cell stream evaluated on
the device (dp.perturb_adj*(..., rng="philox"): lt_lapgraph_philox / lt_edgerand_philox).

    python tools/dp_time.py [--out profiles/dp_time.json] [--reps 5] [--big 17 20]

  (a) at twitch-RU shape (ER graph, N = 4385, E = 37 304, eps 5): wall time of ``perturb_adj_continuous`` and
      ``perturb_adj_discrete`` by both rngs, each the median of ``--reps`` calls after one warm-up call, in ONE process (host
      clock around a call that ends with its result on the host as a scipy matrix);
  (b) the philox LapGraph selection alone (``dp.lapgraph_philox_select``: CSR upload, scans, exact select, cells sorted on
      the host) at n = 2^17 and 2^20 on an ER graph of average degree 16, eps 5: wall time, workspace bytes, candidates,
      scan passes and the cell rate of the streaming pass (cells / second over all passes, selection included).
The two rngs give different graphs for one seed (different streams); what is compared is the time to a served graph.
Needs a GPU; writes one JSON file."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import argparse, contextlib, ctypes as C, io, json, time
import numpy as np, scipy.sparse as sp, torch
from linkteller_amd import _lib, dp, synth


def timed(fn, reps):
    with contextlib.redirect_stdout(io.StringIO()):
        fn()                                            # warm-up
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
    return {"median_s": round(float(np.median(ts)), 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "dp_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, nargs="*", default=[17, 20], help="log2 of the node counts of part (b)")
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "eps": 5.0, "seed": 42}
    n, e = 4385, 37304
    adj = sp.csr_matrix(synth.erdos_renyi_graph(n, e, seed=0))
    row = {"n": n, "edges": e}
    for name, fn in (("continuous", dp.perturb_adj_continuous), ("discrete", dp.perturb_adj_discrete)):
        for rng in ("numpy", "philox"):
            row[f"{name}_{rng}"] = timed(lambda: fn(adj, 5.0, 42, rng=rng), a.reps)
            print(name, rng, row[f"{name}_{rng}"], flush=True)
        row[f"{name}_numpy_over_philox"] = round(row[f"{name}_numpy"]["median_s"] / row[f"{name}_philox"]["median_s"], 2)
    res["twitch_ru"] = row
    for lg in a.big:
        n = 1 << lg
        e = 8 * n
        t = time.perf_counter()
        adj = sp.csr_matrix(synth.erdos_renyi_graph(n, e, seed=1))
        print(f"n = 2^{lg}: graph built in {time.perf_counter() - t:.1f} s", flush=True)
        n_keep = e + int(dp.philox_edge_count_draw(42, 0.05))
        need = C.c_size_t(0)
        _lib.check(_lib.lib().lt_lapgraph_philox_workspace(n, adj.nnz, n_keep, C.byref(need)))
        runs = []
        for _ in range(3 if lg <= 17 else 2):           # the first is the warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            cells, info = dp.lapgraph_philox_select(adj, 42, np.exp(4.95), n_keep)
            runs.append(time.perf_counter() - t)
            print(f"n = 2^{lg}: {runs[-1]:.3f} s, passes {int(info[2])}, candidates {int(info[1])}", flush=True)
        total = n * (n - 1) // 2
        best = min(runs[1:])
        res[f"lapgraph_philox_2^{lg}"] = {"n": n, "edges": e, "n_keep": n_keep, "cells": total, "workspace_bytes": need.value,
                                          "scan_passes": int(info[2]), "candidates": int(info[1]), "first_call_s": round(runs[0], 4),
                                          "later_calls_s": [round(r, 4) for r in runs[1:]],
                                          "cells_per_s": float(f"{total * int(info[2]) / best:.4g}"),
                                          "kept_edges": int(np.isin(cells, (lambda c: c.row.astype(np.int64) * n + c.col)(sp.tril(adj, -1).tocoo())).sum())}
        print(json.dumps(res[f"lapgraph_philox_2^{lg}"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

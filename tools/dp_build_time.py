"""From a noise seed to a HipGraph that is ready to serve, by the host route and by the device route of the philox DP graphs
(``--dp-build host`` / ``device``), stage by stage in ONE process:

    python tools/dp_build_time.py [--out profiles/dp_build_time.json] [--reps 5] [--big 17 20] [--norm FirstOrderGCN]

  stage      host route                                                  device route
  perturb    dp.perturb_adj(..., rng="philox") -> scipy                  dp.perturb_adj_device -> (rowptr, col) on the device
  normalise  graph.fetch_normalization(norm)(m)                          graph.normalize_device
  tensor     graph.sparse_mx_to_torch_sparse_tensor(m).cuda()            graph.torch_sparse_from_device_csr
  graph      HipGraph.from_torch_sparse(t) (coalesce, bincount, create)  HipGraph.from_device_csr(rowptr, col, val)

Shapes: twitch-RU (ER graph, N = 4385, E = 37 304; LapGraph and EdgeRand, eps 5) and n = 2^17, 2^20 with average degree 16
(LapGraph, eps 5); for LapGraph the device route's perturb stage is also cut into selection and symmetrisation.  Every stage is
the median of ``--reps`` runs after one warm-up run of the whole route; a stage ends with a device synchronise, so host clocks
around it are stage times.  Both routes serve the same graph (tests/test_dp_device_gpu.py); the host route is unchanged code and
is the yardstick of the same run.  Needs a GPU; writes one JSON file."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import argparse, contextlib, io, json, time
import numpy as np, scipy.sparse as sp, torch
from linkteller_amd import _lib, dp, graph, synth

STAGES = ("perturb", "normalise", "tensor", "graph")


def host_route(adj, perturb, eps, seed, norm):
    return (lambda _: dp.perturb_adj(adj, perturb, eps, seed, rng="philox"),
            lambda m: graph.fetch_normalization(norm)(m),
            lambda m: graph.sparse_mx_to_torch_sparse_tensor(m).cuda(),
            lambda t: graph.HipGraph.from_torch_sparse(t))


def device_route(adj, perturb, eps, seed, norm):
    return (lambda _: dp.perturb_adj_device(adj, perturb, eps, seed),
            lambda p: graph.normalize_device(norm, *p),
            lambda csr: (csr, graph.torch_sparse_from_device_csr(*csr)),       # the tensor the model and the trainer take
            lambda both: graph.HipGraph.from_device_csr(*both[0]))


def run_once(route, *args):
    """One pass through a route, each stage handed the result of the one before it: the four stage times and the graph."""
    times, val = [], None
    for stage in route(*args):
        torch.cuda.synchronize()
        t = time.perf_counter()
        val = stage(val)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return times, val


def timed(route, args, reps):
    with contextlib.redirect_stdout(io.StringIO()):
        run_once(route, *args)                             # warm-up: code objects, allocator pools
        runs = []
        for _ in range(reps):
            times, g = run_once(route, *args)
            runs.append(times)
    runs = np.array(runs)
    out = {s: {"median_s": round(float(np.median(runs[:, k])), 5), "min_s": round(float(runs[:, k].min()), 5),
               "max_s": round(float(runs[:, k].max()), 5)} for k, s in enumerate(STAGES)}
    out["total_median_s"] = round(float(np.median(runs.sum(axis=1))), 5)
    out["reps"] = reps
    out["served_nnz"] = int(g.nnz)
    return out


def lapgraph_perturb_parts(adj, eps, seed, reps):
    """The device route's perturb stage of LapGraph cut in two: the philox selection (lt_lapgraph_philox, the CSR already on the
    device) and the symmetrisation of its cells (lt_sym_csr_from_cells with its 32-byte read-back)."""
    rowptr, col, nnz = dp._device_csr(adj)
    n = adj.shape[0]
    with contextlib.redirect_stdout(io.StringIO()):
        n_keep, eps_2 = dp._lapgraph_philox_n_keep(n, adj.nnz // 2, eps, seed)
    runs = []
    for _ in range(reps + 1):                              # the first is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cells, _ = dp._lapgraph_philox_cells(rowptr, col, nnz, seed, np.exp(eps_2), n_keep)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        dp._checked_sym_csr(n, cells, None, None)
        torch.cuda.synchronize()
        runs.append((t1 - t0, time.perf_counter() - t1))
    runs = np.array(runs[1:])
    return {"select_median_s": round(float(np.median(runs[:, 0])), 5), "symmetrise_median_s": round(float(np.median(runs[:, 1])), 5),
            "cells": int(n_keep), "reps": reps}


def measure(tag, adj, perturb, eps, seed, norm, reps):
    row = {"n": int(adj.shape[0]), "edges": int(adj.nnz // 2), "perturb": perturb, "eps": eps, "norm": norm}
    for name, route in (("host", host_route), ("device", device_route)):
        row[name] = timed(route, (adj, perturb, eps, seed, norm), reps)
        print(tag, name, json.dumps(row[name]), flush=True)
    # the host EdgeRand route serves its cleared non-edges as explicit zeros: the same graph with more stored entries
    assert perturb == "discrete" or row["host"]["served_nnz"] == row["device"]["served_nnz"], "the two routes serve different graphs"
    row["host_over_device"] = round(row["host"]["total_median_s"] / row["device"]["total_median_s"], 2)
    if perturb == "continuous":
        row["device_perturb_parts"] = lapgraph_perturb_parts(adj, eps, seed, reps)
        print(tag, "device perturb parts", json.dumps(row["device_perturb_parts"]), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "dp_build_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, nargs="*", default=[17, 20], help="log2 of the node counts of the large LapGraph shapes")
    ap.add_argument("--norm", default="FirstOrderGCN")
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "eps": 5.0, "seed": 42, "norm": a.norm, "stages": list(STAGES)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def save():                                            # after every shape: a run that is cut short keeps what it measured
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    adj = sp.csr_matrix(synth.erdos_renyi_graph(4385, 37304, seed=0))
    res["twitch_ru_lapgraph"] = measure("twitch-RU LapGraph", adj, "continuous", 5.0, 42, a.norm, a.reps)
    res["twitch_ru_edgerand"] = measure("twitch-RU EdgeRand", adj, "discrete", 5.0, 42, a.norm, a.reps)
    save()
    for lg in a.big:
        n = 1 << lg
        t = time.perf_counter()
        adj = sp.csr_matrix(synth.erdos_renyi_graph(n, 8 * n, seed=1))
        print(f"n = 2^{lg}: graph built in {time.perf_counter() - t:.1f} s", flush=True)
        res[f"lapgraph_2^{lg}"] = measure(f"2^{lg} LapGraph", adj, "continuous", 5.0, 42, a.norm, a.reps)
        save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()

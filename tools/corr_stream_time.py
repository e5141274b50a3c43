"""Whole-graph edge recovery for the baseline attacks: the correlation square in bands of rows (engine.CorrRows, lt_corr_rows)
through engine.TopPairsStream, against the one-piece square (lt_corr_square) + engine.top_pairs_lower.

    python tools/corr_stream_time.py [--parts a b] [--out profiles/corr_stream_time.json] [--blocks 5] [--reps 3]

  (a) twitch-RU shape (synth.twitch_like_problem("twitch-RU", hidden=256): N = 4385), every node, m = the 4r rung of the density
      ladder, for ``baseline-feat`` (D = 3170 standardised indicators) and ``baseline`` (D = 2 posteriors).  The whole
      ``Attacker.recover_edges()`` call one-shot against ``chunk=256`` and ``chunk=1024``, each with the trapezoid
      (``Attacker.corr_trapezoid``) on and off: ONE process, ALTERNATING blocks after a warm-up of all, per route the median of
      the blocks' medians with min and max (host clock around calls that end in host copies).  All routes are compared once,
      exact.  ``rows_ms``: the streamed call's prepare + rows launches alone, the device waited for once after the last (no
      selector), with the 64 x 64 tiles they compute and the fp64 rate that makes against 78.6 TFLOP/s -- an ASSUMED peak of
      v_mfma_f64_16x16x4_f64 (32 FLOP/clk/SIMD at 2.4 GHz: half the F32 matrix row of the micro-architecture guide, which lists
      no f64 figure; not measured).  The time includes the handle's construction (allocations, memset, column sums, mean, the
      diagonal tiles); the FLOP count is the band tiles' alone: the fraction is a lower bound for the rows kernel.
  (b) flickr's shape (ER graph, N = 89 250, 899 756 edges; D = 500 Gaussian features / D = 7 posteriors), every node,
      ``Attacker.recover_graph(chunk=1024)`` once each: wall time, ``torch.cuda.max_memory_allocated()`` + the selector's bytes,
      the rows handle's bytes, against the n^2 * 4 bytes of a square.
Needs a GPU; writes one JSON file."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import argparse, json, time, types
import numpy as np, scipy.sparse as sp, torch
from linkteller_amd import _lib, engine, graph, recover, synth
from linkteller_amd.attacker import Attacker
from linkteller_amd.gcn import GCN

F64_MFMA_PEAK = 78.6e12      # assumed, see above


def attacker_for(adj, x, w, dev, mode):
    n, f = x.shape
    model = GCN(f, w["W1"].shape[1], w["W2"].shape[1], 0.5)
    model.load_state_dict({"gc1.weight": torch.from_numpy(w["W1"]), "gc1.bias": torch.from_numpy(w["b1"]),
                           "gc2.weight": torch.from_numpy(w["W2"]), "gc2.bias": torch.from_numpy(w["b2"])})
    model.to(dev).eval()
    worker = types.SimpleNamespace(features_2=torch.from_numpy(x).to(dev), adj_ori=adj, n_nodes=n,
                                   adj_2=graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(adj)).to(dev))
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=n, sample_seed=42, influence=1e-4,
                              mode="vanilla-clean", attack_mode=mode, baseline_scores="stream")
    return Attacker(args, model, worker)


def wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def summary(ts):
    return {"block_medians_ms": [round(t, 3) for t in ts], "median_ms": round(float(np.median(ts)), 3),
            "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def rows_only(vec, observed, chunk, trapezoid, reps):
    """ms of prepare + every band's rows launches, one wait after the last; the tiles computed."""
    n = int(observed.numel())
    tiles = 0
    for b in range(0, n, chunk):
        e = min(b + chunk, n)
        tiles += -(-(e - b) // 64) * -(-(max(e - 1, 1) if trapezoid else n) // 64)

    def run():
        h = engine.CorrRows(vec, observed, chunk)
        for b in range(0, n, chunk):
            e = min(b + chunk, n)
            h.rows(b, e - b, max(e - 1, 1) if trapezoid else None)
    run()
    ms = wall_ms(run, reps)
    d = int(vec.shape[1])
    flop = tiles * 64 * 64 * 2.0 * (-(-d // 16) * 16)
    return {"rows_ms": round(ms, 3), "tiles": tiles, "tflops": round(flop / ms / 1e9, 2),
            "of_f64_mfma_peak": round(flop / (ms * 1e-3) / F64_MFMA_PEAK, 4)}


def part_a(a, dev):
    adj, x, w = synth.twitch_like_problem("twitch-RU", hidden=256, n_classes=2, seed=0)
    n = adj.shape[0]
    up = sp.triu(sp.csr_matrix(adj), 1).tocoo()
    out = {}
    for mode in ("baseline-feat", "baseline"):
        atk = attacker_for(adj, x, w, dev, mode)
        atk.test_nodes = list(range(n))
        atk.exist_edges = [(int(p), int(q)) for p, q in zip(up.row, up.col)]
        atk.nonexist_edges = []
        beliefs = [recover.density_ladder(len(atk.exist_edges), n)[-1]]
        m = int(recover.belief_counts(beliefs, n * (n - 1) // 2)[0])

        def streamed(chunk, trapezoid):
            atk.corr_trapezoid = trapezoid
            try:
                return atk.recover_edges(beliefs=beliefs, chunk=chunk)
            finally:
                atk.corr_trapezoid = True
        routes = {"one_shot": lambda: atk.recover_edges(beliefs=beliefs)}
        for chunk in (256, 1024):
            for trapezoid in (True, False):
                routes[f"chunk_{chunk}" + ("" if trapezoid else "_full_rows")] = (lambda c=chunk, t=trapezoid: streamed(c, t))
        ref = None
        for name, fn in routes.items():                          # warm-up of every route, and the comparison (exact)
            fn()
            rec = dict(fn())
            if ref is None:
                ref = rec
            for k in ("pairs", "scores", "is_edge", "counts", "tp"):
                assert np.array_equal(rec[k], ref[k]), (mode, name, k)
            assert (rec["above"], rec["tied_taken"], rec["tied_total"]) == (ref["above"], ref["tied_taken"], ref["tied_total"]), name
        blocks = {k: [] for k in routes}
        for _ in range(a.blocks):
            for name, fn in routes.items():
                blocks[name].append(wall_ms(fn, a.reps))
        vec = atk._baseline_vectors_device()
        row = {"n": n, "D": int(vec.shape[1]), "cells": n * (n - 1) // 2, "m": m, "belief": beliefs[0],
               "n_edges": len(atk.exist_edges), "exact": True, "precision": float(ref["precision"][0]),
               "recall": float(ref["recall"][0]), "tied_total": int(ref["tied_total"]), "square_bytes": 4 * n * n}
        for name, ts in blocks.items():
            row[name] = summary(ts)
        _, observed = atk._device_nodes(np.arange(n, dtype=np.int64), 0, n)
        for chunk in (256, 1024):
            for trapezoid in (True, False):
                name = f"chunk_{chunk}" + ("" if trapezoid else "_full_rows")
                row[name]["rows_only"] = rows_only(vec, observed, chunk, trapezoid, a.reps * a.blocks)
                h = engine.CorrRows(vec, observed, chunk)
                row[name]["rows_handle_bytes"] = h.device_bytes
        # the one-piece square alone, for the same rate
        engine.corr_square(vec, observed)
        ms = wall_ms(lambda: engine.corr_square(vec, observed), a.reps * a.blocks)
        te = -(-n // 64)
        flop = te * (te + 1) // 2 * 64 * 64 * 2.0 * (-(-int(vec.shape[1]) // 16) * 16)
        row["one_shot"]["square_only"] = {"ms": round(ms, 3), "tflops": round(flop / ms / 1e9, 2),
                                          "of_f64_mfma_peak": round(flop / (ms * 1e-3) / F64_MFMA_PEAK, 4)}
        out[mode] = row
    return out


def part_b(a, dev):
    N, E, NF = 89250, 899756, 500
    adj = synth.erdos_renyi_graph(N, E, seed=1)
    x = synth.gaussian_features(N, NF, seed=2)
    w = synth.gcn_weights(NF, 256, 7, seed=4)
    n_edges = sp.triu(sp.csr_matrix(adj), 1).nnz
    beliefs = [recover.density_ladder(n_edges, N)[-1]]
    out = {}
    for mode in ("baseline-feat", "baseline"):
        atk = attacker_for(adj, x, w, dev, mode)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        t = time.perf_counter()
        rec = atk.recover_graph(beliefs=beliefs, chunk=1024)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        st = atk.recover_stream_stats
        peak = int(torch.cuda.max_memory_allocated())
        row = {"n": N, "D": NF if mode == "baseline-feat" else 7, "cells": N * (N - 1) // 2, "m": int(rec["counts"][0]),
               "belief": beliefs[0], "n_edges": int(rec["n_edges"]), "wall_s": round(wall, 3), "pushes": st["pushes"],
               "selector_bytes": st["device_bytes"], "rows_handle_bytes": st["rows_device_bytes"], "torch_peak_bytes": peak,
               "peak_total_bytes": peak + st["device_bytes"], "one_shot_matrix_bytes": 4 * N * N,
               "peak_over_one_shot_matrix": round((peak + st["device_bytes"]) / (4.0 * N * N), 5),
               "precision": float(rec["precision"][0]), "recall": float(rec["recall"][0]), "tied_total": rec["tied_total"],
               "threshold": rec["threshold"]}
        assert row["peak_total_bytes"] * 10 < row["one_shot_matrix_bytes"], "the streamed route's peak is not below a tenth of n^2 * 4"
        out[mode] = row
        del atk
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "corr_stream_time.json"))
    ap.add_argument("--parts", nargs="+", default=["a", "b"], choices=["a", "b"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = os.path.abspath(a.out)
    res = json.load(open(out)) if os.path.exists(out) else {}
    res.update({"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "reps_per_block": a.reps,
                "f64_mfma_peak_tflops": F64_MFMA_PEAK / 1e12})
    eff = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "recover_stream_time.json")
    if os.path.exists(eff):                                      # the efficient attack's figures for the same graphs, beside them
        e = json.load(open(eff))
        res["efficient_attack"] = {"a_one_shot_ms": e.get("a", {}).get("one_shot", {}).get("median_ms"),
                                   "a_chunk_1024_ms": e.get("a", {}).get("chunk_1024", {}).get("median_ms"),
                                   "b_wall_s": e.get("b", {}).get("wall_s"), "b_peak_total_bytes": e.get("b", {}).get("peak_total_bytes")}
    for part in a.parts:
        res[part] = (part_a if part == "a" else part_b)(a, dev)
        print(json.dumps({part: res[part]}))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()

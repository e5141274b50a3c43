"""Whole-graph edge recovery: the streamed route (rows in probe chunks through engine.TopPairsStream) against the one-shot
n x n matrix + engine.top_pairs_lower.

    python tools/recover_stream_time.py [--parts a b] [--out profiles/recover_stream_time.json] [--blocks 5] [--reps 3]

  (a) twitch-RU shape (synth.twitch_like_problem("twitch-RU", hidden=256): N = 4385, 9.6 M cells), every node, mode `delta`,
      m = the 4r rung of the density ladder.  ``Attacker.recover_edges()`` (one shot) against ``recover_edges(chunk=256)`` and
      ``chunk=1024``, the latter also with the triangular observed lists (``Attacker.recover_triangular``): ONE process, ALTERNATING
      blocks after a warm-up of all, per route the median of the blocks' medians with min and max (host clock around calls that
      end in host copies).  The streamed route's split into rows / pushes / finish comes from a pass of its own that waits for
      the device after every stage; the handle's counters say how many chains fired.  All routes are compared once, exact.  ``idle_chain``: 256 one-row pushes
      (a chain that does not fire + a one-block scan each) against 256 trivial one-block launches, microseconds apiece.
  (b) flickr's shape (tools/graphsaint_time.py's generator: ER graph, N = 89 250, 899 756 edges, 500 features), every node,
      2-layer GCN of 256 hidden units, `delta`, ``Attacker.recover_graph(chunk=1024)`` once: wall time, pushes, chains fired, the
      share of exact zeros in a chunk's cells, and ``torch.cuda.max_memory_allocated()`` + the selector's bytes against the
      n^2 * 4 bytes of the one-shot matrix.  ``--one-shot-b`` also runs the one-shot route there, once.
Needs a GPU; writes one JSON file."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import argparse, json, time, types
import numpy as np, scipy.sparse as sp, torch
from linkteller_amd import _lib, engine, graph, recover, synth
from linkteller_amd.attacker import Attacker
from linkteller_amd.gcn import GCN


def attacker_for(adj, x, w, dev):
    n, f = x.shape
    model = GCN(f, w["W1"].shape[1], w["W2"].shape[1], 0.5)
    model.load_state_dict({"gc1.weight": torch.from_numpy(w["W1"]), "gc1.bias": torch.from_numpy(w["b1"]),
                           "gc2.weight": torch.from_numpy(w["W2"]), "gc2.bias": torch.from_numpy(w["b2"])})
    model.to(dev).eval()
    worker = types.SimpleNamespace(features_2=torch.from_numpy(x).to(dev), adj_ori=adj, n_nodes=n,
                                   adj_2=graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(adj)).to(dev))
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=n, sample_seed=42, influence=1e-4,
                              mode="vanilla-clean", attack_mode="efficient", influence_mode="delta")
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


def split_pass(atk, n, m, chunk, triangular):
    """ms of the streamed route's stages, the device waited for after each (so their sum exceeds the pipelined call)."""
    probes, observed = atk._device_nodes(np.arange(n, dtype=np.int64), 0, n)
    sel = engine.TopPairsStream(n, m, min(chunk, n))
    t_rows = t_push = 0.0
    zeros = cells = 0
    for b in range(0, n, chunk):
        e = min(b + chunk, n)
        torch.cuda.synchronize()
        t = time.perf_counter()
        rows = atk._rows(probes[b:e], observed[:e] if (triangular and e > 1) else observed)
        torch.cuda.synchronize()
        t_rows += time.perf_counter() - t
        t = time.perf_counter()
        sel.push(rows, b)
        torch.cuda.synchronize()
        t_push += time.perf_counter() - t
        if b == (n // chunk // 2) * chunk:                    # a middle chunk: the share of exact zeros among its triangle cells
            tri = torch.tril(torch.ones(e - b, e, dtype=torch.bool, device=rows.device), diagonal=b - 1)
            cells, zeros = int(tri.sum()), int(((rows[:, :e] == 0) & tri).sum())
    t = time.perf_counter()
    out = sel.finish()
    torch.cuda.synchronize()
    t_fin = time.perf_counter() - t
    stats = sel.stats()
    nbytes = sel.device_bytes
    sel.close()
    return {"rows_ms": round(t_rows * 1e3, 3), "pushes_ms": round(t_push * 1e3, 3), "finish_ms": round(t_fin * 1e3, 3),
            "pushes": -(-n // chunk), "slabs": stats["slabs"], "chains_fired": stats["fired_between"] + stats["fired_inside"],
            "selector_bytes": nbytes, "zero_share_middle_chunk": round(zeros / max(cells, 1), 4)}, out


def part_a(a, dev):
    adj, x, w = synth.twitch_like_problem("twitch-RU", hidden=256, n_classes=2, seed=0)
    atk = attacker_for(adj, x, w, dev)
    n = adj.shape[0]
    up = sp.triu(sp.csr_matrix(adj), 1).tocoo()
    atk.test_nodes = list(range(n))
    atk.exist_edges = [(int(p), int(q)) for p, q in zip(up.row, up.col)]
    atk.nonexist_edges = []
    ladder = recover.density_ladder(len(atk.exist_edges), n)
    beliefs = [ladder[-1]]
    m = int(recover.belief_counts(beliefs, n * (n - 1) // 2)[0])

    def tri(flag, chunk):
        atk.recover_triangular = flag
        try:
            return atk.recover_edges(beliefs=beliefs, chunk=chunk)
        finally:
            atk.recover_triangular = False
    routes = {"one_shot": lambda: atk.recover_edges(beliefs=beliefs), "chunk_256": lambda: tri(False, 256),
              "chunk_1024": lambda: tri(False, 1024), "chunk_1024_triangular": lambda: tri(True, 1024)}
    ref = None
    for name, fn in routes.items():                          # warm-up of every route, and the comparison (exact)
        fn()
        rec = dict(fn())
        if ref is None:
            ref = rec
        for k in ("pairs", "scores", "is_edge", "counts", "tp"):
            assert np.array_equal(rec[k], ref[k]), (name, k)
        assert (rec["above"], rec["tied_taken"], rec["tied_total"]) == (ref["above"], ref["tied_taken"], ref["tied_total"]), name
    blocks = {k: [] for k in routes}
    for _ in range(a.blocks):
        for name, fn in routes.items():
            blocks[name].append(wall_ms(fn, a.reps))
    row = {"n": n, "cells": n * (n - 1) // 2, "m": m, "belief": beliefs[0], "n_edges": len(atk.exist_edges), "exact": True,
           "precision": float(ref["precision"][0]), "recall": float(ref["recall"][0])}
    for name, ts in blocks.items():
        row[name] = summary(ts)
    for name, chunk, flag in (("chunk_256", 256, False), ("chunk_1024", 1024, False), ("chunk_1024_triangular", 1024, True)):
        split_pass(atk, n, m, chunk, flag)
        row[name]["split"] = split_pass(atk, n, m, chunk, flag)[0]
    sel = engine.TopPairsStream(n, m, 1024)
    probes, observed = atk._device_nodes(np.arange(n, dtype=np.int64), 0, n)
    rows = atk._rows(probes[:1024], observed)

    def idle():                                               # chain + scan of one slab, over and over on the first chunk
        sel.reset()
        sel.push(rows, 0)
    idle()
    row["one_push_1024_rows_ms"] = round(wall_ms(idle, 20), 4)
    # an idle chain: rows 1 .. 256 one row a push at the default slack -- every push is one chain that does not fire (its blocks
    # read the fire word and return) and a one-block scan of at most 256 cells; `scan_only` is the same count of one-block
    # launches of a trivial torch kernel, the floor of a launch on this stream
    small = rows[:257].contiguous()

    def chains():
        sel.reset()
        for i in range(257):                                  # (row 0 holds no cell: no slab, no chain)
            sel.push(small[i:i + 1], i)
    word = torch.zeros(1, device=dev)

    def launches():
        for _ in range(256):
            word.add_(1.0)
    chains(), launches()
    t_chain, t_launch = wall_ms(chains, 10), wall_ms(launches, 10)
    p_bytes = 1
    while (n * n - 1) >> (8 * p_bytes):
        p_bytes += 1
    row["idle_chain"] = {"launches_per_chain": 6 + p_bytes, "us_per_push_chain_plus_one_block_scan": round(t_chain / 256 * 1e3, 2),
                         "us_per_trivial_launch": round(t_launch / 256 * 1e3, 2),
                         "fired": sel.stats()["fired_between"] + sel.stats()["fired_inside"]}
    sel.close()
    return row


def part_b(a, dev):
    N, E, NF = 89250, 899756, 500
    adj = synth.erdos_renyi_graph(N, E, seed=1)
    x = synth.gaussian_features(N, NF, seed=2)
    w = synth.gcn_weights(NF, 256, 7, seed=4)
    atk = attacker_for(adj, x, w, dev)
    atk.recover_keep_stats = True
    n_edges = sp.triu(sp.csr_matrix(adj), 1).nnz
    beliefs = [recover.density_ladder(n_edges, N)[-1]]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t = time.perf_counter()
    rec = atk.recover_graph(beliefs=beliefs, chunk=1024)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t
    st = atk.recover_stream_stats
    peak = int(torch.cuda.max_memory_allocated())
    row = {"n": N, "cells": N * (N - 1) // 2, "m": int(rec["counts"][0]), "belief": beliefs[0], "n_edges": int(rec["n_edges"]),
           "wall_s": round(wall, 3), "pushes": st["pushes"], "slabs": st["slabs"],
           "chains_fired": st["fired_between"] + st["fired_inside"], "selector_bytes": st["device_bytes"],
           "torch_peak_bytes": peak, "peak_total_bytes": peak + st["device_bytes"], "one_shot_matrix_bytes": 4 * N * N,
           "peak_over_one_shot_matrix": round((peak + st["device_bytes"]) / (4.0 * N * N), 5),
           "precision": float(rec["precision"][0]), "recall": float(rec["recall"][0]), "tied_total": rec["tied_total"],
           "threshold": rec["threshold"]}
    assert row["peak_total_bytes"] * 10 < row["one_shot_matrix_bytes"], "the streamed route's peak is not below a tenth of n^2 * 4"
    probes, observed = atk._device_nodes(np.arange(N, dtype=np.int64), 0, N)
    b = 43 * 1024
    rows = atk._rows(probes[b:b + 1024], observed)
    tri = torch.tril(torch.ones(1024, b + 1024, dtype=torch.bool, device=dev), diagonal=b - 1)
    row["zero_share_middle_chunk"] = round(int(((rows[:, :b + 1024] == 0) & tri).sum()) / int(tri.sum()), 5)
    del rows, tri
    if a.one_shot_b:
        up = sp.triu(sp.csr_matrix(adj), 1).tocoo()
        atk.test_nodes = list(range(N))
        atk.exist_edges = list(zip(up.row.tolist(), up.col.tolist()))
        atk.nonexist_edges = []
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        t = time.perf_counter()
        one = atk.recover_edges(beliefs=beliefs)
        torch.cuda.synchronize()
        row["one_shot"] = {"wall_s": round(time.perf_counter() - t, 3), "torch_peak_bytes": int(torch.cuda.max_memory_allocated()),
                           "same_pairs": bool(np.array_equal(one["pairs"], rec["pairs"]))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "recover_stream_time.json"))
    ap.add_argument("--parts", nargs="+", default=["a", "b"], choices=["a", "b"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--one-shot-b", action="store_true")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = os.path.abspath(a.out)
    res = json.load(open(out)) if os.path.exists(out) else {}
    res.update({"device": torch.cuda.get_device_name(0), "mode": "delta", "blocks": a.blocks, "reps_per_block": a.reps})
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

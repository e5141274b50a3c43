#!/usr/bin/env python3
"""Attacking a 2-layer GCN with a wide class layer (9 .. 256 classes): the ONE handle (engine.Baseline2W, lt_baseline2w_create)
against the slice route (engine.WideBaseline: a baseline per slice of <= 8 classes, LT_WIDE2=slices), on the two synthetic graphs
of tools/train_wide_time.py (ppi's shape with C = 121; the flickr-sized graph with F = 602, C = 41), H = 256, mode `delta`,
influence = 1e-4.

  (a) matrix     Attacker.influence_matrix() at n_test = 500 random nodes, the rows widened and landed on the host (the refresh of
                 the fp64 baseline included, as every attack pays it): `handle` against `slices`.  A block is --reps matrices back
                 to back, reported per matrix.
  (b) pair list  the scoring part of `balanced-full` (every edge plus as many non-edges, sampling.construct_balanced_edge_sets,
                 seed 82; from the first launch to the float64 scores on the host): `pairs` = Attacker.pair_scores through
                 Baseline2W.influence_pairs, one call and one copy of n_pairs floats, against `rectangle` =
                 Attacker._pair_scores_rect on the slice route (1024 probes x the distinct observed nodes of their pairs per chunk:
                 what these models took before there was a list).  A rectangle chunk costs the same whichever chunk it is, so the
                 rectangle runs on the pairs of the first --rect-probes (default 2048) probes of the grouped list and its time is
                 scaled by probes / rect_probes; `rect_probes` is in the output.  The list runs whole.

Each route has an Attacker of its own (a switch of the route on one Attacker rebuilds its baseline, which is no part of either
route's time); LT_WIDE2 is set in front of every call.  Wall clock around work that ends on the host, in ALTERNATING blocks inside
one process after one warm-up of each, during which the two routes' scores are asserted to agree within 2e-5 of the largest
score (both are held to 1e-5 of the fp64 reference by the tests).  The figures are block medians with min and max; `gate` = the
first route's slowest block is faster than the second's fastest.  The default of LT_WIDE2 follows gate (a) at BOTH shapes (DESIGN
5.4).  Recorded too: the probes per chunk and the workspace bytes of the handle's calls (lt_influence2w_*_workspace_bytes) and the
bytes copied to the host.

Each shape runs in a child process of its own under a time limit; a child that fails ends the run (nothing is started behind it).

    python tools/wide2_attack_time.py [--shapes ppi reddit] [--blocks 5] [--out profiles/wide2_attack_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ("ppi", "reddit")
H, N_TEST, DELTA, CHUNK, SEED = 256, 500, 1e-4, 1024, 82


def child(name, blocks, reps, reps_pairs, rect_probes):
    import types

    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import train_wide_time as W2
    from linkteller_amd import _lib, engine, graph, sampling, synth
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN

    dev = torch.device("cuda:0")
    n, e, nf, c = W2.SHAPES[name][:4]
    raw = synth.erdos_renyi_graph(n, e, seed=1)
    x = torch.from_numpy(synth.gaussian_features(n, nf, seed=2)).to(dev)
    a_hat = graph.first_order_gcn(raw)
    torch.manual_seed(4)
    model = GCN(nf, H, c, 0.5).to(dev).eval()
    worker = types.SimpleNamespace(features_2=x, adj_ori=raw, n_nodes=n, adj_2=graph.sparse_mx_to_torch_sparse_tensor(a_hat).to(dev))
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=N_TEST, sample_seed=42, influence=DELTA,
                              mode="vanilla-clean", attack_mode="efficient", influence_mode="delta")
    nodes = np.sort(np.random.RandomState(5).choice(n, N_TEST, replace=False)).astype(np.int64)
    atk = {}
    for route in ("handle", "slices"):
        atk[route] = Attacker(args, model, worker)
        atk[route].test_nodes = nodes
    assert atk["handle"]._walk()[0] == "gcn2" and engine.wide_class_shapes(H, c)

    def on(route, fn, reps_=1):
        def run():
            os.environ["LT_WIDE2"] = route
            for _ in range(reps_):
                out = fn(atk[route])
            return out
        return run

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def stats(row, samples, first, second):
        for key, v in samples.items():
            row[f"{key}_ms"] = round(float(np.median(v)), 3)
            row[f"{key}_min_ms"], row[f"{key}_max_ms"] = round(float(min(v)), 3), round(float(max(v)), 3)
            row[f"{key}_blocks_ms"] = [round(float(t), 3) for t in v]
        row["gate"] = bool(max(samples[first]) < min(samples[second]))
        row["faster_in_every_block"] = bool(all(p < r for p, r in zip(samples[first], samples[second])))
        row["speedup"] = round(row[f"{second}_ms"] / row[f"{first}_ms"], 2)

    lib = _lib.lib()
    common = {"shape": name, "n": n, "entries_per_row": round(a_hat.nnz / n, 1), "F": nf, "H": H, "C": c, "mode": "delta", "blocks": blocks}

    def chunk_of(h, total):       # probes per chunk: where the rows call's workspace stops growing by a probe's tables
        ws = [lib.lt_influence2w_workspace_bytes(h, q, 1) for q in (total, total + 1)]
        if ws[1] - ws[0] > 4096:
            return total
        lo, hi = 1, total         # the largest q whose step from q - 1 still adds a probe's tables
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if lib.lt_influence2w_workspace_bytes(h, mid, 1) - lib.lt_influence2w_workspace_bytes(h, mid - 1, 1) > 4096:
                lo = mid
            else:
                hi = mid - 1
        return lo

    # ---- (a) the matrix ----------------------------------------------------------------------------------------------------------
    matrix = lambda a: a.influence_matrix()      # noqa: E731
    _, m_h = wall(on("handle", matrix))           # warm-up of both (code objects, the baselines' buffers, the workspaces) ...
    _, m_s = wall(on("slices", matrix))
    assert isinstance(atk["handle"]._baseline, engine.Baseline2W) and isinstance(atk["slices"]._baseline, engine.WideBaseline)
    diff = float(np.abs(m_h - m_s).max() / m_s.max())
    assert m_s.max() > 0 and diff <= 2e-5, diff   # ... and the same scores
    samples = {"handle": [], "slices": []}
    for _ in range(blocks):
        samples["handle"].append(wall(on("handle", matrix, reps))[0] / reps)
        samples["slices"].append(wall(on("slices", matrix, reps))[0] / reps)
    base_h = atk["handle"]._baseline
    h2w = base_h._h
    chunk = chunk_of(h2w, N_TEST)
    row = dict(common, measure="matrix", n_test=N_TEST, reps_per_block=reps, max_abs_diff_over_max=diff,
               nonzero_share=round(float((m_h > 0).mean()), 3), probes_per_chunk=chunk, chunks=-(-N_TEST // chunk),
               workspace_bytes={"handle": int(lib.lt_influence2w_workspace_bytes(h2w, N_TEST, N_TEST))},
               slice_baselines=len(atk["slices"]._baseline.c_slices) * len(atk["slices"]._baseline.h_slices),
               bytes_to_host={"handle": 8 * N_TEST * N_TEST, "slices": 8 * N_TEST * N_TEST})
    stats(row, samples, "handle", "slices")
    print("ROW " + json.dumps(row), flush=True)

    # ---- (b) the pair list of balanced-full --------------------------------------------------------------------------------------
    np.random.seed(SEED)
    (ex, nex), _ = sampling.construct_balanced_edge_sets("twitch/ES/RU", "balanced-full", raw, n)
    ex, nex = np.asarray(ex, dtype=np.int64).reshape(-1, 2), np.asarray(nex, dtype=np.int64).reshape(-1, 2)
    probe, observed = np.concatenate([ex[:, 0], nex[:, 0]]), np.concatenate([ex[:, 1], nex[:, 1]])
    g_nodes, g_ptr, g_obs, g_order = engine.group_pairs(probe, observed)
    n_probe = len(g_nodes)
    k = min(rect_probes, n_probe)
    k_pairs = int(g_ptr[k])

    def pairs(a):
        return a.pair_scores(probe, observed)

    def rect(a):
        scores = np.full(len(probe), np.nan)
        return a._pair_scores_rect(g_nodes[:k], g_ptr[:k + 1], g_obs[:k_pairs], g_order[:k_pairs], scores, None, CHUNK)

    os.environ["LT_WIDE2"] = "handle"
    assert atk["handle"]._pair_route() is base_h
    _, s_pairs = wall(on("handle", pairs))
    _, s_rect = wall(on("slices", rect))
    assert isinstance(atk["slices"]._baseline, engine.WideBaseline)
    sel = g_order[:k_pairs]
    assert not np.isnan(s_rect[sel]).any() and s_pairs.dtype == np.float64
    diff = float(np.abs(s_pairs[sel] - s_rect[sel]).max() / s_rect[sel].max())
    assert s_rect[sel].max() > 0 and diff <= 2e-5, diff
    samples = {"pairs": [], "rectangle": []}
    for _ in range(blocks):
        samples["pairs"].append(wall(on("handle", pairs, reps_pairs))[0] / reps_pairs)
        samples["rectangle"].append(wall(on("slices", rect))[0] * n_probe / k)
    cols = [len(np.unique(g_obs[int(g_ptr[c0]):int(g_ptr[min(c0 + CHUNK, k)])])) for c0 in range(0, k, CHUNK)]
    chunk = chunk_of(h2w, n_probe)
    row = dict(common, measure="pair_list", edges=int(len(ex)), n_pairs=int(len(probe)), n_probes=n_probe, rect_probes=k,
               rect_pairs=k_pairs, rectangle_chunk=CHUNK, reps_per_block={"pairs": reps_pairs, "rectangle": 1},
               max_abs_diff_over_max=diff, nonzero_share=round(float((s_pairs > 0).mean()), 3), probes_per_chunk=chunk,
               chunks=-(-n_probe // chunk),
               workspace_bytes={"pairs": int(lib.lt_influence2w_pairs_workspace_bytes(h2w, n_probe, len(probe))),
                                "handle_rectangle_chunk": int(lib.lt_influence2w_workspace_bytes(h2w, min(CHUNK, n_probe), max(cols)))},
               bytes_to_host={"pairs": 4 * int(len(probe)), "rectangle_measured": 4 * CHUNK * int(sum(cols)),
                              "rectangle_per_pass_scaled": int(4 * CHUNK * sum(cols) * n_probe / k)})
    stats(row, samples, "pairs", "rectangle")
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="matrices per block")
    ap.add_argument("--reps-pairs", type=int, default=2, help="list passes per block")
    ap.add_argument("--rect-probes", type=int, default=2048)
    ap.add_argument("--limit", type=int, default=280, help="seconds per shape")
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.blocks, a.reps, a.reps_pairs, a.rect_probes)
    rows = []
    for name in a.shapes:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", name, "--blocks", str(a.blocks),
               "--reps", str(a.reps), "--reps-pairs", str(a.reps_pairs), "--rect-probes", str(a.rect_probes)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; nothing more is started", flush=True)
            return r.returncode
        rows += [json.loads(line[4:]) for line in r.stdout.splitlines() if line.startswith("ROW ")]
    if a.out and rows:
        gate = all(r["gate"] for r in rows if r["measure"] == "matrix") and {r["shape"] for r in rows} >= set(SHAPES)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"hidden": H, "n_test": N_TEST, "influence": DELTA, "sample_seed": SEED,
                       "matrix_gate_at_both_shapes": bool(gate), "LT_WIDE2_default": "handle" if gate else "slices", "rows": rows},
                      fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

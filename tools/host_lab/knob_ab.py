"""Alternating blocks of host-landed headline steps (twitch-RU as bench.py builds it, `delta`, 500 x 500, every step behind a refresh)
under the values 0 / 1 of one knob, in one process: ms per step, median / min / max over the blocks; the matrix must keep its bits.
python tools/host_lab/knob_ab.py <knob> <blocks> <steps>   (e.g. feature_lists 10 50, records_early 10 50)"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from linkteller_amd import _lib, engine, graph, synth
knob, blocks, steps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
dev = torch.device("cuda:0")
adj, x_np, w = synth.twitch_like_problem("twitch-RU", hidden=256, n_classes=2, seed=0)
n = adj.shape[0]
base = engine.Baseline(graph.HipGraph(graph.first_order_gcn(adj)), torch.from_numpy(x_np).to(dev),
                       *[torch.from_numpy(w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")])
base.enable_fp64()
print("list entries", base.feature_list_entries(), "of", x_np.size, "values")
np.random.seed(42)
nodes = torch.from_numpy(np.random.choice(np.arange(n), 500, replace=False).astype(np.int32)).to(dev)
step = lambda: base.influence_matrix_host(nodes, nodes, 1e-4, "delta", refresh=True)
ref = None
for v in (0, 1):
    _lib.set_tuning(knob, v)
    for _ in range(10):
        m = step()
    if ref is None:
        ref = m.copy()
    assert np.array_equal(m, ref), knob + " changed the matrix"
res = {0: [], 1: []}
for b in range(blocks):
    for v in ((0, 1) if b % 2 == 0 else (1, 0)):
        _lib.set_tuning(knob, v)
        step()
        t = time.perf_counter()
        for _ in range(steps):
            step()
        res[v].append((time.perf_counter() - t) / steps * 1e3)
_lib.set_tuning(knob, None)
for v in (0, 1):
    print(f"{knob}={v}: median {np.median(res[v]):.4f} ms/step over {blocks} blocks of {steps} (min {min(res[v]):.4f}, max {max(res[v]):.4f})")

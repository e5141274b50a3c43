"""The packed host landing ("export_compact", lt_influence_matrix_host) against whole-row export, in one process at the headline
shape (twitch-RU as bench.py builds it, `delta`, 500 x 500, every step behind a refresh).
1. The host's share: memset of a 2 MB torch pinned block by 1 / 2 / 4 threads (ctypes calls release the GIL), warm (the block
   was just written) and cold (256 MB written elsewhere in between).  Median of 200.
2. Alternating blocks of host-landed steps with export_compact = 0 / 1; the median ms per step of each setting.
--steps-only K --compact X: K steps at one setting and nothing else (what a kernel trace of the host-landed step is taken of).
python tools/host_lab/compact_ab.py [--blocks 10] [--steps 50]"""
import argparse, ctypes, os, sys, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from linkteller_amd import _lib, engine, graph, synth

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=10)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--steps-only", type=int, default=0)
ap.add_argument("--compact", type=int, default=1)
a = ap.parse_args()

dev = torch.device("cuda:0")
adj, x_np, w = synth.twitch_like_problem("twitch-RU", hidden=256, n_classes=2, seed=0)
n = adj.shape[0]
base = engine.Baseline(graph.HipGraph(graph.first_order_gcn(adj)), torch.from_numpy(x_np).to(dev),
                       *[torch.from_numpy(w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")])
base.enable_fp64()
np.random.seed(42)
nodes = torch.from_numpy(np.random.choice(np.arange(n), 500, replace=False).astype(np.int32)).to(dev)


def step():
    return base.influence_matrix_host(nodes, nodes, 1e-4, "delta", refresh=True)


if a.steps_only:
    _lib.set_tuning("export_compact", a.compact)
    for _ in range(a.steps_only):
        step()
    print(f"export_compact={a.compact}: {a.steps_only} steps")
    sys.exit(0)

# ---- 1. host memset ----
blk = torch.empty((500, 500), dtype=torch.float64).pin_memory()
nbytes = blk.numel() * 8
evict = np.empty(256 << 20, dtype=np.uint8)


def memset_by(pool, k):
    if k == 1:
        ctypes.memset(blk.data_ptr(), 0, nbytes)
        return
    part = nbytes // k
    fs = [pool.submit(ctypes.memset, blk.data_ptr() + i * part, 0, part if i < k - 1 else nbytes - i * part) for i in range(k)]
    for f_ in fs:
        f_.result()


for k in (1, 2, 4):
    with ThreadPoolExecutor(max_workers=k) as pool:
        row = []
        for cold in (False, True):
            ts = []
            for _ in range(200):
                if cold:
                    evict.fill(1)
                else:
                    memset_by(pool, k)
                t = time.perf_counter(); memset_by(pool, k); ts.append(time.perf_counter() - t)
            row.append(f"{'cold' if cold else 'warm'} {np.median(ts) * 1e6:.1f} us")
        print(f"memset 2 MB pinned, {k} thread(s): " + ", ".join(row), flush=True)

# ---- 2. alternating A/B ----
ref = None
for c in (0, 1):
    _lib.set_tuning("export_compact", c)
    for _ in range(10):
        m = step()
    if ref is None:
        ref = m.copy()
    assert np.array_equal(m, ref), "export_compact changed the matrix"
res = {0: [], 1: []}
for blk_i in range(a.blocks):
    for c in ((0, 1) if blk_i % 2 == 0 else (1, 0)):
        _lib.set_tuning("export_compact", c)
        step()
        t = time.perf_counter()
        for _ in range(a.steps):
            step()
        res[c].append((time.perf_counter() - t) / a.steps * 1e3)
_lib.set_tuning("export_compact", None)
for c in (0, 1):
    print(f"export_compact={c}: median {np.median(res[c]):.4f} ms/step over {a.blocks} blocks of {a.steps} "
          f"(min {min(res[c]):.4f}, max {max(res[c]):.4f})")
print(f"touched share of the matrix: {np.count_nonzero(ref) / ref.size:.4f}")

"""The early half of the packed host landing ("export_early", lt_influence_matrix_host) in one process at the headline shape
(twitch-RU as bench.py builds it, `delta`, 500 x 500, every step behind a refresh).
Default: alternating blocks of host-landed steps with export_early = 0 / 1 -- ms per step (median, min, max over the blocks) and the
post-wait nanoseconds per call from lt_host_landing_stats, early / late counts.
--steps-only K --early X: K steps at one setting and nothing else (what a kernel trace is taken of).
--forms: a library built with -DLT_HOST_LAB (make CXXEXTRA=-DLT_HOST_LAB) times the post-wait section in three forms (as it is;
  reading the run only; placing from a copy the host made itself) and the early walk with and without the write-prefetch; each
  form runs in a process of its own (the library reads LT_HOST_LAB_FORM / LT_HOST_LAB_NOPF per call, so one process serves).
--lib PATH: load another build of the library (the parent's, for the same loop on the parent: it has no counters).
python tools/host_lab/early_ab.py [--blocks 10] [--steps 50]"""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from linkteller_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=10)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--steps-only", type=int, default=0)
ap.add_argument("--early", type=int, default=1)
ap.add_argument("--forms", action="store_true")
ap.add_argument("--lib", default=None)
a = ap.parse_args()
if a.lib:
    _lib.LIB_PATH = os.path.abspath(a.lib)
from linkteller_amd import engine, graph, synth
import ctypes
has_stats = hasattr(ctypes.CDLL(_lib.LIB_PATH), "lt_host_landing_stats")
if not has_stats:
    _lib.SIGNATURES.pop("lt_host_landing_stats", None)

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


def stats():
    return base.host_landing_stats() if has_stats else {"early": 0, "late": 0, "post_ns": 0, "mismatch": 0}


def timed(k):
    s0 = stats()
    t = time.perf_counter()
    for _ in range(k):
        step()
    dt = (time.perf_counter() - t) / k * 1e3
    s1 = stats()
    return dt, {q: s1[q] - s0[q] for q in s0}


if a.steps_only:
    if has_stats:
        _lib.set_tuning("export_early", a.early)
    dt, d = timed(a.steps_only)
    print(f"export_early={a.early if has_stats else 'n/a'}: {a.steps_only} steps, {dt:.4f} ms/step, {d}")
    sys.exit(0)

if a.forms:
    names = [("post-wait as it is (late form)", 0, 0, 0), ("reading the run only, no stores", 0, 1, 0),
             ("placing from a host-made copy (warm reads)", 0, 2, 0), ("early walk + write-prefetch, then placing", 1, 0, 0),
             ("early walk without prefetch, then placing", 1, 0, 1)]
    for _ in range(20):
        step()
    for rnd in range(2):
        for name, early, form, nopf in names:
            _lib.set_tuning("export_early", early)
            os.environ["LT_HOST_LAB_FORM"] = str(form)
            os.environ["LT_HOST_LAB_NOPF"] = str(nopf)
            step()
            per, ms = [], []
            for _ in range(a.blocks):
                dt, d = timed(a.steps)
                per.append(d["post_ns"] / a.steps)
                ms.append(dt)
            print(f"[{rnd}] {name}: post-wait median {np.median(per):.0f} ns (min {min(per):.0f}, max {max(per):.0f}), "
                  f"step median {np.median(ms):.4f} ms, early/late of the last block {d['early']}/{d['late']}", flush=True)
    os.environ["LT_HOST_LAB_FORM"] = "0"
    os.environ["LT_HOST_LAB_NOPF"] = "0"
    sys.exit(0)

ref = None
for e in (0, 1):
    _lib.set_tuning("export_early", e)
    for _ in range(10):
        m = step()
    if ref is None:
        ref = m.copy()
    assert np.array_equal(m, ref), "export_early changed the matrix"
res = {0: [], 1: []}
post = {0: [], 1: []}
cnt = {0: [0, 0], 1: [0, 0]}
for blk_i in range(a.blocks):
    for e in ((0, 1) if blk_i % 2 == 0 else (1, 0)):
        _lib.set_tuning("export_early", e)
        step()
        dt, d = timed(a.steps)
        res[e].append(dt)
        post[e].append(d["post_ns"] / a.steps)
        cnt[e][0] += d["early"]; cnt[e][1] += d["late"]
_lib.set_tuning("export_early", None)
for e in (0, 1):
    print(f"export_early={e}: median {np.median(res[e]):.4f} ms/step over {a.blocks} blocks of {a.steps} "
          f"(min {min(res[e]):.4f}, max {max(res[e]):.4f}); post-wait median {np.median(post[e]):.0f} ns "
          f"(min {min(post[e]):.0f}, max {max(post[e]):.0f}); early/late calls {cnt[e][0]}/{cnt[e][1]}")

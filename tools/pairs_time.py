"""Scoring listed pairs (lt_influence_pairs) against scoring rectangles (lt_influence_rows) for `balanced-full`.

    python tools/pairs_time.py [--out profiles/pairs_time.json] [--blocks 5] [--reps 5] [--big-nodes 400000]

At twitch-RU shape (synth.twitch_like_problem("twitch-RU", hidden=256), the `balanced-full` pairs of
sampling.construct_balanced_edge_sets):
  (a) the scoring part of the balanced attack, from the first launch to the float64 scores of every pair on the host, no sklearn:
      the rows path (1024 probes x every node per chunk, copied to the host, widened, fancy-indexed: the attack before the pair
      list, restated here) against ``Attacker.pair_scores``, in ALTERNATING blocks in one process -- per kind the median over the
      blocks' medians and the spread between the blocks of the same kind;
  (b) the device time of ``Baseline.influence_pairs`` alone (device events; the baseline current, lists on the device) in `delta`
      and `sparse`, and of its stage B (k_pair_stageB: the library's own launch brackets).
One larger graph whose 1024-probe chunk of rows (4 bytes x 1024 x N) alone exceeds the default 1 GiB chunk budget: pairs path only.
Needs a GPU; writes one JSON file."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import argparse, ctypes as C, json, time, types
import numpy as np, torch
from linkteller_amd import _lib, engine, graph, sampling, synth
from linkteller_amd.attacker import Attacker
from linkteller_amd.gcn import GCN


def attacker_for(adj, x, w, dev):
    n, f = x.shape
    h, c = w["W1"].shape[1], w["W2"].shape[1]
    model = GCN(f, h, c, 0.5)
    model.load_state_dict({"gc1.weight": torch.from_numpy(w["W1"]), "gc1.bias": torch.from_numpy(w["b1"]),
                           "gc2.weight": torch.from_numpy(w["W2"]), "gc2.bias": torch.from_numpy(w["b2"])})
    model.to(dev).eval()
    worker = types.SimpleNamespace(features_2=torch.from_numpy(x).to(dev), adj_ori=adj, n_nodes=n,
                                   adj_2=graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(adj)).to(dev))
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="balanced-full", n_test=n, sample_seed=82, influence=1e-4,
                              mode="vanilla-clean", attack_mode="efficient", influence_mode="delta")
    return Attacker(args, model, worker)


def rows_path(atk, ex, nex, chunk=1024):
    """link_prediction_attack_efficient_balanced before the pair list (attacker.py:250-284 on the rows primitive)."""
    n = atk.worker.n_nodes
    all_nodes = np.arange(n, dtype=np.int64)
    starts = np.union1d(ex[:, 0], nex[:, 0])
    pos = np.full(n, -1, dtype=np.int64)
    s_ex, s_nex = np.empty(len(ex)), np.empty(len(nex))
    for c0 in range(0, len(starts), chunk):
        probes = starts[c0:c0 + chunk]
        rows = atk._rows(probes, all_nodes).cpu().numpy().astype(np.float64)
        pos[:] = -1
        pos[probes] = np.arange(len(probes))
        for pairs, dst in ((ex, s_ex), (nex, s_nex)):
            sel = pos[pairs[:, 0]] >= 0
            dst[sel] = rows[pos[pairs[sel, 0]], pairs[sel, 1]]
    return np.concatenate([s_ex, s_nex])


def pairs_path(atk, ex, nex):
    return atk.pair_scores(np.concatenate([ex[:, 0], nex[:, 0]]), np.concatenate([ex[:, 1], nex[:, 1]]))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def device_ms(base, lists, mode, reps=50):
    """Median device time of one influence_pairs call (events), and of its stage-B launches (the library's brackets)."""
    nodes, ptr, obs = lists
    out = torch.empty((obs.numel(),), dtype=torch.float32, device=obs.device)
    for _ in range(5):
        base.influence_pairs(nodes, ptr, obs, 1e-4, mode, out=out)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        base.influence_pairs(nodes, ptr, obs, 1e-4, mode, out=out)
        b.record()
    torch.cuda.synchronize()
    call = float(np.median([a.elapsed_time(b) for a, b in ev]))
    h = _lib.lib()
    kid = _lib.KERNEL_IDS["item_stageB"]
    h.lt_profile_reset()
    h.lt_profile_enable(1 << kid)
    try:
        for _ in range(reps):
            base.influence_pairs(nodes, ptr, obs, 1e-4, mode, out=out)
        torch.cuda.synchronize()
        tot, cnt = C.c_double(), C.c_int64()
        _lib.check(h.lt_profile_summary(kid, C.byref(tot), C.byref(cnt)))
    finally:
        h.lt_profile_enable(0)
        h.lt_profile_reset()
    return {"call_ms": round(call, 4), "stage_b_ms": round(tot.value / max(cnt.value, 1), 4), "stage_b_launches_per_call": cnt.value / reps}


def device_lists(probe, observed, dev):
    nodes, ptr, obs, _ = engine.group_pairs(probe, observed)
    return torch.from_numpy(nodes).to(dev), ptr, torch.from_numpy(obs).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pairs_time.json"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big-nodes", type=int, default=400_000)
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}

    adj, x, w = synth.twitch_like_problem("twitch-RU", hidden=256, n_classes=2, seed=0)
    np.random.seed(82)
    (ex, nex), _ = sampling.construct_balanced_edge_sets("twitch/ES/RU", "balanced-full", adj, adj.shape[0])
    atk = attacker_for(adj, x, w, dev)
    r0, p0 = rows_path(atk, ex, nex), pairs_path(atk, ex, nex)          # warm-up of both, and: the same scores, bit for bit
    assert np.array_equal(r0, p0), np.abs(r0 - p0).max()
    blocks = {"rows": [], "pairs": []}
    for _ in range(a.blocks):
        blocks["rows"].append(timed(lambda: rows_path(atk, ex, nex), a.reps))
        blocks["pairs"].append(timed(lambda: pairs_path(atk, ex, nex), a.reps))
    tw = {"nodes": int(adj.shape[0]), "n_pairs": int(len(ex) + len(nex)), "n_probes": int(len(np.union1d(ex[:, 0], nex[:, 0]))),
          "blocks": a.blocks, "reps_per_block": a.reps, "bit_equal": True}
    for k, v in blocks.items():
        tw[k] = {"block_medians_ms": [round(t, 3) for t in v], "median_ms": round(float(np.median(v)), 3),
                 "spread_ms": round(max(v) - min(v), 3)}
    tw["rows_over_pairs"] = round(tw["rows"]["median_ms"] / tw["pairs"]["median_ms"], 2)
    base = atk.baseline("delta")
    lists = device_lists(np.concatenate([ex[:, 0], nex[:, 0]]), np.concatenate([ex[:, 1], nex[:, 1]]), dev)
    tw["pairs_call_device"] = {m: device_ms(base, lists, m) for m in ("delta", "sparse")}
    res["twitch_RU_balanced_full"] = tw
    print(json.dumps(tw))

    # the larger graph: a 1024-probe chunk of rows is 4 * 1024 * N bytes of output alone.  Every u < v edge and as many uniform
    # random pairs (the balanced sampler's scalar draws take minutes at this size; adjacency of the random pairs is not excluded)
    n, f, hdim = a.big_nodes, 64, 64
    adjb = synth.erdos_renyi_graph(n, 4 * n, seed=3)
    xb, wb = synth.twitch_like_features(n, f, seed=4, density=0.02), synth.gcn_weights(f, hdim, 2, seed=5)
    coo = adjb.tocoo()
    up = coo.row < coo.col
    exb = np.stack([coo.row[up], coo.col[up]], axis=1).astype(np.int64)
    nexb = np.random.RandomState(6).randint(0, n, size=exb.shape).astype(np.int64)
    atkb = attacker_for(adjb, xb, wb, dev)
    pairs_path(atkb, exb, nexb)
    big = {"nodes": n, "edges": int(len(exb)), "n_pairs": int(2 * len(exb)), "rows_chunk_output_bytes": 4 * 1024 * n,
           "chunk_budget_bytes": 1 << 30, "pairs_path_ms": round(timed(lambda: pairs_path(atkb, exb, nexb), a.reps), 3)}
    baseb = atkb.baseline("delta")
    listsb = device_lists(np.concatenate([exb[:, 0], nexb[:, 0]]), np.concatenate([exb[:, 1], nexb[:, 1]]), dev)
    h = _lib.lib()
    big["pairs_workspace_bytes"] = int(h.lt_influence_pairs_workspace_bytes(baseb.handle, lists_len(listsb), listsb[2].numel(), _lib.MODE_DELTA))
    big["rows_workspace_bytes_1024_probes"] = int(h.lt_influence_workspace_bytes(baseb.handle, 1024, n, _lib.MODE_DELTA))
    big["pairs_call_device"] = {m: device_ms(baseb, listsb, m, reps=10) for m in ("delta", "sparse")}
    res["larger_graph"] = big
    print(json.dumps(big))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


def lists_len(lists):
    return int(lists[0].numel())


if __name__ == "__main__":
    main()

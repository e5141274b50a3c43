"""Edge recovery: selecting the m best pairs on the device (Attacker.recover_edges) against landing the matrix and selecting on
the host (what a user did before lt_top_pairs_lower).

    python tools/recover_time.py [--out profiles/recover_time.json] [--blocks 5] [--reps 20]

At twitch-RU shape (synth.twitch_like_problem("twitch-RU", hidden=256)), `unbalanced` samples of n_test = 500 and 2000 nodes,
mode `delta`, m = the 4r rung of the density ladder (recover.density_ladder on the sample's true edge count):
  (a) the device part of ``recover_edges``: the n_test x n_test rows (``Attacker._rows``), ``engine.top_pairs_lower``, and the
      copies of the m indices, m scores and the four info words to the host;
  (b) ``Attacker.influence_matrix()`` -- the float64 matrix landed on the host -- then ``np.argpartition`` over its strict lower
      triangle at the same m (the triangle's index arrays are built once, outside the timed region).
Both in ONE process on one GPU, in ALTERNATING blocks after a warm-up of both; per route the median over the blocks' medians and
the spread between the blocks (host clock around work that ends in a device synchronisation).  (a)'s per-kernel split comes from
the library's own launch brackets (lt_profile_*), in a pass of its own.  (a) is checked once against the host restatement of the
selection (exact).  Needs a GPU; writes one JSON file."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import argparse, ctypes as C, json, time, types
import numpy as np, torch
from linkteller_amd import _lib, engine, graph, recover, synth
from linkteller_amd.attacker import Attacker
from linkteller_amd.gcn import GCN


def attacker_for(adj, x, w, dev, n_test):
    n, f = x.shape
    h, c = w["W1"].shape[1], w["W2"].shape[1]
    model = GCN(f, h, c, 0.5)
    model.load_state_dict({"gc1.weight": torch.from_numpy(w["W1"]), "gc1.bias": torch.from_numpy(w["b1"]),
                           "gc2.weight": torch.from_numpy(w["W2"]), "gc2.bias": torch.from_numpy(w["b2"])})
    model.to(dev).eval()
    worker = types.SimpleNamespace(features_2=torch.from_numpy(x).to(dev), adj_ori=adj, n_nodes=n,
                                   adj_2=graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(adj)).to(dev))
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=n_test, sample_seed=42, influence=1e-4,
                              mode="vanilla-clean", attack_mode="efficient", influence_mode="delta")
    atk = Attacker(args, model, worker)
    atk.prepare_test_data()
    return atk


def device_route(atk, nodes, m):
    probes, observed = atk._device_nodes(nodes, 0, len(nodes))
    rows = atk._rows(probes, observed)
    idx, val, info = engine.top_pairs_lower(rows, m)
    return idx.cpu().numpy(), val.cpu().numpy(), info["raw"].cpu().numpy(), rows


def host_route(atk, tri, m):
    M = atk.influence_matrix()
    t = time.perf_counter()
    v = M[tri]
    ind = np.argpartition(v, -m)[-m:]
    return ind, (time.perf_counter() - t) * 1e3


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def kernel_split(fn, reps):
    """ms per call of every launch class the route opens (the library's event brackets around its own launches)."""
    h = _lib.lib()
    h.lt_profile_reset()
    h.lt_profile_enable(-1)
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out = {}
        for name, kid in _lib.KERNEL_IDS.items():
            tot, cnt = C.c_double(), C.c_int64()
            _lib.check(h.lt_profile_summary(kid, C.byref(tot), C.byref(cnt)))
            if cnt.value:
                out[name] = {"ms_per_call": round(tot.value / reps, 5), "scopes_per_call": cnt.value / reps}
    finally:
        h.lt_profile_enable(0)
        h.lt_profile_reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "recover_time.json"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n-test", type=int, nargs="+", default=[500, 2000])
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "shape": "twitch-RU, hidden 256, mode delta", "blocks": a.blocks,
           "reps_per_block": a.reps}
    adj, x, w = synth.twitch_like_problem("twitch-RU", hidden=256, n_classes=2, seed=0)
    for n_test in a.n_test:
        atk = attacker_for(adj, x, w, dev, n_test)
        nodes = np.asarray(atk.test_nodes, dtype=np.int64)
        n_total = n_test * (n_test - 1) // 2
        ladder = recover.density_ladder(len(atk.exist_edges), n_test)
        m = int(recover.belief_counts(ladder, n_total)[-1])
        tri = np.tril_indices(n_test, -1)
        # warm-up of both routes, and (a) against the restatement
        for _ in range(3):
            idx, val, raw, rows = device_route(atk, nodes, m)
            host_route(atk, tri, m)
        M = rows.cpu().numpy()
        flat = tri[0].astype(np.int64) * n_test + tri[1]
        v = M[tri] + np.float32(0)
        order = np.lexsort((flat, -v.astype(np.float64)))
        assert np.array_equal(idx, np.sort(flat[order[:m]])), "device selection differs from the host restatement"
        assert np.array_equal(val.view(np.int32), M.reshape(-1)[idx].view(np.int32))
        blocks = {"device_select": [], "host_select": []}
        host_part = []
        for _ in range(a.blocks):
            blocks["device_select"].append(timed(lambda: device_route(atk, nodes, m), a.reps))
            blocks["host_select"].append(timed(lambda: host_part.append(host_route(atk, tri, m)[1]), a.reps))
        row = {"n_test": n_test, "m": m, "ladder": ladder, "n_edges": int(len(atk.exist_edges)), "nonzero_cells": int((v != 0).sum()),
               "threshold": float(v[order[m - 1]]), "tied_total": int(raw[3]), "tied_taken": int(raw[2]),
               "bytes_to_host_device_select": 12 * m + 32, "bytes_to_host_host_select": 8 * n_test * n_test, "exact": True}
        for k, t in blocks.items():
            row[k] = {"block_medians_ms": [round(s, 4) for s in t], "median_ms": round(float(np.median(t)), 4),
                      "spread_ms": round(max(t) - min(t), 4)}
        row["host_select"]["argpartition_part_median_ms"] = round(float(np.median(host_part)), 4)
        row["host_over_device"] = round(row["host_select"]["median_ms"] / row["device_select"]["median_ms"], 2)
        row["device_select"]["kernel_split"] = kernel_split(lambda: device_route(atk, nodes, m), a.reps)
        res[f"n_test_{n_test}"] = row
        print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

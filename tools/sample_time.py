"""Preparing the attack's node pairs: on the device (Attacker.prepare_test_data(pairs="device") / (rng="philox")) against the host
route they stand next to (numpy / scipy enumeration, the Python loop of construct_balanced_edge_sets, engine.group_pairs).

    python tools/sample_time.py [--out profiles/sample_time.json] [--runs 7] [--powerlaw-scale 17]

At twitch-RU shape (the ER graph of synth.twitch_like_problem("twitch-RU"): 4385 nodes, 37 304 edges):
  (i)  `unbalanced` samples of n_test = 500 and 2000: ``prepare_test_data`` plus the label / index build of the first ``evaluate``
       -- host: ``construct_edge_sets_from_random_subgraph`` + ``Attacker._metric_lists`` (with its upload); device: the same node
       draw + ``sampling.square_labels_device`` and the read-back of its four info words.  The device route is timed twice: with
       the graph's pattern uploaded anew for every preparation ("device_cold", what the gate reads) and with the upload kept
       ("device", what a second preparation on one Attacker costs).  The rows and ``engine.score_curve`` behind them are the same
       launches on both routes and are not timed here (tools/metrics_time.py).
  (ii) `balanced-full`: pair construction plus grouping -- host: ``construct_balanced_edge_sets`` (numpy's stream) +
       ``engine.group_pairs``; device: ``sampling.balanced_pairs_philox`` (upload and edge count included) +
       ``engine.group_pairs_device``.  The two streams give different non-edges: the work is the same, the pairs are not.
Optionally (ii) on a power-law graph of 2^scale nodes, device only (the host loop is not run there).
Both routes of a case run in ONE process, ALTERNATING, after a warm-up of both; per route the median, minimum and maximum over the
runs (host clock around work that ends in a device synchronisation).  gate = device median < host median - (host max - host min).
Needs a GPU; writes one JSON file."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import argparse, contextlib, io, json, time, types
import numpy as np, torch
from linkteller_amd import _lib, engine, sampling, synth
from linkteller_amd.attacker import Attacker


def quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn()


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(ts):
    return {"runs_ms": [round(t, 4) for t in ts], "median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4),
            "max_ms": round(max(ts), 4)}


def gate(row, host, device):
    h, d = row[host], row[device]
    row["gate"] = {"host_spread_ms": round(h["max_ms"] - h["min_ms"], 4), "host_minus_device_ms": round(h["median_ms"] - d["median_ms"], 4),
                   "passed": bool(d["median_ms"] < h["median_ms"] - (h["max_ms"] - h["min_ms"])),
                   "host_over_device": round(h["median_ms"] / d["median_ms"], 1)}


def attacker_for(adj, dev, sample_type, n_test):
    worker = types.SimpleNamespace(features_2=torch.zeros(adj.shape[0], 8, device=dev), adj_2=None, adj_ori=adj, n_nodes=adj.shape[0])
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type=sample_type, n_test=n_test, sample_seed=42, influence=1e-4,
                              mode="vanilla-clean", attack_mode="efficient", influence_mode="delta")
    return Attacker(args, None, worker)


def square_case(adj, dev, n_test, runs):
    atk = attacker_for(adj, dev, "unbalanced", n_test)

    def host():
        atk.prepare_test_data()
        atk._metric_lists(n_test, dev)

    def device(cold):
        if cold:
            atk._pattern_cache = None
        atk.prepare_test_data(pairs="device")
        _, _, info = atk._square_lists(n_test, dev)
        atk._square_n_edges(info)

    for _ in range(2):
        quiet(host)
        index_h, labels_h = atk._metric_lists(n_test, dev)
        quiet(lambda: device(True))
        index_d, labels_d, _ = atk._square_lists(n_test, dev)
    # the same items: host order is edges first, device order is the triangle's
    assert torch.equal(torch.sort(index_h * 2 + labels_h).values, torch.sort(index_d * 2 + labels_d).values)
    ts = {"host": [], "device_cold": [], "device": []}
    for _ in range(runs):
        ts["host"].append(clock(lambda: quiet(host)))
        ts["device_cold"].append(clock(lambda: quiet(lambda: device(True))))
        ts["device"].append(clock(lambda: quiet(lambda: device(False))))
    row = {"n_test": n_test, "pairs": n_test * (n_test - 1) // 2, "n_edges": int(labels_d.sum().item()),
           "index_upload_bytes_host": 9 * (n_test * (n_test - 1) // 2), **{k: stats(v) for k, v in ts.items()}}
    gate(row, "host", "device_cold")
    return row


def balanced_device(adj, n):
    csr = sampling.device_pattern_csr(adj)
    u, v, e, info = sampling.balanced_pairs_philox(csr, 42)
    groups = engine.group_pairs_device(u, v, n)
    return e, info, groups


def balanced_case(adj, runs, host=True):
    n = adj.shape[0]

    def host_route():
        np.random.seed(42)
        (ex, nex), _ = sampling.construct_balanced_edge_sets("twitch/ES/RU", "balanced-full", adj, n)
        return engine.group_pairs(np.concatenate([ex[:, 0], nex[:, 0]]), np.concatenate([ex[:, 1], nex[:, 1]]))

    e, info, _ = balanced_device(adj, n)
    ts = {"device": []} if not host else {"host": [], "device": []}
    if host:
        quiet(host_route)
    for _ in range(runs):
        if host:
            ts["host"].append(clock(lambda: quiet(host_route)))
        ts["device"].append(clock(lambda: balanced_device(adj, n)))
    row = {"n": n, "n_edges": int(e), "pairs": int(2 * e), "draws": int(info[1]), "rounds": int(info[2]), "self_pairs": int(info[3]),
           **{k: stats(v) for k, v in ts.items()}}
    if host:
        gate(row, "host", "device")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sample_time.json"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--n-test", type=int, nargs="+", default=[500, 2000])
    ap.add_argument("--powerlaw-scale", type=int, default=17, help="0: skip the power-law graph")
    a = ap.parse_args()
    if a.runs < 5:
        raise SystemExit("--runs: at least 5")
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    adj = synth.twitch_like_problem("twitch-RU", hidden=256, n_classes=2, seed=0)[0]
    res = {"device": torch.cuda.get_device_name(0), "shape": f"twitch-RU ER graph: {adj.shape[0]} nodes, {adj.nnz // 2} edges",
           "runs": a.runs}
    for n_test in a.n_test:
        row = res[f"unbalanced_n_test_{n_test}"] = square_case(adj, dev, n_test, a.runs)
        print(json.dumps(row))
    row = res["balanced_full"] = balanced_case(adj, a.runs)
    print(json.dumps(row))
    if a.powerlaw_scale:
        n = 1 << a.powerlaw_scale
        big = synth.powerlaw_graph(n, 8 * n, seed=1)
        row = res[f"balanced_full_powerlaw_2^{a.powerlaw_scale}"] = balanced_case(big, a.runs, host=False)
        row["max_row"] = int(np.diff(big.indptr).max())
        print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

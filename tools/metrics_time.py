"""Attack metrics: AUC / AP from the device (Attacker.evaluate) against the host route they replace (the float64 matrix landed on
the host, the pair look-ups and the three sklearn calls of compute_and_save).

    python tools/metrics_time.py [--out profiles/metrics_time.json] [--blocks 5] [--reps 10]

At twitch-RU shape (synth.twitch_like_problem("twitch-RU", hidden=256)), `unbalanced` samples of n_test = 500 and 2000 nodes,
mode `delta`:
  (a) ``Attacker.influence_matrix()``, the look-up of the n_test (n_test - 1) / 2 sampled pairs in it, ``metrics.roc_curve`` +
      ``metrics.auc``, ``metrics.precision_recall_curve`` and ``metrics.average_precision_score`` -- ``compute_and_save`` without
      its prints and its file;
  (b) ``Attacker.evaluate()``: the rows on the device, ``engine.score_curve`` through the cached index, eight words to the host.
Both in ONE process on one GPU, in ALTERNATING blocks after a warm-up of both; per route the median over the blocks' medians and
the spread between the blocks (host clock around work that ends in a device synchronisation).  (a)'s host part (everything behind
the matrix) is timed inside it as well.  (b)'s per-kernel split comes from the library's own launch brackets (lt_profile_*), in a
pass of its own.  (b) is checked once against (a): the curves of ``evaluate(curves=True)`` equal sklearn's arrays, AUC / AP agree
within 2 (D + 4) 2^-53.  Needs a GPU; writes one JSON file."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import argparse, contextlib, ctypes as C, io, json, time
import numpy as np, torch
from sklearn import metrics as skm
from linkteller_amd import _lib, synth
from recover_time import attacker_for, timed


def host_route(atk, cells, y):
    M = atk.influence_matrix()
    t = time.perf_counter()
    pred = list(M[cells])
    fpr, tpr, thr = skm.roc_curve(y, pred)
    auc = skm.auc(fpr, tpr)
    precision, recall, thr2 = skm.precision_recall_curve(y, pred)
    ap = skm.average_precision_score(y, pred)
    return (auc, ap, fpr, tpr, thr, precision, recall, thr2), (time.perf_counter() - t) * 1e3


def device_route(atk, curves=False):
    with contextlib.redirect_stdout(io.StringIO()):      # (evaluate prints its two lines)
        return atk.evaluate(curves=curves)


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
    ap.add_argument("--out", default=os.path.join("profiles", "metrics_time.json"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
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
        node2ind = np.full(int(nodes.max()) + 1, -1, dtype=np.int64)
        node2ind[nodes] = np.arange(len(nodes))
        pairs = np.concatenate([np.asarray(atk.exist_edges, dtype=np.int64).reshape(-1, 2),
                                np.asarray(atk.nonexist_edges, dtype=np.int64).reshape(-1, 2)])
        cells = (node2ind[pairs[:, 1]], node2ind[pairs[:, 0]])      # perturb v, observe u (attacker.py:236-245)
        y = [1] * len(atk.exist_edges) + [0] * len(atk.nonexist_edges)
        # warm-up of both routes, and (b) against (a)
        for _ in range(2):
            ref, _ms = host_route(atk, cells, y)
            got = device_route(atk, curves=True)
        c = got["curves"]
        for g_, r_ in ((c["auc"]["fpr"], ref[2]), (c["auc"]["tpr"], ref[3]), (c["auc"]["thresholds"], ref[4]),
                       (c["pr"]["precision"], ref[5]), (c["pr"]["recall"], ref[6]), (c["pr"]["thresholds"], ref[7])):
            assert np.array_equal(g_, r_), "the device curves differ from sklearn's"
        bound = 2 * (got["n_thresholds"] + 4) * 2.0 ** -53
        assert abs(got["auc"] - ref[0]) <= bound and abs(got["ap"] - ref[1]) <= bound
        blocks = {"device_metrics": [], "host_metrics": []}
        host_part = []
        for _ in range(a.blocks):
            blocks["device_metrics"].append(timed(lambda: device_route(atk), a.reps))
            blocks["host_metrics"].append(timed(lambda: host_part.append(host_route(atk, cells, y)[1]), a.reps))
        row = {"n_test": n_test, "pairs": len(y), "n_edges": int(len(atk.exist_edges)), "n_thresholds": got["n_thresholds"],
               "auc": got["auc"], "ap": got["ap"], "auc_minus_sklearn": got["auc"] - ref[0], "ap_minus_sklearn": got["ap"] - ref[1],
               "bytes_to_host_device_metrics": 64, "bytes_to_host_host_metrics": 8 * n_test * n_test, "curves_equal_sklearn": True}
        for k, t in blocks.items():
            row[k] = {"block_medians_ms": [round(s, 4) for s in t], "median_ms": round(float(np.median(t)), 4),
                      "spread_ms": round(max(t) - min(t), 4)}
        row["host_metrics"]["lookup_and_sklearn_part_median_ms"] = round(float(np.median(host_part)), 4)
        row["host_over_device"] = round(row["host_metrics"]["median_ms"] / row["device_metrics"]["median_ms"], 2)
        row["device_metrics"]["kernel_split"] = kernel_split(lambda: device_route(atk), a.reps)
        res[f"n_test_{n_test}"] = row
        print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

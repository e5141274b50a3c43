"""The baseline attacks (LSA2-post / LSA2-attr): scoring the pairs on the device (``args.baseline_scores = "device"``:
engine.corr_square / engine.corr_pairs) against the host route (the reference's fp32 torch arithmetic on the CPU).

    python tools/baseline_time.py [--out profiles/baseline_time.json] [--runs 7] [--warmup 2]

At twitch-RU shape (synth.twitch_like_problem("twitch-RU", hidden=256)): ``baseline-feat`` and ``baseline`` on `unbalanced`
samples of n_test = 500 and 2000 nodes, and both on `balanced-full`.  Per configuration, in ONE process on one GPU, ALTERNATING
after a warm-up of both:
  host    ``Attacker.baseline_attack()`` / ``baseline_attack_balanced()`` with the host route -- the attack method itself, with
          ``compute_and_save`` (sklearn and the file, identical on both routes) replaced by a no-op: the vectors to the host, the
          centring, the product, the pair look-ups;
  device  the same method with ``baseline_scores = "device"``: the vectors stay on the device, one call forms the scores, one copy
          brings them back, the same look-ups.
  evaluate  (device only, informational) ``Attacker.evaluate()``: scores and AUC / AP on the device, eight words to the host.
  library_call_device  (informational) the one library call alone -- all launches of lt_corr_square / lt_corr_pairs -- between two
          stream events, 20 calls.
Reported as median [min - max] over the runs (host clock around work that ends in a device synchronisation).  The device scores
are checked once against the host's: within the fp32 route's own error scale (1e-5).  Gate, at n_test = 2000 ``baseline-feat``: the
host median minus the device median exceeds the host runs' own max - min.  Needs a GPU; writes one JSON file."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import argparse, contextlib, io, json, time
import numpy as np, torch
from linkteller_amd import _lib, synth
from recover_time import attacker_for


def run(atk, route, method, keep):
    atk.args.baseline_scores = route
    atk.compute_and_save = lambda ex, nex, **kw: keep.__setitem__(route, (ex, nex))
    torch.cuda.synchronize()
    t = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        getattr(atk, method)()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def evaluate(atk):
    atk.args.baseline_scores = "device"
    torch.cuda.synchronize()
    t = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        out = atk.evaluate()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def library_call_ms(atk, st, reps=20):
    """Device time of the one library call (engine.corr_square / corr_pairs: all of its launches) between two stream events."""
    from linkteller_amd import engine
    atk.args.baseline_scores = "device"
    vec = atk._baseline_vectors_device()
    if st == "balanced-full":
        u, v, _ = atk._baseline_pair_lists(vec.device)
        call = lambda: engine.corr_pairs(vec, u, v)
    else:
        nodes = np.asarray(atk.test_nodes, dtype=np.int64)
        _, observed = atk._device_nodes(nodes, 0, len(nodes))
        call = lambda: engine.corr_square(vec, observed)
    call()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def stats(ts):
    return {"runs_ms": [round(t, 4) for t in ts], "median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4),
            "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "baseline_time.json"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-test", type=int, nargs="+", default=[500, 2000])
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "shape": "twitch-RU, hidden 256", "runs": a.runs, "warmup": a.warmup}
    adj, x, w = synth.twitch_like_problem("twitch-RU", hidden=256, n_classes=2, seed=0)
    configs = [("unbalanced", n) for n in a.n_test] + [("balanced-full", None)]
    gate = None
    for st, n_test in configs:
        atk = attacker_for(adj, x, w, dev, n_test or 100)
        if st == "balanced-full":
            atk.args.sample_type, atk.args.n_test = st, x.shape[0]
            with contextlib.redirect_stdout(io.StringIO()):
                atk.prepare_test_data()
        method = "baseline_attack_balanced" if st == "balanced-full" else "baseline_attack"
        for am in ("baseline-feat", "baseline"):
            atk.args.attack_mode = am
            keep = {}
            for _ in range(a.warmup):
                run(atk, "host", method, keep)
                run(atk, "device", method, keep)
            h = np.asarray(keep["host"][0] + keep["host"][1])
            d = np.asarray(keep["device"][0] + keep["device"][1])
            diff = float(np.nanmax(np.abs(h - d)))
            assert diff <= 1e-5, f"device scores differ from the host's by {diff}"
            ts = {"host": [], "device": [], "evaluate": []}
            for _ in range(a.runs):
                ts["host"].append(run(atk, "host", method, keep))
                ts["device"].append(run(atk, "device", method, keep))
                ms, ev = evaluate(atk)
                ts["evaluate"].append(ms)
            row = {"attack_mode": am, "sample_type": st, "n_test": n_test, "pairs": int(h.size), "columns": int(x.shape[1] if am == "baseline-feat" else 2),
                   "max_abs_device_minus_host": diff, "auc_device": ev["auc"], "ap_device": ev["ap"]}
            for k, t in ts.items():
                row[k] = stats(t)
            lib = stats(library_call_ms(atk, st))
            row["library_call_device"] = {k: lib[k] for k in ("median_ms", "min_ms", "max_ms")}
            row["host_minus_device_ms"] = round(row["host"]["median_ms"] - row["device"]["median_ms"], 4)
            row["host_spread_ms"] = round(row["host"]["max_ms"] - row["host"]["min_ms"], 4)
            row["host_over_device"] = round(row["host"]["median_ms"] / row["device"]["median_ms"], 2)
            res[f"{am}_{st}" + (f"_{n_test}" if n_test else "")] = row
            print(json.dumps(row))
            if am == "baseline-feat" and n_test == 2000:
                gate = row
    if gate is not None:
        res["gate"] = {"host_minus_device_ms": gate["host_minus_device_ms"], "host_spread_ms": gate["host_spread_ms"],
                       "passed": bool(gate["host_minus_device_ms"] > gate["host_spread_ms"])}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)
    if gate is not None:
        assert res["gate"]["passed"], f"gate: host - device = {gate['host_minus_device_ms']} ms within the host's spread {gate['host_spread_ms']} ms"


if __name__ == "__main__":
    main()

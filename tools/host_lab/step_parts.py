"""Where the serial host time of a host-landed headline step goes (twitch-RU as bench.py builds it, `delta`, 500 x 500, every step
behind a refresh).  Needs a library built with -DLT_HOST_LAB (make CXXEXTRA=-DLT_HOST_LAB): every host-landed call then records
six CLOCK_MONOTONIC stamps -- entry, first launch returned, last launch returned, zero-fill done, wait returned, matrix placed --
and this tool puts time.perf_counter_ns (the same clock) around the Python call.  Two step forms, each timed in alternating blocks:
  calls  refresh(mode), lt_influence_matrix_host, lt_node_check -- the separate library calls the step was before lt_influence_step_host
  step   Baseline.influence_matrix_host as it is (one lt_influence_step_host call)
Printed: medians over the blocks of the per-block medians, in us.  "launch..wait" is first launch returned -> wait returned: GPU span
+ launch latency + completion latency (take the GPU span from a kernel trace of its own, tools/host_lab/trace_medians.py).
--steps-only K --form calls|step: K steps of one form and nothing else (what a kernel trace is taken of).
A call that places its values by look ("host_poll" = 1, the default) also stamps: ready word seen, first value seen, last value
seen, and reports the stall time its budget saw; "wait returned" is then the moment the run was consumed -- unless LT_HOST_LAB_WAIT=1
is set, which makes the lab build still call the stream wait behind the last value: "(a) last value..wait" is then what the
product path saves outright.  --host-poll 0 measures the late form.
python tools/host_lab/step_parts.py --lib PATH [--blocks 10] [--steps 50] [--host-poll 0|1]"""
import argparse, ctypes, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from linkteller_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=10)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--steps-only", type=int, default=0)
ap.add_argument("--form", default="step", choices=["calls", "step"])
ap.add_argument("--lib", default=None)
ap.add_argument("--host-poll", type=int, default=None, choices=[0, 1])
a = ap.parse_args()
if a.lib:
    _lib.LIB_PATH = os.path.abspath(a.lib)
from linkteller_amd import engine, graph, synth

dev = torch.device("cuda:0")
if a.host_poll is not None:
    _lib.set_tuning("host_poll", a.host_poll)
adj, x_np, w = synth.twitch_like_problem("twitch-RU", hidden=256, n_classes=2, seed=0)
n = adj.shape[0]
base = engine.Baseline(graph.HipGraph(graph.first_order_gcn(adj)), torch.from_numpy(x_np).to(dev),
                       *[torch.from_numpy(w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")])
base.enable_fp64()
np.random.seed(42)
nodes = torch.from_numpy(np.random.choice(np.arange(n), 500, replace=False).astype(np.int32)).to(dev)


def step_calls():
    probes = engine._as_nodes(nodes, base.n, dev, "probe_nodes")
    obs = engine._as_nodes(nodes, base.n, dev, "observe_nodes")
    npb, nob = probes.numel(), obs.numel()
    host = torch.empty((npb, nob), dtype=torch.float64, pin_memory=True)
    key = ("scratch", npb, nob)
    out = base._host_scratch.get(key)
    if out is None:
        out = torch.empty((npb, nob), dtype=torch.float32, device=dev)
        base._host_scratch = {key: out}
    base.refresh("delta")
    base.influence_rows(probes, obs, 1e-4, "delta", out=out, host=host, wait=True)
    engine.node_check()
    return host.numpy()


def step_one():
    return base.influence_matrix_host(nodes, nodes, 1e-4, "delta", refresh=True)


forms = {"calls": step_calls, "step": step_one}
if a.steps_only:
    fn = forms[a.form]
    t = time.perf_counter()
    for _ in range(a.steps_only):
        fn()
    print(f"{a.form}: {a.steps_only} steps, {(time.perf_counter() - t) / a.steps_only * 1e3:.4f} ms/step")
    sys.exit(0)

handle = _lib.lib()
if not hasattr(handle, "lt_host_lab_stamps"):
    sys.exit("the library was not built with -DLT_HOST_LAB")
read_stamps = handle.lt_host_lab_stamps10 if hasattr(handle, "lt_host_lab_stamps10") else handle.lt_host_lab_stamps
read_stamps.restype = None
read_stamps.argtypes = [ctypes.POINTER(ctypes.c_int64)]
stamps = (ctypes.c_int64 * 10)()
COLS = ("step", "python before", "library before 1st launch", "launches", "zero-fill", "launch..wait", "wait after zero-fill",
        "placing + node check", "python after", "between calls",
        "1st launch..ready word", "1st launch..first value", "1st launch..last value", "(b) first..last value",
        "(a) last value..wait", "(c) stall seen by the budget")

ref = step_calls().copy()
for fn in forms.values():
    for _ in range(20):
        assert np.array_equal(fn(), ref), "the two forms differ"
res = {k: [] for k in forms}
for blk in range(a.blocks):
    for name in (("calls", "step") if blk % 2 == 0 else ("step", "calls")):
        fn = forms[name]
        fn()
        rows, t_prev = [], None
        for _ in range(a.steps):
            t0 = time.perf_counter_ns()
            fn()
            t1 = time.perf_counter_ns()
            read_stamps(stamps)
            s = list(stamps)
            polled = s[6] >= s[0] and s[8] >= s[6]      # (this call's: a call in the late form leaves an earlier call's stamps)
            rows.append((t1 - t0, s[0] - t0, s[1] - s[0], s[2] - s[1], s[3] - s[2], s[4] - s[1], s[4] - s[3], s[5] - s[4], t1 - s[5],
                         0 if t_prev is None else t0 - t_prev)
                        + ((s[6] - s[1], s[7] - s[1], s[8] - s[1], s[8] - s[7], s[4] - s[8], s[9]) if polled else (np.nan,) * 6))
            t_prev = time.perf_counter_ns()
        res[name].append(np.nanmedian(np.array(rows, dtype=np.float64), axis=0) / 1e3)
for name in forms:
    m = np.median(np.array(res[name]), axis=0)
    lo, hi = np.min(np.array(res[name]), axis=0), np.max(np.array(res[name]), axis=0)
    print(f"{name}: medians of {a.blocks} blocks of {a.steps} steps, us (min .. max of the blocks)")
    for c, v, l, h in zip(COLS, m, lo, hi):
        print(f"    {c:28s} {v:7.2f}  ({l:.2f} .. {h:.2f})")

"""The cases of test_mlp_gpu.py's one-step check and their CPU-side analysis (mlp_restate.step_reference in fp64 and fp32, the
near-kink columns).  Inputs are drawn here, on the CPU, so that the fp64 reference itself stays inside the near-kink cap."""
import numpy as np

import mlp_restate as M
import train_restate as T

LR, DECAY, SEED = 0.01, 5e-4, 0x5EED0123456789

# name: n, F, H (0: depth 1), C, batch size, loss, p, checked steps
CASES = {
    "A": dict(n=700, F=300, H=256, C=8, B=256, loss="ce", p=0.0, steps=(0, 2, 3)),     # crosses an epoch; last batch 188
    "B": dict(n=513, F=40, H=32, C=3, B=256, loss="ce", p=0.0, steps=(2,)),            # a last batch of one row
    "C": dict(n=100, F=40, H=32, C=3, B=256, loss="ce", p=0.0, steps=(0,)),            # a single short batch
    "D": dict(n=150, F=301, H=30, C=3, B=37, loss="ce", p=0.5, steps=(0, 4, 5)),       # F % 4 = 1, H % 4 = 2, per-element Philox
    "E": dict(n=300, F=50, H=64, C=41, B=128, loss="ce", p=0.0, steps=(0, 2)),         # wide single-label head
    "F": dict(n=300, F=50, H=64, C=121, B=128, loss="bce", p=0.0, steps=(0, 2)),       # wide multi-label head
    "G": dict(n=300, F=50, H=0, C=2, B=128, loss="ce", p=0.0, steps=(0, 2)),           # depth 1
    "H": dict(n=300, F=50, H=0, C=121, B=128, loss="bce", p=0.0, steps=(0, 2)),        # depth 1, multi-label
    "I": dict(n=150, F=40, H=32, C=3, B=64, loss="ce", p=1.0, steps=(0, 2)),           # nothing is kept
    "K": dict(n=130, F=1100, H=20, C=2, B=64, loss="ce", p=0.25, steps=(0, 2)),        # three forward slabs, the last one partial
}
CASE_STEPS = [(k, s) for k, c in CASES.items() for s in c["steps"]]


def names(depth):
    return ("dW1", "db1", "dW2", "db2") if depth == 2 else ("dW", "db")


def make(name):
    c = dict(CASES[name], name=name)
    n, f, h, k = c["n"], c["F"], c["H"], c["C"]
    rng = np.random.RandomState(sum(map(ord, name)) + 1000)
    x = (rng.standard_normal((n, f)) * (rng.random_sample((n, f)) < 0.3)).astype(np.float32)
    c["depth"] = 2 if h else 1
    dims = [f, h, k] if h else [f, k]
    params = []
    for a, b in zip(dims[:-1], dims[1:]):
        s = 1.0 / np.sqrt(a)
        params += [rng.uniform(-s, s, (a, b)).astype(np.float32), rng.uniform(-s, s, b).astype(np.float32)]
    c["x"], c["params"] = x, params
    r = rng.standard_normal((f, k)).astype(np.float32)
    score = x @ r
    c["y"] = (score > np.median(score, axis=0)).astype(np.uint8) if c["loss"] == "bce" else score.argmax(axis=1).astype(np.int64)
    spe = -(-n // c["B"])
    c["spe"] = spe
    epochs = max(c["steps"]) // spe + 1
    c["orders"] = np.stack([np.random.RandomState(7 + e).permutation(n) for e in range(epochs)]).astype(np.int64)
    return c


def batch_of(case, step):
    e, k = divmod(step, case["spe"])
    return M.batches(case["orders"][e], case["B"])[k]


def gate(err32, ref64):
    return 2.0 * float(err32) + 1e-6 * float(np.abs(ref64).max()) + 1e-12


def analyse(case, start, step, mask_step=None):
    """The checked step at the read-back parameters ``start``: the fp64 and fp32 references under the step's mask, the hidden
    columns with near-kink elements, and the fp64 gradients with those elements' derivatives all off / all on."""
    rows = batch_of(case, step)
    p, h = case["p"], case["H"]
    keep, scale = None, 1.0
    if case["depth"] == 2 and p > 0:
        keep = M.step_keep(rows.size, h, step if mask_step is None else mask_step, SEED, p)
        scale = T.dropout_scale(p)
    args = (case["x"], case["y"], start, rows, case["depth"], case["loss"], keep, scale)
    r64, r32 = M.step_reference(*args, dtype=np.float64), M.step_reference(*args, dtype=np.float32)
    an = dict(rows=rows, r64=r64, r32=r32, kink_cols=np.zeros(max(h, 1), dtype=bool)[:h], fragile=0)
    if case["depth"] == 2:
        kmask = np.ones((rows.size, h), dtype=bool) if keep is None else keep
        tau, near = T.near_kink(r64["Z1"], r32["Z1"], kmask)
        an["kink_cols"] = near.any(axis=0)
        if near.any():
            on = r64["Z1"] > 0
            an["off"] = M.step_reference(*args, dtype=np.float64, relu_on=on & ~near)["grads"]
            an["on"] = M.step_reference(*args, dtype=np.float64, relu_on=on | near)["grads"]
    an["fragile"] = int((r64["margin"] < 1e-4).sum()) if case["loss"] == "ce" else \
        int(((np.abs(r64["Z"]) < 1e-4) & (case["y"][rows] != 0)).sum())
    return an


def check_conditions(case, an):
    """What the inputs were chosen for: near-kink columns are at most 1/8 of H."""
    if case["depth"] == 2:
        assert int(an["kink_cols"].sum()) <= case["H"] // 8, (case["name"], int(an["kink_cols"].sum()))

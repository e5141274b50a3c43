"""The cases of test_train_backward_gpu.py and what they are compared with: every case is a graph, features, labels, initial
parameters and a dropout rate; `analyse` evaluates train_restate.epoch_reference at given parameters in fp64 and fp32 and
names the near-kink elements.  test_train_cpu.py checks the reference and the cases' conditions without a GPU."""
import numpy as np
import scipy.sparse as sp

import train_restate as T

SEED = (5 << 32) | 1234        # both words of the Philox key are in use
LR, DECAY = 0.01, 5e-4
NAMES = ("dW1", "db1", "dW2", "db2")

#        n, F, H, C, p, epochs checked
SHAPES = {
    "A": (700, 300, 256, 8, 0.5, (0, 3)),
    "B": (1100, 301, 30, 3, 0.3, (0, 2)),
    "C": (300, 160, 16, 1, 0.5, (0,)),
    "D": (513, 64, 100, 7, 0.0, (0,)),
    "E": (1100, 301, 30, 3, 1.0, (0,)),
    "F": (17, 5, 4, 2, 0.5, (0,)),
    "T": (4648, 3170, 256, 2, 0.5, (0,)),
}
CASE_EPOCHS = [(k, e) for k, s in SHAPES.items() for e in s[5]]


def _f32(adj):
    a = sp.csr_matrix(adj).astype(np.float32)      # the values the device holds (graph.csr_arrays)
    a.sum_duplicates()
    a.sort_indices()
    return a


def directed_graph(n, seed):
    """A directed weighted pattern, about 8 entries per row with values in (0, 1), not symmetric; every 9th row is empty and
    every 11th column (offset 3) is empty, so the CSC differs from the CSR in pattern, values and empty lines."""
    rng = np.random.RandomState(seed)
    m = 8 * n
    r, c = rng.randint(0, n, m), rng.randint(0, n, m)
    ok = (r % 9 != 0) & (c % 11 != 3)
    a = sp.csr_matrix((np.ones(int(ok.sum())), (r[ok], c[ok])), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    a.data = rng.uniform(0.05, 0.95, a.nnz)
    return a


def make(name):
    """dict(adj (float32 CSR), x, y, params (W1, b1, W2, b2 as float32 arrays), p, n, F, H, C) of one case; seeds fixed."""
    from linkteller_amd import graph, synth
    n, f, h, c, p, _ = SHAPES[name]
    if name == "T":
        from test_train_gpu import _twitch_shape
        adj, x, y = _twitch_shape()
        w = synth.gcn_weights(f, h, c, seed=5)
    else:
        if name == "A":
            adj = graph.aug_random_walk(synth.powerlaw_graph(n, 6 * n, seed=0))
            x = synth.twitch_like_features(n, f, seed=0, density=0.05)
        elif name == "D":
            adj = directed_graph(n, 0)
            x = synth.gaussian_features(n, f, seed=0)
        else:
            adj = graph.first_order_gcn(synth.erdos_renyi_graph(n, 5 * n if n > 100 else 30, seed=0))
            x = synth.gaussian_features(n, f, seed=0)
        y = np.random.RandomState(1).randint(0, c, n).astype(np.int64)
        w = synth.gcn_weights(f, h, c, seed=0)
    assert x.shape == (n, f)
    return dict(name=name, adj=_f32(adj), x=x, y=y, params=[w[k] for k in ("W1", "b1", "W2", "b2")], p=p, n=n, F=f, H=h, C=c)


def analyse(case, params, epoch, mask_epoch=None):
    """The references of one epoch at ``params``: r64 / r32 (epoch_reference in fp64 / fp32 with that epoch's dropout mask),
    tau and the near-kink elements, the hidden columns that hold one, and for those the fp64 gradients with every near-kink
    derivative off / on.  ``mask_epoch`` substitutes another epoch's mask (the epoch-word check)."""
    p = case["p"]
    keep = T.dropout_keep(case["n"], case["H"], epoch if mask_epoch is None else mask_epoch, SEED, p)
    scale = T.dropout_scale(p)
    args = (case["adj"], case["x"], case["y"], params, keep, scale)
    r64 = T.epoch_reference(*args, np.float64)
    r32 = T.epoch_reference(*args, np.float32)
    tau, near = T.near_kink(r64["Z1"], r32["Z1"], keep)
    out = dict(r64=r64, r32=r32, keep=keep, tau=tau, near=near, kink_cols=near.any(axis=0),
               flipped32=int(((r32["Z1"] > 0) != (r64["Z1"] > 0))[keep].sum()), fragile=T.fragile_rows(r64["Z2"]))
    if near.any():
        on64 = r64["Z1"] > 0
        out["off"] = T.epoch_reference(*args, np.float64, relu_on=on64 & ~near)
        out["on"] = T.epoch_reference(*args, np.float64, relu_on=on64 | near)
    return out


def gate(e32, ref64):
    """The project's fp32 gate (test_first_epoch_gradients_against_fp64): twice the fp32 reference's own error."""
    return 2.0 * float(e32) + 1e-6 * float(np.abs(ref64).max()) + 1e-12


def check_conditions(case, an):
    """The two conditions a case must meet for its comparison to be meaningful: the hidden columns with near-kink elements
    are at most 1/8 of H, and the rows with a fragile argmax at most 1 % of n."""
    n_cols = int(an["kink_cols"].sum())
    print(f"case {case['name']}: tau {an['tau']:.3e}, {int(an['near'].sum())} near-kink elements in {n_cols} of {case['H']} "
          f"columns, fp32 reference flipped {an['flipped32']}, fragile rows {an['fragile']} of {case['n']}")
    assert 8 * n_cols <= case["H"], (case["name"], n_cols, case["H"])
    assert 100 * an["fragile"] <= case["n"], (case["name"], an["fragile"], case["n"])

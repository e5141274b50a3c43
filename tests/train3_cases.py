"""The cases of test_train3_backward_gpu.py and what they are compared with: a graph, features, labels, six initial
parameters and a dropout rate each; ``analyse`` evaluates train3_restate.epoch_reference3 at given parameters in fp64 and fp32
with an epoch's two masks and names the near-kink elements of both hidden layers.  test_train3_cpu.py pins the cases'
conditions without a GPU."""
import numpy as np

import train_cases as K
import train_restate as T
import train3_restate as T3

SEED, LR, DECAY = K.SEED, K.LR, K.DECAY
NAMES = T3.NAMES3

#        n, F, H1, H2, C, p, epochs checked
SHAPES = {
    "A3": (700, 300, 256, 64, 8, 0.5, (0, 3)),
    "B3": (1100, 301, 30, 18, 3, 0.3, (0, 2)),
    "D3": (513, 64, 100, 256, 7, 0.0, (0,)),
    "G3": (600, 130, 64, 200, 2, 0.5, (0,)),
    "E3": (1100, 301, 30, 18, 3, 1.0, (0,)),
    "C3": (300, 160, 16, 12, 1, 0.5, (0,)),
    "F3": (17, 5, 4, 3, 2, 0.5, (0,)),
}
CASE_EPOCHS = [(k, e) for k, s in SHAPES.items() for e in s[6]]


def init_params(f, h1, h2, c, seed=0):
    """W1, b1, W2, b2, W3, b3 from one RandomState(seed), each U(-1/sqrt(out), 1/sqrt(out)) as float32."""
    rng = np.random.RandomState(seed)
    out = []
    for fan_in, fan_out in ((f, h1), (h1, h2), (h2, c)):
        bound = 1.0 / np.sqrt(fan_out)
        out.append(rng.uniform(-bound, bound, (fan_in, fan_out)).astype(np.float32))
        out.append(rng.uniform(-bound, bound, fan_out).astype(np.float32))
    return out


def make(name, h2=None):
    """dict(adj (float32 CSR), x, y, params (six float32 arrays), p, n, F, H1, H2, C) of one case; seeds fixed.  ``h2``
    overrides the second hidden width (B3 with H2 = H1 = 30: the layer-word check)."""
    from linkteller_amd import graph, synth
    n, f, h1, h2_, c, p, _ = SHAPES[name]
    h2 = h2_ if h2 is None else h2
    if name == "A3":
        adj = graph.aug_random_walk(synth.powerlaw_graph(n, 6 * n, seed=0))
        x = synth.twitch_like_features(n, f, seed=0, density=0.05)
    elif name == "D3":
        adj = K.directed_graph(n, 0)
        x = synth.gaussian_features(n, f, seed=0)
    else:
        adj = graph.first_order_gcn(synth.erdos_renyi_graph(n, 5 * n if n > 100 else 30, seed=0))
        x = synth.gaussian_features(n, f, seed=0)
    y = np.random.RandomState(1).randint(0, c, n).astype(np.int64)
    assert x.shape == (n, f)
    return dict(name=name, adj=K._f32(adj), x=x, y=y, params=init_params(f, h1, h2, c), p=p, n=n, F=f, H1=h1, H2=h2, C=c)


def masks(case, epoch, swap=False):
    """(keep1, keep2) of one epoch; ``swap`` exchanges the two layer words (needs H1 = H2)."""
    k1 = T3.dropout_keep3(case["n"], case["H1"], epoch, SEED, case["p"], 1 if swap else 0)
    k2 = T3.dropout_keep3(case["n"], case["H2"], epoch, SEED, case["p"], 0 if swap else 1)
    return k1, k2


def analyse(case, params, epoch, mask_epoch=None, swap=False):
    """r64 / r32 (epoch_reference3 in fp64 / fp32 with that epoch's two masks), per hidden layer tau and the near-kink
    elements, and the number of rows with a fragile argmax.  ``mask_epoch`` substitutes another epoch's masks, ``swap`` the
    other layer's."""
    keep1, keep2 = masks(case, epoch if mask_epoch is None else mask_epoch, swap)
    scale = T.dropout_scale(case["p"])
    args = (case["adj"], case["x"], case["y"], params, keep1, keep2, scale)
    r64 = T3.epoch_reference3(*args, np.float64)
    r32 = T3.epoch_reference3(*args, np.float32)
    tau1, near1 = T.near_kink(r64["Z1"], r32["Z1"], keep1)
    tau2, near2 = T.near_kink(r64["Z2"], r32["Z2"], keep2)
    return dict(r64=r64, r32=r32, keep=(keep1, keep2), scale=scale, args=args, tau=(tau1, tau2), near=(near1, near2),
                fragile=T.fragile_rows(r64["Z3"]))


def check_conditions(case, an):
    """The conditions a case must meet for its comparison to be meaningful: per hidden layer the near-kink elements are at
    most 0.1 % of the kept elements, and no row has a fragile argmax."""
    for k in (0, 1):
        near, kept = int(an["near"][k].sum()), int(an["keep"][k].sum())
        print(f"case {case['name']} layer {k + 1}: tau {an['tau'][k]:.3e}, {near} near-kink of {kept} kept elements")
        assert 1000 * near <= kept, (case["name"], k, near, kept)
    print(f"case {case['name']}: fragile rows {an['fragile']} of {case['n']}")
    assert an["fragile"] == 0, (case["name"], an["fragile"])

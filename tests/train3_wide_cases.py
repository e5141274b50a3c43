"""The cases of test_train3_wide_gpu.py and what they are compared with (train3_wide_restate.epoch_reference3_wide in fp64 and
fp32), and the conditions a case must meet for its comparison to be meaningful.  test_train3_wide_cpu.py asserts the conditions
without a GPU, at the initial parameters and after two Adam steps simulated on the CPU; the GPU tests assert them again at the
parameters they read back.

Multi-label cases draw b3 with magnitudes in [1, 3] and random signs, as train_wide_cases.init_params does for b2.  The seed
of a case is the first of 0, 1, 2, ... at which the restatement alone meets every condition at epoch 0 and at epoch 2
(``find_seed``; ``python tests/train3_wide_cases.py`` prints the search)."""
import numpy as np

import train_cases as K
import train_restate as T
import train_wide_cases as KW
import train_wide_restate as TW
import train3_cases as K3
import train3_wide_restate as TW3

SEED = K.SEED
LR, DECAY = K.LR, K.DECAY
NAMES = TW3.NAMES

#         n,   F,  H1,  H2,  C, loss,  p
SHAPES = {
    "T9": (300, 37, 30, 18, 9, "ce", 0.5),
    "T41": (513, 64, 64, 100, 41, "ce", 0.5),
    "T65": (300, 33, 16, 12, 65, "bce", 0.5),
    "T121": (700, 50, 256, 64, 121, "bce", 0.5),
    "T256": (130, 20, 8, 5, 256, "ce", 0.0),
    "T1": (17, 5, 4, 3, 1, "bce", 0.0),
    "P1": (300, 37, 30, 18, 9, "ce", 1.0),
}
# seed per case: graph, features, labels and parameters all derive from it (found by find_seed on the CPU; T256: seed 0 has one
# near-kink element among the 650 of the second hidden layer, above 0.1 %)
SEEDS = {"T9": 0, "T41": 0, "T65": 0, "T121": 0, "T256": 1, "T1": 0, "P1": 0}
EPOCHS = (0, 2)
CASE_EPOCHS = [(k, e) for k in SHAPES for e in EPOCHS]


def init_params(f, h1, h2, c, loss, seed):
    params = K3.init_params(f, h1, h2, c, seed=seed)
    if loss == "bce":
        rng = np.random.RandomState(seed + 77)
        params[5] = (rng.uniform(1.0, 3.0, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    return params


def make(name, seed=None, h2=None):
    """dict(adj (float32 CSR), x, y, params (six float32 arrays), p, n, F, H1, H2, C, loss) of one case.  ``h2`` overrides the
    second hidden width (T9 with H2 = H1 = 30: the layer-word check)."""
    from linkteller_amd import graph, synth
    n, f, h1, h2_, c, loss, p = SHAPES[name]
    h2 = h2_ if h2 is None else h2
    seed = SEEDS[name] if seed is None else seed
    if name == "T41":
        adj = K.directed_graph(n, seed)
    elif name == "T121":
        adj = graph.aug_random_walk(synth.powerlaw_graph(n, 6 * n, seed=seed))
    else:
        adj = graph.first_order_gcn(synth.erdos_renyi_graph(n, 5 * n if n > 100 else 30, seed=seed))
    x = synth.gaussian_features(n, f, seed=seed)
    return dict(name=name, adj=K._f32(adj), x=x, y=KW.labels_for(n, c, loss, seed), params=init_params(f, h1, h2, c, loss, seed),
                p=p, n=n, F=f, H1=h1, H2=h2, C=c, loss=loss)


def masks(case, epoch, swap=False):
    """(keep1, keep2) of one epoch: the layer words 0 and 1; ``swap`` exchanges them (needs H1 = H2)."""
    return K3.masks(case, epoch, swap)


def analyse(case, params, epoch, swap=False):
    """r64 / r32 at ``params`` with that epoch's two masks, per hidden layer tau and the near-kink elements, the rows with a
    fragile argmax (ce) or the elements with a fragile sign (bce)."""
    keep1, keep2 = masks(case, epoch, swap)
    scale = T.dropout_scale(case["p"])
    args = (case["adj"], case["x"], case["y"], params, keep1, keep2, scale, case["loss"])
    r64 = TW3.epoch_reference3_wide(*args, np.float64)
    r32 = TW3.epoch_reference3_wide(*args, np.float32)
    tau1, near1 = T.near_kink(r64["Z1"], r32["Z1"], keep1)
    tau2, near2 = T.near_kink(r64["Z2"], r32["Z2"], keep2)
    fragile = TW.ce_margin_rows(r64["Z3"]) if case["loss"] == "ce" else TW.bce_small_logits(r64["Z3"])
    return dict(r64=r64, r32=r32, keep=(keep1, keep2), scale=scale, args=args, tau=(tau1, tau2), near=(near1, near2),
                fragile=fragile)


def check_conditions(case, an):
    """Per hidden layer the near-kink kept elements are at most 0.1 % of the kept ones; no row with an fp64 argmax margin below
    1e-4 (ce); no element with an fp64 logit magnitude below 1e-4 (bce)."""
    for k in (0, 1):
        near, kept = int(an["near"][k].sum()), int(an["keep"][k].sum())
        print(f"case {case['name']} layer {k + 1}: tau {an['tau'][k]:.3e}, {near} near-kink of {kept} kept elements")
        assert 1000 * near <= kept, (case["name"], k, near, kept)
    print(f"case {case['name']}: fragile {an['fragile']}")
    assert an["fragile"] == 0, (case["name"], an["fragile"])


def simulate(case, steps):
    """The parameters after ``steps`` epochs on the CPU: the fp64 restatement's gradients, rounded to float32, through
    train_restate.adam_step."""
    params = [p.copy() for p in case["params"]]
    m = [np.zeros_like(p) for p in params]
    v = [np.zeros_like(p) for p in params]
    for e in range(steps):
        keep1, keep2 = masks(case, e)
        r = TW3.epoch_reference3_wide(case["adj"], case["x"], case["y"], params, keep1, keep2, T.dropout_scale(case["p"]),
                                      case["loss"], np.float64)
        for k, name in enumerate(NAMES):
            params[k], m[k], v[k] = T.adam_step(params[k], r[name].astype(np.float32), m[k], v[k], e + 1, LR, weight_decay=DECAY)
    return params


def conditions_hold(case):
    """check_conditions at epoch 0 and, at the simulated parameters, at epoch 2."""
    for epoch in EPOCHS:
        check_conditions(case, analyse(case, simulate(case, epoch), epoch))


def find_seed(name, limit=20):
    for seed in range(limit):
        try:
            conditions_hold(make(name, seed))
        except AssertionError as exc:
            print(f"{name}: seed {seed} refused: {exc}")
            continue
        return seed
    raise RuntimeError(f"{name}: no seed below {limit} meets the conditions")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print({name: find_seed(name) for name in SHAPES})

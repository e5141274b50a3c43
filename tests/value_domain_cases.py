"""Inputs of the value-domain tests (test_value_domain_cpu.py, test_value_domain_gpu.py): six small models, one per route of
`delta`, and the exact transformations that move their hidden units and feature columns apart in scale.  numpy / scipy only.

A hidden unit j of a ReLU network may be rescaled by any s > 0 -- W1[:, j] * s, b1[j] * s, W2[j, :] / s -- and a feature column j
likewise -- X[:, j] * s, W1[j, :] / s -- without changing the function.  With s = 2^k no ROUNDING changes either: every
floating-point evaluation of the model gives the same bits (test_value_domain_cpu.py asserts it of the oracle), so one oracle run
per base case serves the whole ladder of k.  What does change is every quantity stored as fixed point against a local maximum
(value_domain_model.py): the units scaled down lose 2^-k of their resolution."""
import functools

import numpy as np

from linkteller_amd import graph, synth

DELTA = 1e-4
LADDER = (1, -1, 2, -2, 4, -4, 8, -8, 12, -12, 16, -16, 20, -20)
EXACT_KS = (-20, -8, 8, 20)
MAX_PROBES, MAX_OBS = 12, 150

# case -> (graph generator, n, edges, features, F, layer widths): the shapes of the issue's table, not to be grown
SHAPES = {
    "M": ("er", 700, 4200, "gaussian", 300, (64, 2)),          # route 0: the dense product (int8 split / f64 matrix cores)
    "Q": ("er", 700, 4200, "gaussian", 256, (64, 2)),          # route 0 with ONE K slice of the int8 split: the rows leave through k_quant_rows_f64
    "R": ("powerlaw", 600, 3000, "twitch", 304, (64, 3)),      # route 1: feature rows as differences to a reference row
    "A": ("powerlaw", 600, 3000, "gaussian", 40, (64, 2)),     # route 2: aggregate-first
    "G": ("powerlaw", 600, 3000, "gaussian", 40, (32, 16, 2)),  # Baseline3
    "W": ("er", 600, 3600, "gaussian", 300, (320, 12)),        # WideBaseline: hidden slices 256 + 64, class slices 8 + 4
}
# the weights' seeds: 7 as in the existing kink test; Q and G moved (from 7: 2.4e-6 and 3.3e-6 / 5.6e-6) until the storage model puts
# their kink rows at k = 0 inside the domain with room to spare (1.4e-6 and 1.1e-6 / 1.2e-6), as the reference cells must be
WEIGHT_SEED = {"M": 7, "Q": 8, "R": 7, "A": 7, "G": 13, "W": 7}
ROUTE = {"M": 0, "Q": 0, "R": 1, "A": 2}
# the knob sets a case's default-storage run is repeated under
KNOBS = {
    "M": [dict(aggregate_first=0, i8_split=i8, delta_fused=fu) for i8 in (1, 0) for fu in (1, 0)],
    "Q": [dict(aggregate_first=0)],
    "R": [dict(feature_lists=1), dict(feature_lists=0)],
    "A": [dict()], "G": [dict()], "W": [dict()],
}
# the fp64-storage form of a case: no fixed-point rows, no int8 split
FP64_KNOBS = {"M": dict(aggregate_first=0, s1_f32=0, i8_split=0), "Q": dict(aggregate_first=0, s1_f32=0, i8_split=0), "R": dict(s1_f32=0), "A": dict(s1_f32=0), "G": dict(s1_f32=0),
              "W": dict(s1_f32=0)}
WEIGHT_KEYS = {2: ("W1", "b1", "W2", "b2"), 3: ("W1", "b1", "W2", "b2", "W3", "b3")}


def knob_id(kn):
    return "-".join(f"{k}{v}" for k, v in kn.items()) or "default"


def _uniform(rng, shape, fan_out):
    s = 1.0 / np.sqrt(fan_out)
    return rng.uniform(-s, s, size=shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def base(case):
    """dict(a_hat, x, w, r0, probes, obs, depth) of a case; the arrays are shared: copy before writing."""
    gen, n, edges, feats, f, widths = SHAPES[case]
    adj = (synth.erdos_renyi_graph if gen == "er" else synth.powerlaw_graph)(n, edges, seed=3)
    a_hat = graph.first_order_gcn(adj).tocsr()
    a_hat.sort_indices()
    x = synth.gaussian_features(n, f, seed=2) if feats == "gaussian" else synth.twitch_like_features(n, f, seed=2, density=0.02)
    if len(widths) == 2:
        w = dict(synth.gcn_weights(f, widths[0], widths[1], seed=WEIGHT_SEED[case]))
    else:
        rng = np.random.RandomState(WEIGHT_SEED[case])
        h1, h2, c = widths
        w = dict(W1=_uniform(rng, (f, h1), h1), b1=_uniform(rng, (h1,), h1), W2=_uniform(rng, (h1, h2), h2),
                 b2=_uniform(rng, (h2,), h2), W3=_uniform(rng, (h2, c), c), b3=_uniform(rng, (c,), c))
    # a median-degree row, its neighbours as probes, they and their neighbours as observed nodes (the existing kink test's lists)
    deg = np.diff(a_hat.indptr)
    r0 = int(np.argsort(deg, kind="stable")[len(deg) // 2])
    nb = a_hat[r0].indices
    probes = np.concatenate([[r0], nb[nb != r0]])[:MAX_PROBES]
    second = np.unique(np.concatenate([a_hat[int(v)].indices for v in nb]))
    obs = np.concatenate([nb, second[~np.isin(second, nb)]])[:MAX_OBS]
    return dict(a_hat=a_hat, x=x, w=w, r0=r0, probes=np.sort(probes).astype(np.int32), obs=np.sort(obs).astype(np.int32),
                depth=len(widths))


# ---- the transformations ---------------------------------------------------------------------------------------------------------
def _copy(w):
    return {k: v.copy() for k, v in w.items()}


def unit_sets(case):
    """name -> (layer, unit indices) of the hidden units `rescale_units` moves."""
    widths = SHAPES[case][5]
    if case == "G":
        return {"units.l1": (1, np.arange(0, widths[0], 2)), "units.l2": (2, np.arange(0, widths[1], 2))}
    if case == "W":     # inside the first hidden slice of 256, and the whole second slice
        return {"units.s0": (1, np.arange(0, 256, 2)), "units.s1": (1, np.arange(256, widths[0]))}
    return {"units": (1, np.arange(0, widths[0], 2))}


def rescale_units(w, k, layer, idx):
    w = _copy(w)
    s = np.float32(2.0 ** k)
    wi, bi, wo = f"W{layer}", f"b{layer}", f"W{layer + 1}"
    w[wi][:, idx] *= s
    w[bi][idx] *= s
    w[wo][idx, :] /= s
    return w


def rescale_features(x, w, k):
    x, w = x.copy(), _copy(w)
    s = np.float32(2.0 ** k)
    j = np.arange(0, x.shape[1], 8)
    x[:, j] *= s
    w["W1"][j, :] /= s
    return x, w


def kink_row(case, layer=1):
    """The weights with the bias of `layer` chosen so that EVERY unit of that layer has a pre-activation of (almost) zero in row r0:
    b = -(A_hat * input * W)[r0], formed in fp64 and cast to fp32."""
    c = base(case)
    w = _copy(c["w"])
    a = c["a_hat"].astype(np.float64)
    s = c["x"].astype(np.float64) @ w["W1"].astype(np.float64)
    if layer == 2:
        h1 = np.maximum(a @ s + w["b1"].astype(np.float64), 0.0)
        s = h1 @ w["W2"].astype(np.float64)
    w[f"b{layer}"] = (-(a @ s)[c["r0"]]).astype(np.float32)
    return w


def variants(case):
    """The base weight sets whose oracle matrix is a fixture: `plain`, and a kink row per hidden layer."""
    return ("plain", "kink", "kink2") if case == "G" else ("plain", "kink")


def transforms(case, variant):
    """The transformations applied on top of a variant: the unit sets, and for the 2-layer Baseline cases the feature columns."""
    t = list(unit_sets(case))
    # (M's kink row takes the feature columns too: without a row at its kinks only the handful of units that happen to cross one
    # see the int8 split's resolution at all)
    if (variant == "plain" and case in ("M", "R", "A")) or (variant == "kink" and case == "M"):
        t.append("features")
    return t


def inputs(case, variant="plain", transform=None, k=0):
    """(x, w) of a cell.  k = 0 (or no transform): the variant itself."""
    c = base(case)
    w = _copy(c["w"]) if variant == "plain" else kink_row(case, 2 if variant == "kink2" else 1)
    x = c["x"]
    if transform is None or k == 0:
        return x, w
    if transform == "features":
        return rescale_features(x, w, k)
    layer, idx = unit_sets(case)[transform]
    return x, rescale_units(w, k, layer, idx)


def cells(case):
    """Every (variant, transform, k) of a case: k = 0 once per variant (transform None), then the ladder per transformation.  The
    kink rows of A, G and W are k = 0 only (their default storage is fp64 or scales with the units); Q, which is M with one K slice,
    takes the ladder on its kink row only."""
    out = []
    for v in variants(case):
        out.append((v, None, 0))
        if (v != "plain" and case not in ("M", "Q", "R")) or (v == "plain" and case == "Q"):
            continue
        for t in transforms(case, v):
            out.extend((v, t, k) for k in LADDER)
    return out


def cell_key(case, variant, transform, k):
    return f"{case}.{variant}.{transform or 'none'}.{k}"

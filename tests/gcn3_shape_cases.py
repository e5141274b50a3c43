"""Inputs of the GCN3 shape tests (test_gcn3_shapes_cpu.py, test_gcn3_shapes_gpu.py): the width and class ladders of the 3-layer
attack (lt_influence3_rows_mode / lt_influence3_pairs, narrow and wide handles), a graph whose probe bitmaps have more than 256
words, and a row at its kinks behind padded and wide layers.  numpy / scipy only; the small graphs, their node lists and the
weights are those of test_gcn3_wide_attack_gpu (imported where they are needed: that module imports torch).

What the shapes are for (lt_gcn3.hip): a hidden width H is served as Hp = lt_round_up(H, 4) columns by a lane group of
lt_lpr_for(Hp) lanes, four columns a lane.  H != Hp puts pad columns behind every layer kernel (k3_pad, the memsets of S2 / S2x /
Spd, the K = H tail of the MFMA products); a class count C of a wide handle does the same to the last step (Cp, `coff + k < C`)."""
import functools

import numpy as np
import scipy.sparse as sp

from linkteller_amd import graph, synth

DELTA = 1e-4
KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")

# (H1, H2, C) of the issue's ladders: narrow handles (engine.Baseline3, C <= 8) and wide ones (lt_baseline3_create_wide)
NARROW = ((1, 1, 1), (3, 2, 1), (5, 3, 2), (7, 9, 3), (13, 6, 4), (17, 5, 5), (30, 19, 7), (33, 31, 8), (66, 35, 2), (127, 65, 3),
          (129, 130, 6), (255, 253, 8), (250, 256, 5))
WIDE = ((5, 3, 1), (7, 9, 4), (13, 6, 5), (17, 5, 10), (30, 19, 11), (33, 31, 13), (3, 4, 16), (66, 35, 17), (18, 22, 23),
        (127, 65, 32), (9, 30, 33), (6, 7, 47), (129, 130, 64), (21, 14, 65), (11, 127, 99), (255, 253, 128), (10, 129, 129),
        (250, 256, 190), (2, 3, 255))
LADDER = [(s, False) for s in NARROW] + [(s, True) for s in WIDE]
GRAPHS = ("er", "loops")
# the graph whose feature rows have an odd stride (F = 29: ldx odd, rows of X off 16 bytes)
ER29 = (((7, 9, 3), False), ((30, 19, 7), False), ((30, 19, 11), True), ((21, 14, 65), True))
# the padded shapes the relations without a tolerance run on
RELATIONS = (((7, 9, 3), False), ((30, 19, 7), False), ((30, 19, 11), True), ((21, 14, 65), True), ((10, 129, 129), True))
# the graph of more than 256 bitmap words
BIG_N = 16500
BIG = (((17, 9, 3), False), ((17, 9, 13), True), ((16, 12, 9), True))
# every node of `er` as a probe: more than 256 probes in one wide chunk
ALL_PROBES = ((16, 12, 9), (17, 5, 10))
# a row at its kinks: (widths, weight seed, handles)
KINKS = (((30, 19, 41), 0, ("wide",)), ((30, 19, 7), 4, ("narrow", "wide")))
VARIANTS = ("plain", "kink", "kink2")
EXACT_KS = (-20, -8, 8, 20)


def case_id(case):
    return "x".join(map(str, case[0])) + ("w" if case[1] else "")


# ---- the library's width rules, restated -------------------------------------------------------------------------------------------
def round_up4(x):
    """lt_round_up(x, 4)"""
    return (x + 3) // 4 * 4


def lpr_for(hp):
    """lt_lpr_for: lanes of the group that serves hp (a multiple of 4) columns, four a lane -- the next power of two."""
    need, l = hp // 4, 1
    while l < need:
        l <<= 1
    return l


def lprs(shape, wide):
    """(LPR of Hp1, LPR of Hp2, LPR of Cp or None for a narrow handle)"""
    h1, h2, c = shape
    return lpr_for(round_up4(h1)), lpr_for(round_up4(h2)), lpr_for(round_up4(c)) if wide else None


def padded(shape, wide):
    """which of (H1, H2, C) have pad columns (C: of a wide handle alone; a narrow one keeps its class rows dense)"""
    h1, h2, c = shape
    return h1 % 4 != 0, h2 % 4 != 0, wide and c % 4 != 0


# ---- the small graphs ----------------------------------------------------------------------------------------------------------------
def er_recipe(f):
    """The `er` graph of test_gcn3_wide_attack_gpu._graph with F = f feature columns: the same adjacency and node lists (the same
    draws in the same order), features of the same law.  (test_gcn3_shapes_cpu.py asserts that f = 32 gives that graph itself.)"""
    n, m, seed = 300, 600, 3
    rng = np.random.RandomState(seed)
    a = sp.lil_matrix((n, n))
    while a.nnz < 2 * m:
        i, j = rng.randint(0, n, 2)
        if i != j:
            a[i, j] = a[j, i] = 1.0
    a_hat = sp.csr_matrix(graph.first_order_gcn(sp.csr_matrix(a))).astype(np.float32)
    a_hat.sort_indices()
    x = synth.gaussian_features(n, f, seed=seed + 10).copy()
    pick = rng.choice(n, 44, replace=False)
    probes = list(pick[:24]) + [int(pick[3])]
    obs = list(pick[12:44]) + [int(pick[20]), int(pick[40])]
    zero = int(pick[1])
    x[zero] = 0.0
    probes, obs = np.asarray(probes, dtype=np.int32), np.asarray(obs, dtype=np.int32)
    return a_hat, np.ascontiguousarray(x, dtype=np.float32), probes, obs, int(np.flatnonzero(probes == zero)[0])


@functools.lru_cache(maxsize=None)
def small_graph(name):
    """(a_hat, x, probes, obs, row of the all-zero probe) of `er`, `loops` (test_gcn3_wide_attack_gpu._graph) or `er29`."""
    if name == "er29":
        return er_recipe(29)
    import test_gcn3_wide_attack_gpu as W
    return W._graph(name)


def small_params(name, shape):
    """The weights of test_gcn3_wide_attack_gpu._params(shape); on `er29` the first 29 rows of its W1."""
    import test_gcn3_wide_attack_gpu as W
    p = dict(W._params(tuple(shape)))
    if name == "er29":
        p["W1"] = np.ascontiguousarray(p["W1"][:29])
    return p


# ---- the graph of 516 bitmap words ---------------------------------------------------------------------------------------------------
BIG_SPECIAL = (8191, 8192, 16383, 16384, BIG_N - 1)      # the ends of the stretches of 256 words, and the last node


def stretch_of(ids):
    """the 256-word stretch (8192 node ids) of k3_list2 / k3w_rank2 an id falls in"""
    return np.asarray(ids) // 8192


def hops(a_hat, v, k):
    """the nodes within k hops of v along the pattern of a_hat (its diagonal included), ascending"""
    at = a_hat.T.tocsr()
    cur = np.array([v])
    for _ in range(k):
        cur = np.unique(np.concatenate([at[int(r)].indices for r in cur]))
    return cur


@functools.lru_cache(maxsize=None)
def big_graph():
    """(a_hat, x, probes, obs, row of the all-zero probe): n = 16500 -- 516 words, stretches of 256, 256 and 4.  An Erdos-Renyi
    draw of 2 n edges (R2 of 10 .. 30 nodes anywhere in the id range) plus planted edges: node 0 is tied to the ends of the
    stretches and to the last node, so R2 of probe 0 and of every one of those holds all five ids; nodes 5 and 16400 get a
    neighbour in each stretch.  Probes: 0, the five special ids, 5, 16400, random ones (one of them twice, one with an all-zero
    feature row).  Observed: nodes of the probes' 3-hop sets (most of them near node 0, which the planted probes share), the
    special ids, and nodes no probe reaches."""
    n = BIG_N
    adj = synth.erdos_renyi_graph(n, 2 * n, seed=11).tolil()
    for u, v in [(0, s) for s in BIG_SPECIAL] + [(5, 9000), (5, 16450), (16400, 77), (16400, 12000), (16400, 16499 - 1)]:
        adj[u, v] = adj[v, u] = 1.0
    a_hat = sp.csr_matrix(graph.first_order_gcn(sp.csr_matrix(adj))).astype(np.float32)
    a_hat.sort_indices()
    x = synth.gaussian_features(n, 32, seed=12).copy()
    rng = np.random.RandomState(13)
    far = [int(v) for v in rng.choice(n, 5, replace=False)]
    probes = [0] + list(BIG_SPECIAL) + [5, 16400] + far + [far[1]]
    zero = far[0]
    x[zero] = 0.0
    near = hops(a_hat, 0, 3)
    reach = np.unique(np.concatenate([hops(a_hat, v, 3) for v in probes]))
    others = np.setdiff1d(reach, near)
    unreached = np.setdiff1d(np.arange(n), reach)
    obs = np.concatenate([rng.choice(near, 40, replace=False), BIG_SPECIAL, [0], rng.choice(others, 12, replace=False),
                          rng.choice(unreached, 8, replace=False), [unreached[0], unreached[-1]]])
    obs = np.concatenate([obs, obs[:2]])                       # repeated observed ids
    probes, obs = np.asarray(probes, dtype=np.int32), np.asarray(obs, dtype=np.int32)
    return a_hat, np.ascontiguousarray(x, dtype=np.float32), probes, obs, int(np.flatnonzero(probes == zero)[0])


def big_params(shape):
    import test_gcn3_wide_attack_gpu as W
    return W._params(tuple(shape))


# ---- a row at its kinks ----------------------------------------------------------------------------------------------------------------
def _uniform(rng, shape, fan_out):
    s = 1.0 / np.sqrt(fan_out)
    return rng.uniform(-s, s, size=shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def kink_base():
    """graph, features, r0, probes and observed list of value_domain_cases.base("G")"""
    import value_domain_cases as V
    c = V.base("G")
    return dict(a_hat=c["a_hat"], x=c["x"], r0=c["r0"], probes=c["probes"], obs=c["obs"])


def kink_weights(widths, seed, variant="plain", k=0):
    """Three layers drawn as value_domain_cases.base draws them; `kink` / `kink2`: b1 / b2 chosen as value_domain_cases.kink_row
    chooses it, so that every unit of row r0 has a pre-activation of zero in that layer; k != 0: the even hidden units of layer 2
    rescaled by 2^k (value_domain_cases.rescale_units)."""
    import value_domain_cases as V
    c = kink_base()
    f = c["x"].shape[1]
    h1, h2, cc = widths
    rng = np.random.RandomState(seed)
    w = dict(W1=_uniform(rng, (f, h1), h1), b1=_uniform(rng, (h1,), h1), W2=_uniform(rng, (h1, h2), h2),
             b2=_uniform(rng, (h2,), h2), W3=_uniform(rng, (h2, cc), cc), b3=_uniform(rng, (cc,), cc))
    if variant != "plain":
        layer = 2 if variant == "kink2" else 1
        a = c["a_hat"].astype(np.float64)
        s = c["x"].astype(np.float64) @ w["W1"].astype(np.float64)
        if layer == 2:
            s = np.maximum(a @ s + w["b1"].astype(np.float64), 0.0) @ w["W2"].astype(np.float64)
        w[f"b{layer}"] = (-(a @ s)[c["r0"]]).astype(np.float32)
    if k:
        w = V.rescale_units(w, k, 2, np.arange(0, h2, 2))
    return w


def pre_activation(c, w, layer):
    """fp64 pre-activation of `layer` (1 or 2), every row"""
    a = c["a_hat"].astype(np.float64)
    z = a @ (c["x"].astype(np.float64) @ w["W1"].astype(np.float64)) + w["b1"].astype(np.float64)
    if layer == 2:
        z = a @ (np.maximum(z, 0.0) @ w["W2"].astype(np.float64)) + w["b2"].astype(np.float64)
    return z

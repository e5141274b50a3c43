"""Inputs of the shape tests of the wide 2-layer handle (lt_baseline2w_create; test_wide2_shapes_cpu.py, test_wide2_shapes_gpu.py):
the (H, C) ladder over every lane-group width of both sides, one model per storage form of the inner fp64 baseline, a graph of more
than 256 bitmap words, probe lists of 300 and of 65537 entries, and probes whose item counts sit at the 64-row tile edges of the
product dS2x = dH1x W2.  numpy / scipy only; the small graphs, their node lists and the F = 32 weights are those of
test_wide2_handle_gpu (imported where they are needed: that module imports torch), the width rules and the graph of 516 bitmap words
those of gcn3_shape_cases.

What the shapes are for (lt_gcn3.hip, influence2w_impl): the hidden width is served as Hp = lt_round_up(H, 4) columns by a lane group
of lt_lpr_for(Hp) lanes (k3d_items1<LPR>), the class width as Cp columns by lt_lpr_for(Cp) lanes (k3dw_stageC<LPR> /
k3dw_stageC_pairs<LPR>); between them lt_launch_gemm_mdev forms dS2x with K = H, N = C, lda = Hp, ldb = C, ldc = Cp over a row count
that lives on the device.  The probes' fp64 product rows and the pre-activation come from an inner 2-layer baseline whose storage form
is decided by compute_s1d (lt_fp64.hip) from shapes, knobs and the features: STORAGE below has one case per form."""
import functools

import numpy as np

import boundary_cases as B
import gcn3_shape_cases as S
from gcn3_shape_cases import lpr_for, round_up4
from linkteller_amd import synth

DELTA = 1e-4
GATE = 1e-5                  # the project's bound of every `delta` test: |ours - ref64|.max() <= 1e-5 * ref64.max()
KEYS = ("W1", "b1", "W2", "b2")
KEYS3 = ("W1", "b1", "W2", "b2", "W3", "b3")

# ---- 1. the lane-group ladder ----------------------------------------------------------------------------------------------------
LADDER = ((1, 13), (3, 4), (5, 17), (7, 33), (9, 65), (13, 129), (17, 10), (21, 7), (30, 63), (33, 64), (65, 127), (127, 128),
          (129, 193), (64, 192), (255, 23), (253, 256), (256, 255), (250, 190), (6, 1), (22, 9), (12, 32), (16, 16), (2, 5))
GRAPHS = ("er", "loops")
# the padded shapes (Hp != H and Cp != C) the relations without a tolerance run on
RELATIONS = ((7, 33), (30, 63), (13, 129), (21, 7))


def shape_id(shape):
    return "x".join(map(str, shape))


def small_graph(name):
    """(a_hat, x, probes, obs, row of the all-zero probe) of test_wide2_handle_gpu._graph: `er` (n = 300, 1500 edges) or `loops`."""
    import test_wide2_handle_gpu as W
    return W._graph(name)


def small_params(shape):
    import test_wide2_handle_gpu as W
    return W._params(tuple(shape))


def oracle(a_hat, x, params, probes, obs):
    """oracle.linkteller_oracle.influence_matrix on float64 tensors, as test_wide2_handle_gpu._oracle calls it (three layers: as
    test_gcn3_wide_attack_gpu._oracle does)."""
    if "W3" in params:
        import test_gcn3_wide_attack_gpu as W3
        return W3._oracle(a_hat, x, params, probes, obs)
    import test_wide2_handle_gpu as W
    return W._oracle(a_hat, x, params, probes, obs)


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ladder_ref(name, shape):
    a_hat, x, probes, obs, _ = small_graph(name)
    return _frozen(oracle(a_hat, x, small_params(shape), probes, obs))


def logits64(a_hat, x, params):
    import torch
    from oracle import linkteller_oracle as O
    fwd = O.gcn3_forward if "W3" in params else O.gcn_forward
    return fwd(torch.from_numpy(np.asarray(x)).double(), O.to_torch_sparse(a_hat).double(),
               {k: torch.from_numpy(np.asarray(v)).double() for k, v in params.items()}).numpy()


# ---- 2. one model per storage form of the inner baseline -------------------------------------------------------------------------
# case -> (features, F, H, C, knobs, expected form).  The form: route (lt_baseline_fp64_route of a narrow twin), fixed (32-bit
# fixed-point product rows), deferred (the readers add cref), i8 (the int8 split of the dense product), slices (its K slices),
# same_as (the case whose bits the knobs must keep), tiled (the fp64 SpMM takes lt_launch_rows_tiled_f64).  "feature_delta" = 1: the
# detector of lt_baseline_enable_fp64 leaves an indicator matrix of this density to the matrix cores (asserted on the GPU, case g)
STORAGE = {
    "a": ("gaussian", 300, 64, 41, {}, dict(route=0, fixed=True, deferred=False, i8=True, slices=2)),
    "b": ("gaussian", 256, 64, 9, {}, dict(route=0, fixed=True, deferred=False, i8=True, slices=1)),
    "c": ("gaussian", 300, 256, 121, {}, dict(route=0, fixed=True, deferred=False, i8=True, slices=2)),
    "d": ("gaussian", 300, 64, 41, dict(i8_split=0), dict(route=0, fixed=True, deferred=False, i8=False)),
    "e": ("gaussian", 300, 64, 41, dict(i8_split=0, s1_f32=0), dict(route=0, fixed=False, deferred=False, i8=False)),
    "f": ("gaussian", 300, 66, 41, {}, dict(route=0, fixed=False, deferred=False, i8=False)),
    "g": ("twitch", 304, 64, 41, dict(feature_delta=1), dict(route=1, fixed=True, deferred=True, i8=False)),
    "h": ("twitch", 304, 64, 41, dict(feature_delta=1, defer_cref=0), dict(route=1, fixed=False, deferred=False, i8=False)),
    "i": ("twitch", 304, 66, 41, dict(feature_delta=1), dict(route=1, fixed=False, deferred=False, i8=False)),
    "j": ("twitch", 303, 64, 41, dict(feature_delta=1), dict(route=1, fixed=True, deferred=True, i8=False)),
    "k1": ("twitch", 304, 64, 41, dict(feature_delta=1, feature_lists=1), dict(route=1, fixed=True, deferred=True, i8=False, same_as="g")),
    "k0": ("twitch", 304, 64, 41, dict(feature_delta=1, feature_lists=0), dict(route=1, fixed=True, deferred=True, i8=False, same_as="g")),
    "l": ("gaussian", 300, 64, 41, dict(i8_split=0, tiled_min_bytes=0, s1_f32=0, defer_cref=0),
          dict(route=0, fixed=False, deferred=False, i8=False, same_as="e", tiled=True)),
    "m": ("gaussian", 32, 128, 41, {}, dict(route=0, fixed=True, deferred=False, i8=False, big=True)),
}
# the feature and weight seeds: the first ones tried -- the storage model puts every case inside the domain with room to spare
# (test_wide2_shapes_cpu.test_storage_model_is_inside_the_domain prints the figures; NOTES.md has them)
FEATURE_SEED = {"gaussian": 31, "twitch": 32}
WEIGHT_SEED = {k: 40 for k in STORAGE}
# the cases the refresh checks run on, and the 3-layer widths (H2, C) the same first layers sit behind in part 5
REFRESH = ("a", "g")
BEHIND3 = {"narrow": (19, 7), "wide": (19, 13)}


def stores(case):
    """does the case store fixed point or take the int8 split (value_domain_model has something to model)"""
    form = STORAGE[case][5]
    return form["fixed"] or form["i8"]


def model_kw(case):
    form = STORAGE[case][5]
    return dict(rows="rows31" if form["fixed"] else None, i8=form["i8"])


def i8_shapes_ok(n, h, f):
    """lt_i8_shapes_ok (lt_i8_split.hip.h)"""
    return n >= 256 and f >= 256 and h >= 64 and h % 64 == 0 and f < (1 << 15)


def dense_quant_shapes(n, h):
    """dense_quant_shapes (lt_fp64.hip): the dense product's rows leave as 32-bit fixed point"""
    return n * round_up4(h) * 8 < (32 << 20) and h <= 256 and h % 4 == 0


def fp64_big(n, h):
    """fp64_big (lt_fp64.hip): the 128-wide tiles of the f64 matrix-core product"""
    return n >= 1024 and h % 128 == 0


@functools.lru_cache(maxsize=None)
def storage_features(kind, f, big=False):
    """Features of a storage case on `er` (n = 300) or on the graph of 516 bitmap words.  Gaussian ones keep the all-zero row of the
    graph's zero probe; the twitch-like indicator matrix (synth.twitch_like_features, density 0.05 as value_domain_cases' case R
    draws it at 0.02) keeps every row as it is: a row of zeros differs from the reference row in every column."""
    if big:
        assert kind == "gaussian" and f == 32
        return S.big_graph()[1]
    n = 300
    if kind == "twitch":
        return np.ascontiguousarray(synth.twitch_like_features(n, f, seed=FEATURE_SEED[kind], density=0.05))
    _, _, probes, _, zrow = small_graph("er")
    x = synth.gaussian_features(n, f, seed=FEATURE_SEED[kind]).copy()
    x[probes[zrow]] = 0.0
    return np.ascontiguousarray(x, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def storage_case(case):
    """dict(a_hat, x, w, probes, obs, zrow, knobs, form) of a storage case; the arrays are shared: copy before writing."""
    kind, f, h, c, kn, form = STORAGE[case]
    big = bool(form.get("big"))
    if big:
        a_hat, _, probes, obs, zrow = big_graph2()
    else:
        a_hat, _, probes, obs, zrow = small_graph("er")
    x = storage_features(kind, f, big)
    w = dict(synth.gcn_weights(f, h, c, seed=WEIGHT_SEED[case]))
    return dict(a_hat=a_hat, x=x, w=w, probes=probes, obs=obs, zrow=zrow if kind == "gaussian" else None, knobs=dict(kn), form=form,
                shape=(f, h, c))


def inputs_key(case):
    """cases with the same key have the same inputs (a, d, e, l; g, k1, k0): the knobs change no input, one oracle run serves them"""
    kind, f, h, c, _, form = STORAGE[case]
    return kind, f, h, c, WEIGHT_SEED[case], bool(form.get("big"))


@functools.lru_cache(maxsize=None)
def _ref_of_inputs(key, case):
    c = storage_case(case)
    return _frozen(oracle(c["a_hat"], c["x"], c["w"], c["probes"], c["obs"]))


def storage_ref(case):
    key = inputs_key(case)
    return _ref_of_inputs(key, min(k for k in STORAGE if inputs_key(k) == key))


def updated(case, what):
    """The inputs of a refresh check: `w1` -- W1 scaled by 1.25 on its even columns (in place on the device: the same fp32 products);
    `x` -- on top of that, three entries of one probe's feature row moved (the row stays sparse on the feature route)."""
    c = storage_case(case)
    w = {k: v.copy() for k, v in c["w"].items()}
    w["W1"][:, ::2] *= np.float32(1.25)
    x = c["x"].copy()
    if what == "x":
        row = int(c["probes"][5])
        for j, v in ((3, 0.5), (17, -1.25), (c["x"].shape[1] - 1, 2.0)):
            x[row, j] += np.float32(v)
    return x, w


@functools.lru_cache(maxsize=None)
def updated_ref(case, what):
    c = storage_case(case)
    x, w = updated(case, what)
    return _frozen(oracle(c["a_hat"], x, w, c["probes"], c["obs"]))


def behind3_params(case, kind):
    """Three layers whose first is the storage case's: (W1, b1) of the case, then H2 and C of BEHIND3, drawn by the init law."""
    c = storage_case(case)
    h = c["shape"][1]
    h2, cc = BEHIND3[kind]
    rng = np.random.RandomState(500 + 7 * h2 + cc)

    def u(shape, fan_out):
        s = 1.0 / np.sqrt(fan_out)
        return rng.uniform(-s, s, size=shape).astype(np.float32)
    return dict(W1=c["w"]["W1"], b1=c["w"]["b1"], W2=u((h, h2), h2), b2=u((h2,), h2), W3=u((h2, cc), cc), b3=u((cc,), cc))


@functools.lru_cache(maxsize=None)
def behind3_ref(case, kind):
    c = storage_case(case)
    return _frozen(oracle(c["a_hat"], c["x"], behind3_params(case, kind), c["probes"], c["obs"]))


# ---- 3. bitmap words, chunk sizes, item counts -----------------------------------------------------------------------------------
BIG = ((17, 13), (16, 41))
ALL_PROBES = ((16, 41), (17, 10))
CAP = 65534                  # carve2w: probes per chunk at the most
CAP_PROBES = 65537
CAP_SHAPE = (5, 9)
HUB_SHAPE = (18, 65)
HUB_COLUMNS = (1, 63, 64, 65, 128, 129, 513)
# (probe, the one item that can serve the cell, first id the item must reach): the planted edges of gcn3_shape_cases.big_graph
STRETCH_CELLS = ((16400, 12000, 8192), (5, 16450, 16384), (5, 9000, 8192))


@functools.lru_cache(maxsize=None)
def big_graph2():
    """gcn3_shape_cases.big_graph (n = 16500: 516 bitmap words) with an observed list for TWO hops, by the same recipe: nodes of the
    2-hop set of node 0 (which the planted probes share), the special ids, node 0, nodes of the other probes' 2-hop sets, nodes no
    probe reaches, repeated ids -- and, per entry of STRETCH_CELLS, a neighbour of the item that is a neighbour of no other item of
    the probe: a cell only that item can serve."""
    a_hat, x, probes, _, zrow = S.big_graph()
    n = a_hat.shape[0]
    rng = np.random.RandomState(14)
    near = S.hops(a_hat, 0, 2)
    reach = np.unique(np.concatenate([S.hops(a_hat, int(v), 2) for v in probes]))
    others = np.setdiff1d(reach, near)
    unreached = np.setdiff1d(np.arange(n), reach)
    planted = [stretch_cell(a_hat, v, r)[0] for v, r, _ in STRETCH_CELLS]
    obs = np.concatenate([rng.choice(near, 24, replace=False), S.BIG_SPECIAL, [0], rng.choice(others, 24, replace=False), planted,
                          rng.choice(unreached, 8, replace=False), [unreached[0], unreached[-1]]])
    obs = np.concatenate([obs, obs[:2]])
    return a_hat, x, probes, obs.astype(np.int32), zrow


def stretch_cell(a_hat, v, r):
    """(u, items): the first neighbour u of item r of probe v whose row meets the probe's items in r alone."""
    items = a_hat.T.tocsr()[int(v)].indices
    assert r in items
    for u in a_hat.T.tocsr()[int(r)].indices:
        if u != r and u != v and np.array_equal(np.intersect1d(a_hat[int(u)].indices, items), [r]):
            return int(u), items
    raise AssertionError((v, r))


@functools.lru_cache(maxsize=None)
def big_ref(shape):
    a_hat, x, probes, obs, _ = big_graph2()
    return _frozen(oracle(a_hat, x, small_params(shape), probes, obs))


@functools.lru_cache(maxsize=None)
def all_probes_ref(shape):
    a_hat, x, _, obs, _ = small_graph("er")
    return _frozen(oracle(a_hat, x, small_params(shape), np.arange(a_hat.shape[0], dtype=np.int32), obs))


@functools.lru_cache(maxsize=None)
def cap_lists():
    """(probes of the graph `loops`, the same list tiled to 65537 entries, three observed nodes)"""
    _, _, probes, obs, _ = small_graph("loops")
    assert 5 in probes and len(probes) == 28
    return probes, np.resize(probes, CAP_PROBES).astype(np.int32), np.asarray([obs[0], obs[13], 5], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def cap_ref():
    a_hat, x, _, _, _ = small_graph("loops")
    probes, _, obs = cap_lists()
    return _frozen(oracle(a_hat, x, small_params(CAP_SHAPE), probes, obs))


@functools.lru_cache(maxsize=None)
def hub_lists():
    """(probes, observed) on the hub ladder of boundary_cases.py: the nodes whose columns hold HUB_COLUMNS entries -- the item counts
    of a chunk of one; observed: the hub rows of 129, 257 and 1025 entries and, per probe, the first row of its column (a pool node:
    through its self loop the cell reads that one item)."""
    g = B.hub_ladder()
    probes = np.asarray([g.v[c] for c in HUB_COLUMNS], dtype=np.int32)
    obs = np.asarray([g.u[129], g.u[257], g.u[1025]] + [int(g.col_sets[c][0]) for c in HUB_COLUMNS], dtype=np.int32)
    return probes, obs


@functools.lru_cache(maxsize=None)
def hub_ref():
    a_hat, x, _, _, _ = small_graph("hub")
    probes, obs = hub_lists()
    return _frozen(oracle(a_hat, x, small_params(HUB_SHAPE), probes, obs))


# ---- 4. strides through the C ABI ------------------------------------------------------------------------------------------------
ER29 = ((7, 33), (30, 63))


def er29_params(shape):
    p = dict(small_params(shape))
    p["W1"] = np.ascontiguousarray(p["W1"][:29])
    return p

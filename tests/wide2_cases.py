"""Inputs and references of the wide 2-layer attack's tests (test_wide2_cpu.py, test_wide2_gpu.py): lt_wide_combine restated bit
for bit, the pairs' difference VECTORS of lt_influence_rows_vec in plain fp64 in the oracle's order of operations, and the shapes
engine.WideBaseline is cut at.
numpy / scipy only; the graphs, node lists, features, weights and the oracle matrices are those of boundary_cases.py (F = 32).

What the shapes are for (engine.WideBaseline._build): the hidden layer is served in slices of 256 units, the classes in slices
of 8; a slice of h units is stored as hp = (h + 3) // 4 * 4 columns (H = 257: one unit behind three pad columns); lt_wide_combine
takes at most 32 hidden slices (LT_WIDE_MAX_VEC, lt_influence.hip) and at most 8 classes a call (LT_MAX_C)."""
import functools
import types

import numpy as np

import boundary_cases as B
from train_restate import fma32

DELTA = B.DELTA
GATE = 1e-5             # the project's bound of every `delta` test: |ours - ref64|.max() <= 1e-5 * ref64.max()
MAX_VEC = 32            # LT_WIDE_MAX_VEC
MAX_C = 8               # LT_MAX_C: classes of one slice
H_SLICE = 256

# (test_boundary_gpu.ITEM_KNOBS, copied: the stage-B variants of the item kernels)
ITEM_KNOBS = [dict(stageb_rows=0), dict(pair_marks=0, pair_list=0), dict(pair_marks=0, pair_list=1),
              dict(bits_max_bytes=0, hub_short_side=0), dict(bits_max_bytes=0, hub_short_side=1), dict(item_bits=0),
              dict(bits_max_bytes=0, pair_marks=-1, hub_short_side=0), dict(bits_max_bytes=0, pair_marks=-1, hub_short_side=1),
              dict(item_bits=0, pair_marks=-1),
              dict(hub_short_side=1), dict(hub_short_side=1, stageb_rows=0)]

# (H, C) of WideBaseline on the hub ladder: (hidden slices, class slices)
WIDE_SHAPES = ((257, 2),      # 256 + 1: a hidden slice of one unit
               (260, 9),      # 256 + 4, 8 + 1: a one-class slice
               (512, 8),      # two full hidden slices, one class slice
               (513, 3),      # three hidden slices
               (64, 17),      # class slices 8 + 8 + 1
               (256, 24))     # one hidden slice, three full class slices
KNOB_SHAPE = (260, 9)


def slices(h, c):
    """(hidden slices, class slices) as WideBaseline cuts them."""
    return ([(s, min(s + H_SLICE, h)) for s in range(0, h, H_SLICE)], [(t, min(t + MAX_C, c)) for t in range(0, c, MAX_C)])


# ---- A. lt_wide_combine ---------------------------------------------------------------------------------------------------------
def combine_restated(vecs, C, delta, ss, first, last):
    """include/linkteller_hip.h, lt_wide_combine, in float32 numpy: per pair and class d = ((v0 + v1) + v2 ...) in slice order,
    d = d / delta, acc = fma(d, d, acc) in class order from 0 (first) or from ss, sqrt on the last class slice.  ``vecs``: the
    slices' [n_pairs, C] arrays; returns the new ss (``ss`` itself is left alone)."""
    f = np.float32
    vecs = [np.asarray(v, dtype=f).reshape(-1, C) for v in vecs]
    acc = np.zeros(len(vecs[0]), dtype=f) if first else np.array(ss, dtype=f).ravel()
    with np.errstate(all="ignore"):
        for c in range(C):
            d = vecs[0][:, c]
            for v in vecs[1:]:
                d = np.add(d, v[:, c], dtype=f)
            d = np.divide(d, f(delta), dtype=f)
            acc = fma32(d, d, acc)
        return np.sqrt(acc, dtype=f) if last else acc


def combine_inputs(n_vec, C, n_pairs, seed=0):
    """float32 [n_vec, n_pairs, C]: unscaled differences of mixed sign whose magnitudes spread over four decades around
    DELTA x (a score of order one), so that neither the slices' sum nor the classes' fma chain is exact in any order; and,
    where they fit, the odd pairs:
      0  the slices cancel exactly (v1 = -v0, the others zero): d = 0;
      1  all zeros of mixed sign;
      2  one subnormal component and nothing else (d is normal, its square underflows);
      3  a subnormal component beside normal ones;
      4  two slices whose sum is subnormal (a cancellation that leaves 2^-143)."""
    rng = np.random.RandomState(1000 * n_vec + 10 * C + seed)
    v = (rng.standard_normal((n_vec, n_pairs, C)) * 10.0 ** rng.uniform(-7, -3, (n_vec, n_pairs, C))).astype(np.float32)
    if n_pairs >= 5:
        if n_vec >= 2:
            v[2:, 0] = 0
            v[1, 0] = -v[0, 0]
            v[:, 4] = 0
            v[0, 4, 0] = np.float32(2.0 ** -120 + 2.0 ** -140)           # (its last place is 2^-143)
            v[1, 4, 0] = -np.float32(2.0 ** -120 + 2.0 ** -140 - 2.0 ** -143)
        v[:, 1] = np.where(rng.randint(0, 2, (n_vec, C)) == 1, np.float32(-0.0), np.float32(0.0))
        v[:, 2] = 0
        v[0, 2, 0] = np.float32(1e-41)
        v[0, 3, C - 1] = np.float32(-3e-42)
    return v


COMBINE_DELTAS = (1e-4, -1e-4)
# (n_vec, C, n_pairs): every n_pairs of the block ladder at full width, C and n_vec swept at 257 pairs (two blocks, the second one thread)
COMBINE_CASES = ([(MAX_VEC, MAX_C, n) for n in (1, 255, 256, 257, 70001)]
                 + [(nv, c, 257) for nv in (1, 2, 3, MAX_VEC) for c in range(1, MAX_C + 1) if (nv, c) != (MAX_VEC, MAX_C)])
# one pair shows an order by chance (about every other draw does): the one-pair case takes a draw whose pair shows both orders
# (test_wide2_cpu.test_combine_inputs_have_bite asserts it)
ONE_PAIR_SEED = 5


def combine_case(n_vec, C, n_pairs):
    return combine_inputs(n_vec, C, n_pairs, ONE_PAIR_SEED if n_pairs == 1 else 0)


# ---- B. the difference vectors in fp64 ---------------------------------------------------------------------------------------------
def forward64(a, x, w):
    """f = A relu(A X W1 + b1) W2 + b2 in float64, the reference's op order (gcn/layers.py:30-36); (logits, H1 W2)."""
    s2 = np.maximum(a @ (x @ w["W1"]) + w["b1"], 0.0) @ w["W2"]
    return a @ s2 + w["b2"], s2


def _w64(w):
    return {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}


def probe_differences(a, x, w, probes, obs, delta=DELTA):
    """Per probe v: X with row v scaled by 1 + delta (x_v + x_v delta, attacker.py:103-105) through forward64, minus the
    unperturbed forward, over delta.  Returns (vectors [n_probe, n_obs, C], hidden [n_probe, n, C]): the rows ``obs`` of the
    logits' difference, and the difference of H1 W2 on every row -- A[u] @ hidden[i] is vectors[i, u] up to fp64 rounding,
    which is how the mutation test evaluates a changed row of A without another forward.  ``a`` is the adjacency as the
    device holds it (B.f32_values)."""
    a = B.f32_values(a)
    x = np.asarray(x, dtype=np.float64)
    w = _w64(w)
    base, s2 = forward64(a, x, w)
    vec = np.zeros((len(probes), len(obs), base.shape[1]))
    hid = np.zeros((len(probes),) + s2.shape)
    for i, v in enumerate(probes):
        xp = x.copy()
        xp[v] = x[v] + x[v] * delta
        out_p, s2_p = forward64(a, xp, w)
        vec[i] = (out_p - base)[obs] / delta
        hid[i] = (s2_p - s2) / delta
    return vec, hid


@functools.lru_cache(maxsize=None)
def _differences(name, h, c):
    probes, obs = B.node_lists(name)
    return probe_differences(B.graph_of(name).a, B.features(name), B.weights(h, c), probes, obs)


def blas_vectors64(name, h, c):
    """The vectors of probe_differences: the same quantity with the products in whatever order numpy's and scipy's take."""
    return _differences(name, h, c)[0]


# The oracle's own arithmetic.  Its three kinds of product round alike on the CPU: torch.mm (K <= 256) and torch.spmm add every
# output element's terms in index order as ONE chain of fused multiply-adds from zero, and the bias is one more addition
# (measured: such chains reproduce both calls bit for bit; numpy's X W1 does too, scipy's CSR product -- no fma -- and numpy's
# K = 64 product do not).  Two fp64 evaluations of (f(X') - f(X)) / 1e-4 that round differently stand 2e-12 ... 6e-12 of the largest
# score apart (one rounding of a logit of 1.4 over 1e-4 is 1.6e-12), so the restatement below keeps that order.
_SPLIT = 134217729.0          # 2^27 + 1 (Veltkamp)
BLOCK = 1 << 15               # elements of one block of a chain: the temporaries of fma64 stay in cache


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma64(a, b, c):
    """Correctly rounded float64 fma(a, b, c) in numpy (Boldo & Melquiond 2008): the exact product as a pair (Dekker), TwoSum
    with c, the two error terms added with rounding to odd, one final rounding.  No overflow / underflow handling: the values
    here are of order one."""
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    uh = a * b
    ul = al * bl - (((uh - ah * bh) - al * bh) - ah * bl)
    th, tl = _two_sum(c, uh)
    v, e = _two_sum(tl, ul)
    fix = (e != 0) & ((v.view(np.int64) & 1) == 0)
    if fix.any():
        v = np.where(fix, np.nextafter(v, np.where(e > 0, np.inf, -np.inf)), v)
    return th + v


def dense_chain(x, w):
    """x @ w, every element one fma chain over k = 0, 1, ... from zero."""
    out = np.zeros((x.shape[0], w.shape[1]))
    step = max(1, BLOCK // w.shape[1])
    for r0 in range(0, x.shape[0], step):
        xb = x[r0:r0 + step]
        acc = np.zeros((xb.shape[0], w.shape[1]))
        for k in range(w.shape[0]):
            acc = fma64(xb[:, k, None], w[k], acc)
        out[r0:r0 + step] = acc
    return out


def rows_chain(a, rows, gather, width, lead=()):
    """The rows ``rows`` of CSR a times a dense operand, every element one fma chain over the row's entries in column order
    from zero.  ``gather(sel, cols)`` -> [*lead, len(sel), width]: the operand's rows ``cols`` as the rows ``rows[sel]`` see them."""
    rows = np.asarray(rows)
    start, length = a.indptr[rows], a.indptr[rows + 1] - a.indptr[rows]
    acc = np.zeros(tuple(lead) + (len(rows), width))
    by_length = np.argsort(-length, kind="stable")
    step = max(1, BLOCK // (width * int(np.prod(lead, dtype=np.int64))))
    for b0 in range(0, len(rows), step):
        order = by_length[b0:b0 + step]
        ls = length[order]
        part = np.zeros(tuple(lead) + (len(order), width))
        for t in range(int(ls[0])):
            m = int(np.searchsorted(-ls, -t, side="left"))          # the rows of the block with more than t entries
            e = start[order[:m]] + t
            part[..., :m, :] = fma64(a.data[e][:, None], gather(order[:m], a.indices[e]), part[..., :m, :])
        acc[..., order, :] = part
    return acc


def ordered_differences(a, x, w, probes, obs, delta=DELTA):
    """[n_probe, n_obs, C]: (f(X with row v scaled by 1 + delta) - f(X))[u, :] / delta with f = A relu(A X W1 + b1) W2 + b2 in
    float64, every product in the oracle's order (above).  The unperturbed forward once; per probe only what can differ from it --
    row v of X W1, the rows of column v of the pre-activation and of H1 W2, the observed rows -- each a whole chain again: every
    other element has the bits of the unperturbed forward, as in the oracle's two forwards (attacker.py:100-108)."""
    a = B.f32_values(a)
    a.sort_indices()
    x = np.asarray(x, dtype=np.float64)
    w = _w64(w)
    probes, obs = np.asarray(probes), np.asarray(obs)
    s1 = dense_chain(x, w["W1"])
    z1 = rows_chain(a, np.arange(a.shape[0]), lambda sel, col: s1[col], s1.shape[1]) + w["b1"]
    s2 = dense_chain(np.maximum(z1, 0.0), w["W2"])
    C = s2.shape[1]
    out = rows_chain(a, obs, lambda sel, col: s2[col], C) + w["b2"]
    s1p = dense_chain(x[probes] + x[probes] * delta, w["W1"])          # attacker.py:103-105: x_v + x_v delta, two roundings
    csc = a.tocsc()
    csc.sort_indices()
    pi = np.concatenate([np.full(csc.indptr[v + 1] - csc.indptr[v], i) for i, v in enumerate(probes)])
    rr = np.concatenate([csc.indices[csc.indptr[v]:csc.indptr[v + 1]] for v in probes])          # the items (probe, row of its column)
    pv = probes[pi]

    def perturbed_s1(sel, col):
        src = s1[col]
        hit = col == pv[sel]
        src[hit] = s1p[pi[sel][hit]]
        return src

    z1p = rows_chain(a, rr, perturbed_s1, s1.shape[1]) + w["b1"]
    s2all = np.broadcast_to(s2, (len(probes),) + s2.shape).copy()
    s2all[pi, rr] = dense_chain(np.maximum(z1p, 0.0), w["W2"])
    outp = rows_chain(a, obs, lambda sel, col: s2all[:, col], C, lead=(len(probes),)) + w["b2"]
    return (outp - out) / delta


@functools.lru_cache(maxsize=None)
def diff_vectors64(name, h, c):
    """float64 [n_probe, n_obs, C] over B.node_lists(name): (f(X with row v scaled by 1 + DELTA) - f(X))[u, :] / DELTA, in plain
    numpy in the oracle's order of operations (ordered_differences)."""
    probes, obs = B.node_lists(name)
    return ordered_differences(B.graph_of(name).a, B.features(name), B.weights(h, c), probes, obs)


def hidden_differences64(name, h, c):
    return _differences(name, h, c)[1]


# ---- C. the slice limit: a tiny graph -----------------------------------------------------------------------------------------------
TINY_N, TINY_F = 64, 8


@functools.lru_cache(maxsize=None)
def tiny():
    """Erdos-Renyi, n = 64, F = 8: every node observed, every third one probed, one probe twice."""
    from linkteller_amd import graph, synth
    a_hat = graph.first_order_gcn(synth.erdos_renyi_graph(TINY_N, 150, seed=17)).tocsr()
    x = synth.gaussian_features(TINY_N, TINY_F, seed=18)
    probes = np.concatenate([np.arange(0, TINY_N, 3), [6]]).astype(np.int32)
    obs = np.arange(TINY_N, dtype=np.int32)
    return types.SimpleNamespace(a=a_hat, x=x, probes=probes, obs=obs)


@functools.lru_cache(maxsize=None)
def tiny_weights(h, c):
    from linkteller_amd import synth
    return synth.gcn_weights(TINY_F, h, c, seed=h + c)


@functools.lru_cache(maxsize=None)
def tiny_ref64(h, c):
    """The norms of probe_differences on the tiny graph (the oracle's quantity: test_wide2_cpu pins the two on the hub ladder)."""
    t = tiny()
    vec, _ = probe_differences(t.a, t.x, tiny_weights(h, c), t.probes, t.obs)
    return np.linalg.norm(vec, axis=2)


# ---- the exact relations' weights ---------------------------------------------------------------------------------------------------
def relation_weights(kind, control=False):
    """"hidden": H = 300, C = 2 with W2[256:] = 0 -- the second hidden slice contributes exact zeros, the model IS the narrow one
    on W1[:, :256]; "classes": H = 64, C = 12 with W2[:, 8:] = 0 and b2[8:] = 0 -- the second class slice's logits are constant
    zeros, the scores are those of the first 8 classes.  ``control``: the zeroed block holds small random values instead.
    Returns (wide weights, narrow weights)."""
    h, c = (300, 2) if kind == "hidden" else (64, 12)
    w = {k: v.copy() for k, v in B.weights(h, c).items()}
    rng = np.random.RandomState(77)
    if kind == "hidden":
        w["W2"][256:] = (1e-3 * rng.standard_normal((h - 256, c))).astype(np.float32) if control else 0
        narrow = dict(W1=w["W1"][:, :256].copy(), b1=w["b1"][:256].copy(), W2=w["W2"][:256].copy(), b2=w["b2"].copy())
    else:
        w["W2"][:, 8:] = (1e-3 * rng.standard_normal((h, c - 8))).astype(np.float32) if control else 0
        w["b2"][8:] = 0
        narrow = dict(W1=w["W1"].copy(), b1=w["b1"].copy(), W2=w["W2"][:, :8].copy(), b2=w["b2"][:8].copy())
    return w, narrow

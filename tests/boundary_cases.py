"""Constructed "ladder" graphs: rows, columns and member lists of EXACTLY the lengths at which a graph kernel changes its
code path, one below and one above.  Plain numpy / scipy, no GPU; shared by test_boundary_cpu.py (the ladder does what it
claims, and a lost or doubled entry moves the results by far more than the GPU tolerances) and test_boundary_gpu.py.

The graphs are directed CSR matrices with columns strictly increasing inside each row (the ABI takes any such matrix).
  * a filler POOL of 3000 nodes; every pool row holds a self loop (0.5), two random pool entries and an entry of 0.5 in
    the column of one of N_ANCHOR anchor probes t_j (j = row mod N_ANCHOR): every pool node is one strong hop from a probe,
    so every entry of a ladder row reaches the influence matrix (pair (t_j, u_d)) with a weight that does not shrink with d;
  * row-ladder nodes u_d: a row of exactly d entries, all in the pool (their columns are empty);
  * column-ladder nodes v_c: a column of exactly c entries, all in pool rows (their rows are empty);
  * (hub_ladder) member-ladder probes w_m: a column that meets row(u_1025) in exactly m entries, the rest of it outside
    that row; one "heavy" copy (a column of 600 entries: more than LT_BIG_RV, a bitmap slot) and one "tight" copy (m + 28
    entries: at most 93 up to m = 65, which stageB_long_block counts as light against the 1025-entry row even with a bitmap
    row -- cnt * 11 <= 1025, lt_influence.hip:1006-1009 -- and searches from the short side; without a bitmap row every tight
    copy is light, and the lists of 129 and 257 members are refilled).  The members sit at unweighted positions of the hub
    row and a member carries 1 / (m + 28) of its column in either copy, so the member-ladder cells (w_m, u_1025) are sums of like terms and one lost
    member shows in its cell (test_boundary_cpu.test_mutation_margin_of_the_member_ladder).
Weights: in a ladder row of more than 10 entries the entries at the positions a cut can lose -- 0, d - 1, 127, 128, the last
segment's first entry and the one before it, 1023, 1024 -- carry SPECIAL_SHARE = 0.1 each (0.05 left the fp32 modes' margin of
test_boundary_cpu.py below 4) and the others share the remainder equally; shorter rows carry 1 / d per entry (>= 0.1).  Every ladder row sums to 1, so ladder rows give outputs of one magnitude whatever their
length.  Ladder columns get the same treatment at the same positions of the CSC order.
"""
import functools
import types

import numpy as np
import scipy.sparse as sp

# The constants the ladders are cut at, restated once with their source lines (linkteller_amd/csrc/).
LT_ROW_SEG = 128       # lt_internal.h:63      rows longer than this are hubs, summed in segments of this many entries
LT_L2_CHUNK = 1024     # lt_forward.hip:155    layer 2 stages a hub row this many entries at a time
LT_SB_SHORT = 32       # lt_influence.hip:2087 stage B of SPARSE / DELTA: another loop for rows up to this length
LT_SB_PASS = 2048      # lt_influence.hip:2089 probes per pass of a k_item_stageB_rows block
LT_SBL_MC = 128        # lt_influence.hip:932  members of a light probe kept in LDS at a time
LT_BIG_RV = 512        # lt_items.hip.h:55     a probe column longer than this gets a bitmap slot
LT_BIG_SLOTS = 64      # lt_items.hip.h:56
LT_DL_MAX_T = 4096     # lt_core.hip:201       incidences of one node up to which a graph keeps its records
TILE_CLASS = 16        # lt_core.hip:533       the tiled SpMM sorts rows into classes of this many entries
LT_ERR_UNSUPPORTED = -3

POWERS = (8, 16, 32, 64, 128, 256, 512, 1024, 2048)      # TILE_CLASS / 2 .. 2 LT_L2_CHUNK: every constant above is among them
LADDER = tuple(sorted({0, 1, 2, 383, 384, 385} | {k + s for k in POWERS for s in (-1, 0, 1)}))
MEMBERS = (0, 1, 63, 64, 65, 120, 127, 128, 129, 257)
HUB = 1025             # the observed hub of the member ladder: one stage-B chunk of C = 2 plus one entry
N_POOL = 3000
N_ANCHOR = 10
F = 32
SPECIAL_SHARE = 0.1
MODEL_SHAPES = ((24, 2), (64, 3), (256, 8))      # (H, C): the three class-count buckets of stageB_long_block


def special_positions(d):
    """The positions of a d-entry row (or column) that a cut can lose."""
    last = (d - 1) // LT_ROW_SEG * LT_ROW_SEG if d > 0 else 0
    cand = (0, d - 1, LT_ROW_SEG - 1, LT_ROW_SEG, last - 1, last, LT_L2_CHUNK - 1, LT_L2_CHUNK)
    return sorted({p for p in cand if 0 <= p < d})


def ladder_weights(d):
    if d == 0:
        return np.zeros(0)
    if d <= 10:
        return np.full(d, 1.0 / d)
    sp_ = special_positions(d)
    w = np.full(d, (1.0 - SPECIAL_SHARE * len(sp_)) / (d - len(sp_)))
    w[sp_] = SPECIAL_SHARE
    return w


def _build(row_lengths, col_lengths, members, seed, top_incidences=None):
    rng = np.random.RandomState(seed)
    n_row, n_col = len(row_lengths), len(col_lengths)
    u0, v0 = N_POOL, N_POOL + n_row
    w0 = v0 + n_col
    t0 = w0 + 2 * len(members)
    n = t0 + N_ANCHOR
    rows, cols, vals = [], [], []

    def add(r, c, v):
        rows.append(np.broadcast_to(np.asarray(r), np.shape(v)).ravel())
        cols.append(np.broadcast_to(np.asarray(c), np.shape(v)).ravel())
        vals.append(np.asarray(v, dtype=np.float64).ravel())

    pool = np.arange(N_POOL)
    add(pool, pool, np.full(N_POOL, 0.5))
    for k in (1, 2):          # two more pool entries per pool row, never the diagonal, never twice
        add(pool, (pool + rng.randint(1, N_POOL // 2, N_POOL) + (k - 1) * (N_POOL // 2)) % N_POOL, rng.uniform(0.05, 0.25, N_POOL))
    add(pool, t0 + pool % N_ANCHOR, np.full(N_POOL, 0.5))
    u = {d: u0 + i for i, d in enumerate(row_lengths)}
    v = {c: v0 + i for i, c in enumerate(col_lengths)}
    row_sets = {}
    for d in row_lengths:
        row_sets[d] = np.sort(rng.choice(N_POOL, d, replace=False))
        add(u[d], row_sets[d], ladder_weights(d))
    col_sets = {}
    for c in col_lengths:
        col_sets[c] = np.sort(rng.choice(N_POOL, c, replace=False))
        add(col_sets[c], v[c], ladder_weights(c))
    w = {}
    if members:
        hub = row_sets[HUB]
        outside = np.setdiff1d(pool, hub)
        plain = np.setdiff1d(np.arange(HUB), special_positions(HUB))
        for i, m in enumerate(members):
            for j, (kind, total) in enumerate((("heavy", 600), ("tight", m + 28))):
                node = w0 + 2 * i + j
                pos = rng.choice(plain, m, replace=False)
                col = np.concatenate([hub[pos], rng.choice(outside, total - m, replace=False)])
                # a member carries 1 / (m + 28) in either copy, the other entries share the rest: the column sums to 1
                add(col, node, np.concatenate([np.full(m, 1.0 / (m + 28)), np.full(total - m, 28.0 / (m + 28) / (total - m))]))
                w[(m, kind)] = node
    a = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    a.sum_duplicates()
    assert a.nnz == sum(len(x) for x in vals), "an entry was drawn twice"
    if top_incidences is not None:
        a = _raise_incidences(a, v[max(col_lengths)], [v[c] for c in col_lengths if c != max(col_lengths)], top_incidences, rng)
    a.sort_indices()
    return types.SimpleNamespace(a=a, n=n, u=u, v=v, w=w, t=list(range(t0, n)), row_sets=row_sets, col_sets=col_sets, seed=seed)


def incidences(a):
    """Per node v: the sum over the rows r of column v of the length of column r (lt_core.hip:229-246)."""
    pat = sp.csr_matrix((np.ones(a.nnz), a.indices, a.indptr), shape=a.shape)
    col_len = np.asarray(pat.sum(axis=0)).ravel()
    return np.asarray(pat.T @ col_len).ravel().astype(np.int64)


def _raise_incidences(a, node, others, target, rng):
    """Pool entries (q, r) with r a row of column `node` and of no other ladder column, until `node` sits at `target` incidences."""
    csc = a.tocsc()
    mine = csc.indices[csc.indptr[node]:csc.indptr[node + 1]]
    taken = np.unique(np.concatenate([csc.indices[csc.indptr[o]:csc.indptr[o + 1]] for o in others]))
    mine = np.setdiff1d(mine, taken)
    need = target - int(incidences(a)[node])
    assert need > 0 and len(mine) > 0
    lil = a.tolil()
    k = 0
    while need > 0:
        r = int(mine[k % len(mine)])
        q = int(rng.randint(0, N_POOL))
        k += 1
        if lil[q, r] == 0:
            lil[q, r] = rng.uniform(0.05, 0.25)
            need -= 1
    return sp.csr_matrix(lil)


@functools.lru_cache(maxsize=None)
def hub_ladder():
    """The full ladder on both sides, the member ladder on u_1025."""
    return _build(LADDER, LADDER, MEMBERS, seed=11)


@functools.lru_cache(maxsize=None)
def short_ladder_at(top_incidences):
    g = _build(tuple(d for d in LADDER if d <= LT_ROW_SEG), tuple(c for c in LADDER if c <= LT_BIG_RV + 1), (), seed=12,
               top_incidences=top_incidences)
    assert np.diff(g.a.indptr).max() == LT_ROW_SEG
    return g


def short_ladder():
    """Rows up to and including exactly 128 entries and none longer (the graph keeps its incidence records: the fused DELTA route
    and the packed host landing apply); columns up to 513 entries; the node of the longest column sits at 4050 incidences
    (short_ladder_at(4096) / (4097): the same graph with that node at the cap and one past it)."""
    return short_ladder_at(4050)


def csr32(g):
    """The arrays lt_graph_create / lt_graph_records_host take."""
    a = g.a.astype(np.float32)
    return (g.n, a.nnz, np.ascontiguousarray(a.indptr, dtype=np.int32), np.ascontiguousarray(a.indices, dtype=np.int32),
            np.ascontiguousarray(a.data, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def pool_nodes(name):
    """The pool nodes probed AND observed: those at the weighted positions of the rows of 129, 257 and 1025 entries and at the
    positions next to them (through its self loop such a node is a member of its own column: the pair (node, u_d) then reads
    that one entry of row u_d), the rows of the last two CSC entries of the columns of 129 and 513 entries, and a few more."""
    g = hub_ladder() if name == "hub" else short_ladder()
    picks = []
    for d in (129, 257, 1025):
        if d in g.row_sets:
            picks += [int(g.row_sets[d][q]) for p in special_positions(d) for q in (p, p + 1 if p + 1 < d else p - 1)]
    for c in (129, 513):
        picks += [int(g.col_sets[c][-1]), int(g.col_sets[c][-2])]
    if name != "hub":
        picks += [int(g.row_sets[128][p]) for p in special_positions(128)]
    extra = np.random.RandomState(5).choice(N_POOL, 6, replace=False)
    return np.unique(np.concatenate([picks, extra])).astype(np.int32)


@functools.lru_cache(maxsize=None)
def node_lists(name):
    """(probes, observed) of the influence tests: all column-ladder nodes, the member-ladder probes, the anchors and the pool nodes; all
    row-ladder nodes, the pool nodes, and u_1025 a second time."""
    g = hub_ladder() if name == "hub" else short_ladder()
    pn = pool_nodes(name)
    probes = np.concatenate([[g.v[c] for c in sorted(g.v)], [g.w[k] for k in sorted(g.w)], g.t, pn]).astype(np.int32)
    obs = np.concatenate([[g.u[d] for d in sorted(g.u)], pn, [g.u[HUB]] if HUB in g.u else []]).astype(np.int32)
    return probes, obs


@functools.lru_cache(maxsize=None)
def features(name):
    from linkteller_amd import synth
    g = hub_ladder() if name == "hub" else short_ladder()
    return synth.gaussian_features(g.n, F, seed=21)


@functools.lru_cache(maxsize=None)
def weights(h, c):
    from linkteller_amd import synth
    return synth.gcn_weights(F, h, c, seed=h + c)


def mutate(a, row, pos, kind):
    """A copy of CSR `a` with entry `pos` of row `row` removed ("drop"), or its weight added onto the next entry of the row
    (the previous one for the last entry) ("double"): what a kernel that loses an entry, or counts one twice, computes."""
    b = a.copy()
    e0, e1 = b.indptr[row], b.indptr[row + 1]
    assert 0 <= pos < e1 - e0
    if kind == "drop":
        b.data[e0 + pos] = 0.0
    else:
        assert e1 - e0 > 1
        b.data[e0 + (pos + 1 if pos + 1 < e1 - e0 else pos - 1)] += b.data[e0 + pos]
    return b


def mutate_column(a, col, pos, kind):
    """The same on entry `pos` (CSC order) of column `col`."""
    return sp.csr_matrix(mutate(sp.csr_matrix(a.T), col, pos, kind).T)


# ---- references, computed once per process --------------------------------------------------------------------------------
DELTA = 1e-4


def graph_of(name):
    return hub_ladder() if name == "hub" else short_ladder()


def f32_values(a):
    """The adjacency as the device holds it: values rounded to float32 (graph.csr_arrays), as float64."""
    return sp.csr_matrix(a).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def oracle_matrix(name, h, c, dtype_name):
    """The reference's influence matrix over node_lists(name), verbatim op order (oracle.get_gradient_eps_mat), in float64 or
    float32."""
    import torch
    from oracle import linkteller_oracle as O
    torch.set_num_threads(1)
    dtype = getattr(torch, dtype_name)
    g = graph_of(name)
    probes, obs = node_lists(name)
    adj_t = O.to_torch_sparse(g.a).to(dtype)
    P = {k: torch.from_numpy(v).to(dtype) for k, v in weights(h, c).items()}
    xt = torch.from_numpy(features(name)).to(dtype)
    out = np.zeros((len(probes), len(obs)))
    idx = torch.as_tensor(obs.astype(np.int64))
    with torch.no_grad():
        for i, v in enumerate(probes):
            out[i] = O.get_gradient_eps_mat(xt, adj_t, P, int(v), DELTA)[idx].norm(dim=1).double().numpy()
    return out


@functools.lru_cache(maxsize=None)
def oracle_logits(name, h, c):
    import torch
    from oracle import linkteller_oracle as O
    g = graph_of(name)
    P = {k: torch.from_numpy(v).double() for k, v in weights(h, c).items()}
    return O.gcn_forward(torch.from_numpy(features(name)).double(), O.to_torch_sparse(g.a).double(), P).numpy()


SPMM_COLS = (8, 64, 256)


@functools.lru_cache(maxsize=None)
def spmm_inputs(name, ncols):
    """(S, bias, A S in float64) of the SpMM tests.  |S| in [0.5, 1.5] with random signs: no entry of a row meets a value so
    small that losing it would not show; a bias of the size of a ladder row's sums, so that the ReLU clamps by the row."""
    g = graph_of(name)
    rng = np.random.RandomState(100 + ncols)
    s = (rng.uniform(0.5, 1.5, (g.n, ncols)) * rng.choice([-1.0, 1.0], (g.n, ncols))).astype(np.float32)
    b = (0.15 * rng.standard_normal(ncols)).astype(np.float32)
    return s, b, f32_values(g.a) @ s.astype(np.float64)


def spmm_want(name, ncols, epilogue):
    s, b, prod = spmm_inputs(name, ncols)
    return np.maximum(prod + b, 0) if epilogue else prod


def ladder_rows(g):
    """[(d, node)] of the row ladder."""
    return sorted(g.u.items())


# ---- the training cases: one epoch on hub_ladder, dropout 0 (the backward walks the columns: the column ladder) ---------------
TRAIN2_SHAPE = (64, 3)
TRAIN3_SHAPE = (32, 16, 2)


@functools.lru_cache(maxsize=None)
def train_case2():
    """A case dict in the form of train_cases.make."""
    import train_cases as K
    g = hub_ladder()
    h, c = TRAIN2_SHAPE
    w = weights(h, c)
    y = np.random.RandomState(31).randint(0, c, g.n).astype(np.int64)
    return dict(name="hub_ladder", adj=K._f32(g.a), x=features("hub"), y=y, params=[w[k] for k in ("W1", "b1", "W2", "b2")], p=0.0,
                n=g.n, F=F, H=h, C=c)


@functools.lru_cache(maxsize=None)
def train_case3():
    """A case dict in the form of train3_cases.make."""
    import train_cases as K
    import train3_cases as K3
    g = hub_ladder()
    h1, h2, c = TRAIN3_SHAPE
    y = np.random.RandomState(32).randint(0, c, g.n).astype(np.int64)
    return dict(name="hub_ladder3", adj=K._f32(g.a), x=features("hub"), y=y, params=K3.init_params(F, h1, h2, c, seed=3), p=0.0,
                n=g.n, F=F, H1=h1, H2=h2, C=c)


def params3():
    return dict(zip(("W1", "b1", "W2", "b2", "W3", "b3"), train_case3()["params"]))


@functools.lru_cache(maxsize=None)
def oracle_matrix3(dtype_name):
    """The 3-layer reference over node_lists("hub") with the parameters of train_case3, verbatim op order."""
    import torch
    from oracle import linkteller_oracle as O
    torch.set_num_threads(1)
    dtype = getattr(torch, dtype_name)
    g = hub_ladder()
    probes, obs = node_lists("hub")
    adj_t = O.to_torch_sparse(g.a).to(dtype)
    P = {k: torch.from_numpy(v).to(dtype) for k, v in params3().items()}
    xt = torch.from_numpy(features("hub")).to(dtype)
    out = np.zeros((len(probes), len(obs)))
    idx = torch.as_tensor(obs.astype(np.int64))
    with torch.no_grad():
        for i, v in enumerate(probes):
            out[i] = O.get_gradient_eps_mat(xt, adj_t, P, int(v), DELTA, forward=O.gcn3_forward)[idx].norm(dim=1).double().numpy()
    return out


def canonical_spmm_rows(name, ncols, epilogue, rows):
    """{row: float32 [ncols]}: the documented canonical order of lt_spmm_csr_f32 restated in numpy (lt_rows.hip.h:68-71,
    lt_spmm.hip): fmaf chains of LT_ROW_SEG entries in entry order, each from +0; the chains added in segment order; then the
    bias; then the ReLU."""
    from train_restate import fma32
    g = graph_of(name)
    a = g.a.astype(np.float32)
    s, b, _ = spmm_inputs(name, ncols)
    out = {}
    for r in rows:
        e0, e1 = a.indptr[r], a.indptr[r + 1]
        total = None
        for s0 in range(e0, max(e1, e0 + 1), LT_ROW_SEG):
            acc = np.zeros(ncols, dtype=np.float32)
            for e in range(s0, min(e1, s0 + LT_ROW_SEG)):
                acc = fma32(a.data[e], s[a.indices[e]], acc)
            total = acc if total is None else (total + acc).astype(np.float32)
        if epilogue:
            total = np.maximum((total + b).astype(np.float32), np.float32(0))
        out[r] = total
    return out


def member_cells():
    """(rows, column) of the member ladder in the matrix over node_lists("hub"): the probes w_m against the first u_1025."""
    g = hub_ladder()
    probes, obs = node_lists("hub")
    rows = np.array([int(np.flatnonzero(probes == g.w[k])[0]) for k in sorted(g.w)])
    return rows, int(np.flatnonzero(obs == g.u[HUB])[0])

"""The wide-class GCN3 attack (lt_baseline3_create_wide, 9 .. 256 classes; LT_MODE_DELTA through the probe primitive) on the GPU.

The oracle is oracle.linkteller_oracle.influence_matrix(..., forward=gcn3_forward) on float64 tensors with influence = 1e-4: called
on the list (probes ++ observed) with probe_range = the probes, the block [probes, observed] read out of it.  The bound is the
project's bound for narrow GCN3 `delta`: |ours - ref64|.max() <= 1e-5 * ref64.max(), and exact zeros where the oracle has them.

Graphs (F = 32): an Erdos-Renyi graph (n = 300, 600 edges: between a tenth and nine tenths of its fp64 cells are exact zeros,
asserted, so the zero check has something to show), a graph with an isolated node and self loops (n = 120), and the hub ladder of
boundary_cases.py (n = 3096: rows of 129 .. 2049 entries; a handful of its probes and observed rows).  Node lists: a probe whose
feature row is all zero, u == v, a repeated probe, a repeated observed id, an observed list that is not the probe list."""
import argparse
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import boundary_cases as B
from conftest import GOLDEN, csr_from
from linkteller_amd import _lib

pytestmark = pytest.mark.gpu

F = 32
DELTA = 1e-4
SHAPES = ((16, 12, 9), (16, 12, 41), (32, 16, 121), (256, 64, 256), (20, 12, 8))
GRAPHS = ("er", "loops", "hub")
KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")
LT_ERR_INVALID, LT_ERR_UNSUPPORTED, LT_ERR_WORKSPACE = -1, -3, -4


# ---- cases, built once per process ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(name):
    """(normalised adjacency as float32 CSR, float32 features, probes, observed)."""
    from linkteller_amd import graph, synth
    if name == "hub":
        g = B.hub_ladder()
        a_hat = sp.csr_matrix(g.a).astype(np.float32)
        x = B.features("hub").copy()
        pool = B.pool_nodes("hub")
        # columns of 129 / 513 entries, a member-ladder probe, an anchor, pool nodes; rows of 129 / 257 / 1025 entries
        probes = [g.v[129], g.v[513], g.w[(129, "heavy")], g.t[0], int(pool[0]), int(pool[1]), int(pool[2]), int(pool[0])]
        obs = [g.u[129], g.u[257], g.u[1025], int(pool[0]), int(pool[3]), int(pool[4]), g.u[1025], g.u[1]]
        zero = int(pool[2])
    else:
        n, m, seed = (300, 600, 3) if name == "er" else (120, 260, 4)
        rng = np.random.RandomState(seed)
        a = sp.lil_matrix((n, n))
        while a.nnz < 2 * m:
            i, j = rng.randint(0, n, 2)
            if i != j:
                a[i, j] = a[j, i] = 1.0
        if name == "loops":
            a[5, :] = 0
            a[:, 5] = 0                              # node 5 is isolated
            for i in (0, 7, 40):
                a[i, i] = 1.0                        # self loops in the raw adjacency
        a_hat = sp.csr_matrix(graph.first_order_gcn(sp.csr_matrix(a))).astype(np.float32)
        a_hat.sort_indices()
        x = synth.gaussian_features(n, F, seed=seed + 10).copy()
        pick = rng.choice(n, 44, replace=False)
        probes = list(pick[:24]) + [int(pick[3])]                           # a repeated probe
        obs = list(pick[12:44]) + [int(pick[20]), int(pick[40])]            # overlaps the probes (u == v), repeated ids
        if name == "loops":
            probes += [5, 0, 7]
            obs += [5, 0, 40]
        zero = int(pick[1])
    x[zero] = 0.0                                     # a probe whose feature row is all zero
    probes, obs = np.asarray(probes, dtype=np.int32), np.asarray(obs, dtype=np.int32)
    assert zero in probes and set(probes) & set(obs) and len(set(probes)) < len(probes) and len(set(obs)) < len(obs)
    return a_hat, np.ascontiguousarray(x, dtype=np.float32), probes, obs, int(np.flatnonzero(probes == zero)[0])


@functools.lru_cache(maxsize=None)
def _params(shape, seed=0):
    h1, h2, c = shape
    rng = np.random.RandomState(1000 * seed + h1 + 3 * h2 + 7 * c)
    out = {}
    for i, (fi, fo) in enumerate(((F, h1), (h1, h2), (h2, c)), start=1):
        s = 1.0 / np.sqrt(fo)                          # GraphConvolution.reset_parameters (gcn/layers.py)
        out[f"W{i}"] = rng.uniform(-s, s, (fi, fo)).astype(np.float32)
        out[f"b{i}"] = rng.uniform(-s, s, fo).astype(np.float32)
    return out


def _oracle(a_hat, x, params, probes, obs):
    from oracle import linkteller_oracle as O
    torch.set_num_threads(min(16, torch.get_num_threads()))
    nodes = np.concatenate([probes, obs]).astype(np.int64)
    P = {k: torch.from_numpy(np.asarray(v)).double() for k, v in params.items()}
    full = O.influence_matrix(torch.from_numpy(x).double(), O.to_torch_sparse(a_hat).double(), P, nodes, DELTA,
                              forward=O.gcn3_forward, probe_range=range(len(probes)))
    return full[:len(probes), len(probes):]


@functools.lru_cache(maxsize=None)
def _ref64(name, shape):
    a_hat, x, probes, obs, _ = _graph(name)
    return _oracle(a_hat, x, _params(shape), probes, obs)


def _wide3(*a):
    """engine.Baseline3 made through lt_baseline3_create_wide whatever the class count."""
    from linkteller_amd import engine

    class Wide3(engine.Baseline3):
        NARROW_MAX_C = 0
    return Wide3(*a)


def _baseline(name, shape, gpu, params=None):
    from linkteller_amd import engine, graph
    a_hat, x, *_ = _graph(name)
    p = params or _params(shape)
    dev = [torch.from_numpy(np.asarray(p[k])).to(gpu) for k in KEYS]
    base = _wide3(graph.HipGraph(a_hat), torch.from_numpy(x).to(gpu), *dev)
    assert base.wide and isinstance(base, engine.Baseline3)
    return base, dev


def _rows(base, probes, obs):
    return base.influence_rows(probes, obs, DELTA, "delta").cpu().numpy().astype(np.float64)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------
def test_engine_makes_a_wide_handle_above_eight_classes(gpu):
    from linkteller_amd import engine, graph
    a_hat, x, probes, obs, _ = _graph("er")
    hg, xt = graph.HipGraph(a_hat), torch.from_numpy(x).to(gpu)
    wide = engine.Baseline3(hg, xt, *[torch.from_numpy(_params((16, 12, 9))[k]).to(gpu) for k in KEYS])
    narrow = engine.Baseline3(hg, xt, *[torch.from_numpy(_params((20, 12, 8))[k]).to(gpu) for k in KEYS])
    assert wide.wide and not narrow.wide
    for mode in ("sparse", "full", None):
        with pytest.raises(NotImplementedError):
            wide.influence_rows(probes, obs, DELTA, mode) if mode else wide.influence_rows(probes, obs, DELTA)
    # the narrow and the wide kernels on the same 8-class model: the same fp64 quantity
    ref = _ref64("er", (20, 12, 8))
    got = narrow.influence_rows(probes, obs, DELTA, "delta").cpu().numpy().astype(np.float64)
    assert np.abs(got - ref).max() <= 1e-5 * ref.max()


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_delta_parity_with_the_fp64_oracle(gpu, name, shape):
    ref = _ref64(name, shape)
    _, _, probes, obs, zrow = _graph(name)
    zeros = float((ref == 0).mean())
    if name == "er":
        assert 0.1 <= zeros <= 0.9, zeros              # a condition of the zero check below, not a measurement
    base, _ = _baseline(name, shape, gpu)
    got = _rows(base, probes, obs)
    err = np.abs(got - ref).max() / ref.max()
    print(f"gcn3w {name} {shape}: max {ref.max():.3g} zeros {zeros:.2f} |ours - ref64| / max = {err:.2e}")
    assert ref.max() > 0 and np.isfinite(got).all()
    assert err <= 1e-5
    assert np.all(got[ref == 0] == 0) and not np.signbit(got).any()
    assert np.all(ref[zrow] == 0) and np.all(got[zrow] == 0)      # the all-zero feature row: nothing to perturb
    from linkteller_amd import engine
    torch.cuda.synchronize()
    engine.node_check()


# ---- 2. chunk invariance -------------------------------------------------------------------------------------------------------
def test_chunking_subsets_and_runs_give_the_same_bits(gpu):
    shape = (16, 12, 41)
    a_hat, x, probes, obs, _ = _graph("er")
    base, _ = _baseline("er", shape, gpu)
    lib = _lib.lib()
    one = base.influence_rows(probes, obs, DELTA, "delta").clone()
    assert torch.equal(base.influence_rows(probes, obs, DELTA, "delta"), one)                 # two runs
    need1 = lib.lt_influence3_workspace_bytes(base._h, 1, len(obs))
    need_all = lib.lt_influence3_workspace_bytes(base._h, len(probes), len(obs))
    assert need_all > 8 * need1                      # the default budget takes all the probes in one chunk
    try:
        for budget in (1, 2 * need1):
            _lib.set_tuning("chunk_budget_bytes", budget)
            need = lib.lt_influence3_workspace_bytes(base._h, len(probes), len(obs))
            assert need < 4 * need1, (budget, need, need1)                                   # chunks of 1 .. 3 probes
            assert torch.equal(base.influence_rows(probes, obs, DELTA, "delta"), one), budget
    finally:
        _lib.set_tuning("chunk_budget_bytes", None)
    sel = np.array([9, 2, 24, 2, 17])
    assert torch.equal(base.influence_rows(probes[sel], obs, DELTA, "delta"), one[torch.from_numpy(sel).to(gpu)])
    cols = np.array([30, 1, 1, 12])
    assert torch.equal(base.influence_rows(probes, obs[cols], DELTA, "delta"), one[:, torch.from_numpy(cols).to(gpu)])


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
def _raw_create(gpu, hg, xt, shape, fn="lt_baseline3_create_wide"):
    h1, h2, c = shape
    t = [torch.zeros(s, device=gpu) for s in ((F, h1), (h1,), (h1, h2), (h2,), (h2, c), (c,))]
    h = C.c_void_p()
    rc = getattr(_lib.lib(), fn)(hg.handle, xt.data_ptr(), F, F, t[0].data_ptr(), t[1].data_ptr(), h1, t[2].data_ptr(), t[3].data_ptr(),
                                 h2, t[4].data_ptr(), t[5].data_ptr(), c, None, C.byref(h))
    return rc, h, _lib.lib().lt_last_error().decode()


def test_refusals(gpu):
    from linkteller_amd import engine, graph
    lib = _lib.lib()
    a_hat, x, probes, obs, _ = _graph("loops")
    n = a_hat.shape[0]
    hg, xt = graph.HipGraph(a_hat), torch.from_numpy(x).to(gpu)
    for shape in ((16, 12, 257), (16, 257, 41), (257, 12, 41)):
        rc, h, msg = _raw_create(gpu, hg, xt, shape)
        assert rc == LT_ERR_UNSUPPORTED and not h.value and "lt_baseline3_create_wide" in msg
    rc, h, msg = _raw_create(gpu, hg, xt, (16, 12, 9), fn="lt_baseline3_create")           # the narrow entry keeps its limit
    assert rc == LT_ERR_UNSUPPORTED and not h.value and "C <= 8" in msg
    rc, h, _ = _raw_create(gpu, hg, xt, (16, 12, 256))
    assert rc == 0 and h.value
    assert lib.lt_baseline3_destroy(h) == 0

    base, _ = _baseline("loops", (16, 12, 41), gpu)
    pt, ot = torch.from_numpy(probes).to(gpu), torch.from_numpy(obs).to(gpu)
    npb, nob = len(probes), len(obs)
    need = lib.lt_influence3_workspace_bytes(base._h, npb, nob)
    ws = engine._workspace(need, gpu)
    out = torch.full((npb, nob), 7.0, device=gpu)

    def call(mode, ws_bytes=None):
        return lib.lt_influence3_rows_mode(base._h, pt.data_ptr(), npb, ot.data_ptr(), nob, DELTA, mode, out.data_ptr(), nob,
                                           ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, engine._stream())
    assert call(_lib.MODE_DELTA) == LT_ERR_INVALID and "lt_baseline3_enable_fp64" in lib.lt_last_error().decode()
    for mode in (_lib.MODE_SPARSE, _lib.MODE_FULL):
        assert call(mode) == LT_ERR_UNSUPPORTED and "wide handle" in lib.lt_last_error().decode()
    assert lib.lt_influence3_rows(base._h, pt.data_ptr(), npb, ot.data_ptr(), nob, DELTA, out.data_ptr(), nob, ws.data_ptr(), ws.numel(),
                                  engine._stream()) == LT_ERR_UNSUPPORTED
    assert "wide handle" in lib.lt_last_error().decode()
    base.enable_fp64()
    assert call(_lib.MODE_SPARSE) == LT_ERR_UNSUPPORTED          # ... with the fp64 baseline too
    assert call(_lib.MODE_DELTA, ws_bytes=need - 256) == LT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                               # nothing was enqueued by any of them
    assert call(_lib.MODE_DELTA) == 0
    torch.cuda.synchronize()
    good = out.clone()
    assert np.array_equal(good.cpu().numpy(), base.influence_rows(probes, obs, DELTA, "delta").cpu().numpy())
    engine.node_check()
    # ids out of range: replaced by node 0 on the device (no access out of bounds: the call completes), reported afterwards
    for which, bad in (("probe", n), ("observed", n + 12345), ("probe", -1), ("observed", 2 ** 31 - 1)):
        p2, o2 = probes.copy(), obs.copy()
        (p2 if which == "probe" else o2)[2] = bad
        got = base.influence_rows(torch.from_numpy(p2).to(gpu), torch.from_numpy(o2).to(gpu), DELTA, "delta")
        torch.cuda.synchronize()
        assert torch.isfinite(got).all()
        with pytest.raises(IndexError):
            engine.node_check()
        engine.node_check()
    assert torch.equal(base.influence_rows(pt, ot, DELTA, "delta"), good)
    torch.cuda.synchronize()
    engine.node_check()


# ---- 4. baseline ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 12, 9), (32, 16, 121), (20, 12, 8)], ids=lambda s: "x".join(map(str, s)))
def test_wide_logits_and_refresh(gpu, shape):
    from oracle import linkteller_oracle as O
    a_hat, x, probes, obs, _ = _graph("er")
    base, dev = _baseline("er", shape, gpu)

    def ref_logits(p):
        return O.gcn3_forward(torch.from_numpy(x).double(), O.to_torch_sparse(a_hat).double(),
                              {k: torch.from_numpy(np.asarray(v)).double() for k, v in p.items()}).numpy()
    ref = ref_logits(_params(shape))
    got = base.logits().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6      # test_gpu_parity's bound
    before = _rows(base, probes, obs)
    # an in-place update of every layer + refresh(): logits and rows follow the new weights
    new = _params(shape, seed=1)
    with torch.no_grad():
        for t, k in zip(dev, KEYS):
            t.copy_(torch.from_numpy(new[k]))
    base.refresh()
    ref2 = ref_logits(new)
    got2 = base.logits().cpu().numpy().astype(np.float64)
    assert np.abs(got2 - ref2).max() <= 2e-5 * np.abs(ref2).max() + 1e-6
    rows_ref = _oracle(a_hat, x, new, probes, obs)
    after = _rows(base, probes, obs)
    assert np.abs(after - rows_ref).max() <= 1e-5 * rows_ref.max() and np.all(after[rows_ref == 0] == 0)
    assert np.abs(after - before).max() > 1e-3 * rows_ref.max()


# ---- 5. attacker ---------------------------------------------------------------------------------------------------------------
def test_attacker_takes_the_wide_handle(gpu, tmp_path, monkeypatch):
    from linkteller_amd import engine, graph
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN3
    from oracle import linkteller_oracle as O
    g = np.load(os.path.join(GOLDEN, "next_rows.npz"), allow_pickle=False)
    a = csr_from(g, "adj")
    x = torch.from_numpy(g["x"]).to(gpu)
    adj_t = graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(a)).to(gpu)
    w = types.SimpleNamespace(features_2=x, adj_2=adj_t, adj_ori=a, n_nodes=a.shape[0])
    torch.manual_seed(7)
    model = GCN3(x.shape[1], 16, 12, 41, 0.5).to(gpu).eval()
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("LT_INFLUENCE_MODE", raising=False)
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=32, sample_seed=42, influence=DELTA,
                              mode="vanilla-clean", attack_mode="efficient")
    atk = Attacker(args, model, w)
    atk.prepare_test_data()
    assert atk._walk()[0] == "gcn3w" and not atk._is_three_layer()
    nodes = np.asarray(atk.test_nodes, dtype=np.int64)
    mat = atk.influence_matrix()
    assert atk.baseline3().wide
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    own = engine.Baseline3(atk.adj, atk.features, *[sd[f"gc{i}.{p}"] for i in (1, 2, 3) for p in ("weight", "bias")])
    want = own.influence_rows(nodes, nodes, DELTA, "delta").cpu().numpy().astype(np.float64)
    assert mat.dtype == np.float64 and np.array_equal(mat, want) and mat.max() > 0
    assert np.array_equal(atk.influence_matrix("delta"), mat)
    # `sparse` / `full` stay the loop over the unfused layers, bit for bit
    loop = atk._rows_generic(nodes, nodes).cpu().numpy().astype(np.float64)
    assert np.array_equal(atk.influence_matrix("sparse"), loop) and np.array_equal(atk.influence_matrix("full"), loop)
    assert not np.array_equal(loop, mat)
    monkeypatch.setenv("LT_INFLUENCE_MODE", "sparse")             # the switch that keeps the old numbers
    assert np.array_equal(atk.influence_matrix(), loop)
    monkeypatch.delenv("LT_INFLUENCE_MODE")
    # the fp64 oracle on the same model
    P = {k: sd[n].double().cpu() for k, n in zip(KEYS, ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias", "gc3.weight", "gc3.bias"))}
    ref = O.influence_matrix(x.double().cpu(), O.to_torch_sparse(O.first_order_gcn(a)).double(), P, nodes, DELTA, forward=O.gcn3_forward)
    assert np.abs(mat - ref).max() <= 1e-5 * ref.max() and np.all(mat[ref == 0] == 0)
    # evaluate(): the metrics of the matrix's cells
    ind = {int(v): i for i, v in enumerate(nodes)}

    def cells(pairs):       # perturb v, observe u (attacker.py:236-245)
        return [mat[ind[int(v)], ind[int(u)]] for u, v in np.asarray(pairs).reshape(-1, 2)]
    m = O.attack_metrics(cells(atk.exist_edges), cells(atk.nonexist_edges))
    out = atk.evaluate()
    assert abs(out["auc"] - m["auc"]) <= 1e-4 and abs(out["ap"] - m["ap"]) <= 1e-4
    # pair_scores on a shuffled pair list: the matrix's cells
    rng = np.random.RandomState(0)
    pi, oi = rng.randint(0, len(nodes), 200), rng.randint(0, len(nodes), 200)
    assert np.array_equal(atk.pair_scores(nodes[pi], nodes[oi]), mat[pi, oi])

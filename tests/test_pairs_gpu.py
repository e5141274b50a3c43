"""lt_influence_pairs on the device: the scores of a LIST of (probe, observed) pairs.

What is pinned here:
  * the same BITS as the rectangle: ``influence_pairs`` equals ``influence_rows(probes, observed)[i, j]`` for the same mode, on every
    stage-A route the rows call takes (the fused record route, the item kernels, hub rows, a directed pattern), under forced
    probe chunking and without the membership bitmap;
  * `delta` within 1e-5 of the largest score of the reference evaluated in fp64 (oracle.RestrictedOracle) -- the bound of every
    `delta` test of this suite -- with exact zeros where the oracle has them;
  * the naive attack (attacker.py:143-201) and ``balanced-full`` (attacker.py:250-284) end to end on the fixtures, and
    ``balanced-full`` on a graph of 1e5 nodes, where a 1024-probe chunk of rows asks for more workspace than the whole pair call.
"""
import argparse
import ctypes as C
import os
import time

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import csr_from

pytestmark = pytest.mark.gpu

F_IN = 48


def _params(w, dev):
    return [torch.from_numpy(w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")]


def _graph(kind):
    """(served adjacency, nodes every list must hold).  `er`: Erdos-Renyi with isolated nodes, records for the fused route; `pl`:
    power-law with hub rows; `dir`: a directed pattern with empty rows and columns."""
    from linkteller_amd import graph, synth
    if kind == "er":
        a = synth.erdos_renyi_graph(1500, 3000, seed=1)
        iso = np.where(np.diff(a.indptr) == 0)[0]
        assert len(iso) >= 2
        return graph.first_order_gcn(a), iso[:2]
    if kind == "pl":
        a_hat = graph.first_order_gcn(synth.powerlaw_graph(3000, 20000, seed=2))
        deg = np.diff(a_hat.indptr)
        hubs = np.argsort(-deg)[:3]
        assert deg[hubs].min() > 128                      # (LT_ROW_SEG: observed hub rows, probed hubs)
        return a_hat, hubs
    n = 2500
    rng = np.random.RandomState(11)
    rows, cols = rng.randint(0, n, 30000), rng.randint(0, n, 30000)
    keep = (rows != cols) & (cols >= 40) & (rows >= 20)            # columns 0..39 stay empty, rows 0..19 too
    a = sp.csr_matrix((rng.uniform(0.05, 0.3, keep.sum()).astype(np.float32), (rows[keep], cols[keep])), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    return a, np.array([0, 5, 39, 40, 3, 41])


def _features(kind, n):
    from linkteller_amd import synth
    if kind == "twitch":
        return synth.twitch_like_features(n, F_IN, seed=4, density=0.02)      # (no row with more than 8 indicators set: rows the feature-difference route takes)
    return synth.gaussian_features(n, F_IN, seed=2)


def _baseline(a_hat, x, w, gpu):
    """A `delta` baseline on one of the routes that form the product rows (the feature-difference route for standardised
    indicator features, the dense fp64 product otherwise), where the rows call of a graph with records takes the fused route."""
    from linkteller_amd import _lib, engine, graph
    _lib.set_tuning("aggregate_first", 0)
    try:
        base = engine.Baseline(graph.HipGraph(a_hat), torch.from_numpy(x).to(gpu), *_params(w, gpu)).enable_fp64()
    finally:
        _lib.set_tuning("aggregate_first", None)
    return base


def _ragged(a_hat, special, seed, n_probe=48, n_pool=160):
    """A ragged pair list: probes with repeats and without pairs, the special nodes as probes and as observed nodes, u == v,
    pairs listed twice; about three quarters of a probe's partners are nodes its perturbation reaches (rows that read a member of R_v),
    the rest random.  Returns (probe_nodes, pair_ptr, pair_obs, pool): every observed node is in `pool`."""
    n = a_hat.shape[0]
    rng = np.random.RandomState(seed)
    a = sp.csr_matrix(a_hat)
    at, ac = a.T.tocsr(), a.tocsc()
    pool = np.unique(np.concatenate([special, rng.choice(n, n_pool, replace=False)]))
    probes = np.concatenate([special, rng.choice(n, n_probe - len(special) - 4, replace=False)])
    probes = np.concatenate([probes, probes[:2], pool[:2]])              # repeats; probes that are observed as well
    rng.shuffle(probes)
    ptr, obs = [0], []
    extra = []
    for i, v in enumerate(probes):
        cnt = int(rng.choice([0, 0, 1, 3, 10, 40]))
        if v in special and cnt == 0:
            cnt = 6
        r_v = at[v].indices
        reach = np.unique(np.concatenate([ac[:, r].indices for r in r_v])) if len(r_v) else np.empty(0, dtype=np.int64)
        mine = []
        for _ in range(cnt):
            if len(reach) and rng.rand() < 0.75:
                u = int(reach[rng.randint(len(reach))])
                extra.append(u)
            else:
                u = int(pool[rng.randint(len(pool))])
            mine.append(u)
        if cnt >= 3:
            mine[1] = int(v)                                             # u == v
            mine[2] = mine[0]                                            # the same pair twice
            extra.append(int(v))
        if cnt >= 6:
            mine[3] = int(special[i % len(special)])                     # every special node is observed by someone
        obs += mine
        ptr.append(len(obs))
    pool = np.unique(np.concatenate([pool, np.asarray(extra, dtype=np.int64)]))
    probes, ptr, obs = probes.astype(np.int64), np.asarray(ptr, dtype=np.int64), np.asarray(obs, dtype=np.int64)
    assert (np.diff(ptr) == 0).any() and len(np.unique(probes)) < len(probes)
    for s in special:
        assert s in probes and s in obs
    return probes, ptr, obs, pool


def _from_rect(rect, ptr, obs, pool):
    col = np.searchsorted(pool, obs)
    assert np.array_equal(pool[col], obs)
    return rect[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), col]


def _case(gkind, shape, fkind, gpu, seed=0):
    from linkteller_amd import synth
    a_hat, special = _graph(gkind)
    x = _features(fkind, a_hat.shape[0])
    w = synth.gcn_weights(F_IN, shape[0], shape[1], seed=3)
    base = _baseline(a_hat, x, w, gpu)
    return a_hat, x, w, base, _ragged(a_hat, special, seed + 7)


SHAPES = [(16, 2), (256, 8), (30, 3)]


@pytest.mark.parametrize("fkind", ["twitch", "gauss"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"h{s[0]}c{s[1]}")
@pytest.mark.parametrize("gkind", ["er", "pl", "dir"])
def test_pairs_are_the_bits_of_the_rectangle(gpu, gkind, shape, fkind):
    """1. influence_pairs == influence_rows(probes, observed)[i, j], bit for bit: `delta` with the rows call on its default route
    (the fused record route on the Erdos-Renyi graph: asserted) and on the item kernels, `sparse`, and `full` (evaluated as
    `sparse`) against the rows call's `sparse`."""
    from test_gpu_round4 import _item_stage_a_launches
    from linkteller_amd import _lib
    a_hat, x, w, base, (probes, ptr, obs, pool) = _case(gkind, shape, fkind, gpu)
    assert base.fp64_route() == (1 if fkind == "twitch" else 0)      # the feature-difference route / the dense fp64 product
    if gkind == "er":
        assert _item_stage_a_launches(lambda: base.influence_rows(probes, pool, 1e-4, "delta")) == 0      # the record route
    if gkind == "pl":
        deg = np.diff(a_hat.indptr)
        assert (deg[obs] > 128).any() and (deg[probes[np.diff(ptr) > 0]] > 128).any()
    got = base.influence_pairs(probes, ptr, obs, 1e-4, "delta").cpu().numpy()
    assert got.shape == (len(obs),) and got.dtype == np.float32
    rect = base.influence_rows(probes, pool, 1e-4, "delta").cpu().numpy()
    want = _from_rect(rect, ptr, obs, pool)
    assert np.array_equal(got, want), np.abs(got - want).max()
    _lib.set_tuning("delta_fused", 0)
    try:
        rect0 = base.influence_rows(probes, pool, 1e-4, "delta").cpu().numpy()
        got0 = base.influence_pairs(probes, ptr, obs, 1e-4, "delta").cpu().numpy()
    finally:
        _lib.set_tuning("delta_fused", None)
    assert np.array_equal(got0, _from_rect(rect0, ptr, obs, pool)) and np.array_equal(got0, got)
    assert (got > 0).sum() >= len(got) // 4 and (got == 0).any()
    sparse = base.influence_pairs(probes, ptr, obs, 1e-4, "sparse").cpu().numpy()
    rect_s = base.influence_rows(probes, pool, 1e-4, "sparse").cpu().numpy()
    assert np.array_equal(sparse, _from_rect(rect_s, ptr, obs, pool))
    assert np.array_equal(base.influence_pairs(probes, ptr, obs, 1e-4, "full").cpu().numpy(), sparse)
    assert (sparse > 0).any()


@pytest.mark.parametrize("gkind,shape,fkind", [("er", (16, 2), "gauss"), ("er", (256, 8), "twitch"), ("pl", (256, 8), "twitch"),
                                               ("pl", (30, 3), "gauss"), ("dir", (30, 3), "gauss"), ("dir", (16, 2), "twitch")])
def test_pairs_against_the_reference_in_fp64(gpu, gkind, shape, fkind):
    """2. `delta` within 1e-5 x the largest score of oracle.RestrictedOracle on the listed pairs' probes; exact zeros where the
    oracle has them; at least a third of the compared pairs are non-zero in the oracle."""
    from oracle import linkteller_oracle as O
    a_hat, x, w, base, (probes, ptr, obs, pool) = _case(gkind, shape, fkind, gpu, seed=1)
    got = base.influence_pairs(probes, ptr, obs, 1e-4, "delta").cpu().numpy().astype(np.float64)
    ref = _from_rect(O.RestrictedOracle(x, a_hat, w).rows(probes, pool, 1e-4), ptr, obs, pool)
    nz = (ref != 0).mean()
    err = np.abs(got - ref).max()
    print(f"{gkind} {shape} {fkind}: {len(ref)} pairs, {nz:.2f} non-zero in the oracle, max score {ref.max():.3f}, |pairs - fp64| = {err:.2e}")
    assert nz >= 1 / 3
    assert err <= 1e-5 * ref.max()
    assert np.all(got[ref == 0] == 0)


def test_pairs_under_forced_chunking_and_without_the_bitmap(gpu):
    """3. The same bits with a 32 KB chunk budget (a few probes per chunk: chunks whose probes own no pair, hub probes alone in
    a chunk) and with the membership bitmap off (find_row); also on the aggregate-first route small dense features take."""
    from linkteller_amd import _lib, engine, graph, synth
    a_hat, x, w, base, (probes, ptr, obs, pool) = _case("pl", (256, 8), "twitch", gpu, seed=2)
    _lib.set_tuning("aggregate_first", 1)
    try:
        dflt = engine.Baseline(graph.HipGraph(a_hat), torch.from_numpy(synth.gaussian_features(a_hat.shape[0], F_IN, seed=2)).to(gpu),
                               *_params(w, gpu)).enable_fp64()
    finally:
        _lib.set_tuning("aggregate_first", None)
    for b in (base, dflt):
        ref = {m: b.influence_pairs(probes, ptr, obs, 1e-4, m).cpu().numpy() for m in ("delta", "sparse")}
        rect = b.influence_rows(probes, pool, 1e-4, "delta").cpu().numpy()
        assert np.array_equal(ref["delta"], _from_rect(rect, ptr, obs, pool))
        for key, value in (("chunk_budget_bytes", 1 << 15), ("item_bits", 0)):
            _lib.set_tuning(key, value)
            try:
                got = {m: b.influence_pairs(probes, ptr, obs, 1e-4, m).cpu().numpy() for m in ("delta", "sparse")}
            finally:
                _lib.set_tuning(key, None)
            for m in ref:
                assert np.array_equal(got[m], ref[m]), (key, m, np.abs(got[m] - ref[m]).max())
    assert dflt.fp64_route() == 2


def test_pairs_follow_a_weight_update(gpu):
    """4. An in-place weight update + refresh(): the pairs follow the new weights and equal the rows call made afterwards."""
    a_hat, x, w, base, (probes, ptr, obs, pool) = _case("er", (30, 3), "twitch", gpu, seed=3)
    for mode in ("delta", "sparse"):
        before = base.influence_pairs(probes, ptr, obs, 1e-4, mode).cpu().numpy()
        base.w1.mul_(1.25)
        base.w2.add_(0.01)
        base.refresh()
        after = base.influence_pairs(probes, ptr, obs, 1e-4, mode).cpu().numpy()
        rect = base.influence_rows(probes, pool, 1e-4, mode).cpu().numpy()
        assert np.array_equal(after, _from_rect(rect, ptr, obs, pool))
        assert not np.array_equal(after, before)


def test_pairs_refusals_and_empty_calls(gpu):
    """5. Empty calls succeed and launch nothing; an id out of range surfaces as IndexError after engine.node_check(); a pair_ptr
    that is not a valid offset array is refused before anything is written."""
    from linkteller_amd import _lib, engine
    a_hat, x, w, base, (probes, ptr, obs, pool) = _case("er", (16, 2), "gauss", gpu, seed=4)
    n = a_hat.shape[0]
    assert base.influence_pairs(probes, np.zeros(len(probes) + 1, dtype=np.int64), [], 1e-4, "delta").numel() == 0
    assert base.influence_pairs([], [0], [], 1e-4, "sparse").numel() == 0
    h = _lib.lib()
    assert h.lt_influence_pairs(base.handle, None, 0, None, None, 0, 1e-4, 2, None, None, 0, None) == 0
    torch.cuda.synchronize()
    engine.node_check()
    for bad_probe in (True, False):
        p = torch.tensor([3, n if bad_probe else 4, 5], dtype=torch.int32, device=gpu)
        o = torch.tensor([1, 2, 7 if bad_probe else -1, 9], dtype=torch.int32, device=gpu)
        base.influence_pairs(p, [0, 2, 3, 4], o, 1e-4, "delta" if bad_probe else "sparse")
        torch.cuda.synchronize()
        with pytest.raises(IndexError):
            engine.node_check()
        engine.node_check()                                              # cleared
    out = torch.full((len(obs),), -7.0, dtype=torch.float32, device=gpu)
    for wrong in (ptr[::-1].copy(), np.concatenate([[1], ptr[1:]]), np.concatenate([ptr[:-1], [ptr[-1] + 1]]),
                  np.concatenate([ptr[:3], [ptr[2] - 1], ptr[4:]])):
        with pytest.raises(_lib.LinkTellerHipError):
            base.influence_pairs(probes, wrong, obs, 1e-4, "delta", out=out)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=gpu)
    po = torch.zeros(4, dtype=torch.int32, device=gpu)
    assert h.lt_influence_pairs(base.handle, po.data_ptr(), 1, None, po.data_ptr(), 2, 1e-4, 2, out.data_ptr(), ws.data_ptr(),
                                ws.numel(), None) == -1                  # NULL pair_ptr with pairs
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    with pytest.raises(ValueError):
        base.influence_pairs(probes, ptr[:-1], obs, 1e-4)


def _next_rows(gpu, prefix_adj, xkey):
    import types
    from linkteller_amd import graph
    from linkteller_amd.gcn import GCN
    g = np.load(os.path.join(__import__("conftest").GOLDEN, "next_rows.npz"), allow_pickle=False)
    a = csr_from(g, prefix_adj)
    x = torch.from_numpy(g[xkey]).to(gpu)
    adj_t = graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(a)).to(gpu)
    w = types.SimpleNamespace(features_2=x, adj_2=adj_t, adj_ori=a, n_nodes=a.shape[0])
    model = GCN(64, 32, 2, 0.5)
    model.load_state_dict({k: torch.from_numpy(g[f"sd.{k}"]) for k in ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias")})
    model.to(gpu).eval()
    return g, a, w, model


def test_naive_attack_on_the_device(gpu, tmp_path, monkeypatch):
    """6. ``link_prediction_attack`` (attacker.py:143-201) on the fixture graph: scores within 1e-5 x max of
    ``get_gradient_eps_mat(v)[u].norm()`` evaluated in float64, AUC / AP within 1e-4 of the oracle's, the bits of the values the
    efficient attack reads from ``influence_matrix()``, the naive file name."""
    from oracle import linkteller_oracle as O
    from linkteller_amd.attacker import Attacker
    g, a, w, model = _next_rows(gpu, "adj", "x")
    monkeypatch.chdir(tmp_path)
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=32, sample_seed=42, influence=1e-4,
                              mode="vanilla-clean", attack_mode="naive")
    atk = Attacker(args, model, w)
    atk.prepare_test_data()
    atk.link_prediction_attack()
    name = os.path.join("eval_twitch/ES/RU", "unbalanced_32_42.pt")
    assert atk.naive_result_filename() == name and os.path.exists(name)
    saved = torch.load(name, weights_only=False)
    ex = np.asarray(atk.exist_edges, dtype=np.int64).reshape(-1, 2)
    nex = np.asarray(atk.nonexist_edges, dtype=np.int64).reshape(-1, 2)
    pred = np.asarray(saved["result"]["pred"])
    assert saved["result"]["y"] == [1] * len(ex) + [0] * len(nex) and len(pred) == len(ex) + len(nex)
    # the reference's quantity, pair by pair, in float64 (one perturbed forward per distinct v)
    x64 = torch.from_numpy(g["x"]).double()
    adj64 = O.to_torch_sparse(O.first_order_gcn(a)).double()
    P64 = {k: torch.from_numpy(g[f"sd.{n}"]).double() for k, n in (("W1", "gc1.weight"), ("b1", "gc1.bias"), ("W2", "gc2.weight"), ("b2", "gc2.bias"))}
    mats = {}
    with torch.no_grad():
        for v in np.unique(np.concatenate([ex[:, 1], nex[:, 1]])):
            mats[int(v)] = O.get_gradient_eps_mat(x64, adj64, P64, int(v), 1e-4)
    ref = np.array([mats[int(v)][int(u)].norm().item() for u, v in np.concatenate([ex, nex])])
    err = np.abs(pred - ref).max()
    print(f"naive: {len(ex)} + {len(nex)} pairs, max score {ref.max():.3f}, |naive - fp64| = {err:.2e}")
    assert err <= 1e-5 * ref.max()
    m = O.attack_metrics(list(ref[:len(ex)]), list(ref[len(ex):]))
    assert abs(atk.auc - m["auc"]) <= 1e-4 and abs(atk.ap - m["ap"]) <= 1e-4
    # the values the efficient attack reads from its matrix, bit for bit
    infl = atk.influence_matrix()
    ne, nn = O.pair_scores(infl, list(atk.test_nodes), ex.tolist(), nex.tolist())
    assert np.array_equal(pred, np.asarray(ne + nn))
    # the naive attack of `vanilla` runs carries the noise parameters in its name, still without the attack-mode prefix
    args.mode, args.perturb_type, args.epsilon, args.noise_seed = "vanilla", "discrete", 5.0, 7
    assert atk.naive_result_filename() == os.path.join("eval_twitch/ES/RU", "unbalanced_discrete_32_42_eps-5.0_seed-7.pt")


@pytest.mark.parametrize("mode", ["delta", "sparse"])
def test_balanced_full_pred_is_unchanged(gpu, tmp_path, monkeypatch, mode):
    """7. ``link_prediction_attack_efficient_balanced`` through the pair list: the saved ``pred`` is, value for value, the list
    assembled from ``_rows(starts, all_nodes)`` -- the computation of attacker.py:250-284 restated here."""
    from linkteller_amd.attacker import Attacker
    g, ab, w, model = _next_rows(gpu, "bf.adj", "bf.x")
    monkeypatch.chdir(tmp_path)
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="balanced-full", n_test=7, sample_seed=82, influence=1e-4,
                              mode="vanilla-clean", attack_mode="efficient", influence_mode=mode)
    atk = Attacker(args, model, w)
    atk.prepare_test_data()
    atk.link_prediction_attack_efficient_balanced()
    pred = np.asarray(torch.load(str(g["bf.ref32.filename"]), weights_only=False)["result"]["pred"])
    ex = np.asarray(atk.exist_edges, dtype=np.int64).reshape(-1, 2)
    nex = np.asarray(atk.nonexist_edges, dtype=np.int64).reshape(-1, 2)
    n = ab.shape[0]
    starts = np.union1d(ex[:, 0], nex[:, 0])
    rows = atk._rows(starts, np.arange(n, dtype=np.int64)).cpu().numpy().astype(np.float64)
    pos = np.full(n, -1, dtype=np.int64)
    pos[starts] = np.arange(len(starts))
    s_ex, s_nex = rows[pos[ex[:, 0]], ex[:, 1]], rows[pos[nex[:, 0]], nex[:, 1]]
    want = np.concatenate([s_ex[np.argsort(ex[:, 0], kind="stable")], s_nex[np.argsort(nex[:, 0], kind="stable")]])
    assert pred.shape == want.shape and np.array_equal(pred, want)
    assert (pred > 0).any()


def test_balanced_full_at_1e5_nodes(gpu, tmp_path, monkeypatch):
    """8. ``balanced-full`` on 100 000 nodes / 400 000 edges (mean degree 8), H = 64, with the default 1 GiB chunk budget: 800 000
    pairs from ~1e5 probes in one pair call whose workspace is below what ONE 1024-probe chunk of rows asks for; 2 000 sampled
    pairs (half edges) within the fp64 bound.  Wall time of the whole test on an MI355X: see the printed line (the two
    host-side samplers -- the reference's scalar draws -- are most of it)."""
    import types
    from oracle import linkteller_oracle as O
    from linkteller_amd import _lib, graph, synth
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN
    t_all = time.time()
    n, e, f, hdim = 100_000, 400_000, 64, 64
    a = synth.erdos_renyi_graph(n, e, seed=3)
    x = synth.twitch_like_features(n, f, seed=4, density=0.05)
    wts = synth.gcn_weights(f, hdim, 2, seed=5)
    a_hat = graph.first_order_gcn(a)
    w = types.SimpleNamespace(features_2=torch.from_numpy(x).to(gpu), adj_2=graph.sparse_mx_to_torch_sparse_tensor(a_hat).to(gpu),
                              adj_ori=a, n_nodes=n)
    model = GCN(f, hdim, 2, 0.5)
    model.load_state_dict({"gc1.weight": torch.from_numpy(wts["W1"]), "gc1.bias": torch.from_numpy(wts["b1"]),
                           "gc2.weight": torch.from_numpy(wts["W2"]), "gc2.bias": torch.from_numpy(wts["b2"])})
    model.to(gpu).eval()
    monkeypatch.chdir(tmp_path)
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="balanced-full", n_test=0, sample_seed=82, influence=1e-4,
                              mode="vanilla-clean", attack_mode="efficient")
    atk = Attacker(args, model, w)
    atk.prepare_test_data()
    t_prep = time.time() - t_all
    t0 = time.time()
    atk.link_prediction_attack_efficient_balanced()
    t_attack = time.time() - t0
    ex = np.asarray(atk.exist_edges, dtype=np.int64).reshape(-1, 2)
    nex = np.asarray(atk.nonexist_edges, dtype=np.int64).reshape(-1, 2)
    assert len(ex) == e and len(nex) == e
    h = _lib.lib()
    starts = np.union1d(ex[:, 0], nex[:, 0])
    ws_pairs = h.lt_influence_pairs_workspace_bytes(atk._baseline.handle, len(starts), 2 * e, _lib.MODE_DELTA)
    ws_rows = h.lt_influence_workspace_bytes(atk._baseline.handle, 1024, n, _lib.MODE_DELTA)
    assert 0 < ws_pairs < ws_rows, (ws_pairs, ws_rows)
    pred = np.asarray(torch.load(os.path.join("eval_twitch/ES/RU", f"efficient_balanced-full_{n}_82.pt"), weights_only=False)["result"]["pred"])
    oe, on = np.argsort(ex[:, 0], kind="stable"), np.argsort(nex[:, 0], kind="stable")
    rng = np.random.RandomState(9)
    ie, ine = rng.choice(e, 1000, replace=False), rng.choice(e, 1000, replace=False)
    got = np.concatenate([pred[:e][ie], pred[e:][ine]])
    pairs = np.concatenate([ex[oe][ie], nex[on][ine]])                   # (probe = first node, observed = second)
    ro = O.RestrictedOracle(x, a_hat, wts)
    ref = np.array([ro.rows([u], [v], 1e-4)[0, 0] for u, v in pairs])
    err = np.abs(got - ref).max()
    print(f"balanced-full n={n}: sampling {t_prep:.1f} s, attack {t_attack:.1f} s, workspace pairs {ws_pairs / 2**20:.1f} MiB against "
          f"{ws_rows / 2**20:.1f} MiB for one 1024-probe chunk of rows; |pairs - fp64| / max = {err / ref.max():.2e}; "
          f"whole test {time.time() - t_all:.1f} s")
    assert (ref != 0).mean() >= 1 / 3
    assert err <= 1e-5 * ref.max()
    assert np.all(got[ref == 0] == 0)

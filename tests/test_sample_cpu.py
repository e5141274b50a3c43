"""The sampling contracts without a GPU: the numpy restatements of tests/sample_restate.py against the host functions they
restate (sampling.edge_sets_among_nodes, engine.group_pairs, the acceptance rule of construct_balanced_edge_sets), the draw counts
of Philox stream 3 recorded when the contract was written, the command line's refusals, and the loud failure of the device routes."""
import argparse
import types

import numpy as np
import pytest
import scipy.sparse as sp

import sample_restate as S


def _complete(n, loops):
    return sp.csr_matrix(np.ones((n, n)) - (0 if loops else 1) * np.eye(n))


def _with_zeros_and_loops(n=60, seed=5):
    """A directed pattern with stored zeros (about half the entries) and self loops (every third node)."""
    rng = np.random.RandomState(seed)
    loops = np.arange(0, n, 3)
    r = np.concatenate([rng.randint(0, n, 5 * n), loops])
    c = np.concatenate([rng.randint(0, n, 5 * n), loops])
    out = sp.csr_matrix((np.ones(r.size), (r, c)), shape=(n, n))
    out.sum_duplicates()
    out.sort_indices()
    out.data = rng.randint(0, 2, out.nnz).astype(np.float64)       # (nothing eliminates the zeros: they stay stored)
    assert (out.data == 0).any() and (out.data != 0).any() and out.nnz > out.count_nonzero()
    return out


@pytest.mark.parametrize("k", [2, 3, 17, 64])
def test_square_labels_restatement_equals_the_host_enumeration(k):
    from linkteller_amd import sampling, synth
    for adj in (synth.erdos_renyi_graph(200, 1500, seed=3), _with_zeros_and_loops()):
        n = adj.shape[0]
        nodes = np.random.RandomState(k).choice(n, min(k, n), replace=False)
        index, labels, count = S.square_labels(adj, nodes, len(nodes) + 3)
        iu, ju = S.triangle(len(nodes))
        ex, nex = sampling.edge_sets_among_nodes(adj, nodes)
        pairs = np.stack([nodes[iu], nodes[ju]], axis=1)
        assert np.array_equal(pairs[labels == 1], ex) and np.array_equal(pairs[labels == 0], nex)
        assert count == len(ex)
        # the index is Attacker._metric_lists' arithmetic: ind[v] * lds + ind[u] for the pair (u, v)
        node2ind = np.full(n, -1, dtype=np.int64)
        node2ind[nodes] = np.arange(len(nodes))
        assert np.array_equal(index, node2ind[pairs[:, 1]] * (len(nodes) + 3) + node2ind[pairs[:, 0]])


def test_stored_zeros_count_as_present():
    from linkteller_amd import sampling
    adj = _with_zeros_and_loops()
    nodes = np.arange(adj.shape[0])[::-1].copy()
    _, labels, _ = S.square_labels(adj, nodes, len(nodes))
    dropped = sp.csr_matrix(adj, copy=True)
    dropped.eliminate_zeros()
    _, labels_dropped, _ = S.square_labels(dropped, nodes, len(nodes))
    assert labels.sum() > labels_dropped.sum()                     # the case does hold stored zeros among the sampled pairs
    ex, _ = sampling.edge_sets_among_nodes(adj, nodes)
    assert len(ex) == labels.sum()


@pytest.mark.parametrize("m", [1, 2, 300, 257])
def test_group_pairs_restatement_equals_the_host_function(m):
    from linkteller_amd import engine
    rng = np.random.RandomState(m)
    probe = rng.randint(0, 70000 if m == 300 else 40, m)
    observed = rng.randint(0, 70000, m)
    if m == 300:
        probe[::7] = probe[0]
        observed[::7] = observed[0]                                # repeated pairs
    for p in (probe, np.full(m, 5)):
        want = engine.group_pairs(p, observed)
        got = S.group_pairs(p, observed)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


def _check_acceptance(adj, r):
    pat = S.pattern(adj)
    dense = pat.toarray() != 0
    for u, v in r["non_edges"]:
        assert not dense[u, v] and not dense[v, u]
    assert r["self_pairs"] == int((r["non_edges"][:, 0] == r["non_edges"][:, 1]).sum())


def test_balanced_restatement_and_the_recorded_draw_counts():
    from linkteller_amd import sampling, synth
    a = synth.erdos_renyi_graph(300, 1500, seed=1)
    r = S.balanced_pairs(a, 42)
    assert r["ok"] and len(r["edges"]) == 1500 and r["draws"] == 1553 and len(r["non_edges"]) == 1500
    _check_acceptance(a, r)
    # the edges are construct_balanced_edge_sets' edges, in its order
    np.random.seed(0)
    (ex, _), _ = sampling.construct_balanced_edge_sets("x", "balanced-full", a, 0)
    assert np.array_equal(r["edges"], ex)

    b = synth.erdos_renyi_graph(40, 390, seed=2)
    r = S.balanced_pairs(b, 42)
    assert r["ok"] and len(r["edges"]) == 390 and r["draws"] == 786 and r["self_pairs"] == 14
    _check_acceptance(b, r)
    short = S.balanced_pairs(b, 42, max_draws=700)
    assert not short["ok"] and short["accepted"] < 390 and short["draws"] == 700
    assert np.array_equal(short["non_edges"], r["non_edges"][:short["accepted"]])      # a prefix of the same stream

    k = _complete(12, loops=False)
    r = S.balanced_pairs(k, 42)
    assert r["ok"] and len(r["edges"]) == 66 and r["draws"] == 882 and r["draws"] <= S.default_max_draws(66)
    assert r["self_pairs"] == 66 and (r["non_edges"][:, 0] == r["non_edges"][:, 1]).all()      # only u == v is acceptable
    full = S.balanced_pairs(_complete(12, loops=True), 42)
    assert not full["ok"] and full["accepted"] == 0 and full["draws"] == S.default_max_draws(66)
    assert S.balanced_pairs(a, 43)["non_edges"].tolist() != S.balanced_pairs(a, 42)["non_edges"].tolist()


def test_draws_follow_the_stated_counter_layout():
    """Draw t is a function of t alone (rounds cannot show), both key words are in use, and t >> 32 reaches counter word 1."""
    from train_restate import philox4x32_10
    seed = (7 << 32) | 99
    u, v = S.draws(1000, seed, 0, 300)
    u2, v2 = S.draws(1000, seed, 100, 50)
    assert np.array_equal(u[100:150], u2) and np.array_equal(v[100:150], v2)
    assert 0 <= u.min() and u.max() < 1000 and 0 <= v.min() and v.max() < 1000
    t = (1 << 32) + 5
    w = philox4x32_10(np.array([[5, 1, 3, 0]], dtype=np.uint64), np.array([[99, 7]], dtype=np.uint64))[0].astype(np.uint64)
    ub, vb = S.draws(1000, seed, t, 1)
    assert ub[0] == (int(w[0]) * 1000) >> 32 and vb[0] == (int(w[1]) * 1000) >> 32
    assert S.draws(1000, 99, 0, 300)[0].tolist() != u.tolist()


def test_cli_sample_switches(monkeypatch):
    from linkteller_amd import main as lt_main, worker
    d = lt_main.get_arguments([])
    assert d.sample_build == "host" and d.sample_rng == "numpy"
    assert lt_main.get_arguments(["--sample-build", "device"]).sample_build == "device"
    assert lt_main.get_arguments(["--sample-rng", "philox"]).sample_rng == "philox"
    for bad in (["--sample-build", "gpu"], ["--sample-rng", "mt"]):
        with pytest.raises(SystemExit):
            lt_main.get_arguments(bad)

    def no_worker(*a, **k):
        raise AssertionError("a Worker was built")
    monkeypatch.setattr(worker, "Worker", no_worker)
    common = ["--test", "--dataset", "twitch/ES/RU"]
    for extra in (["--sample-build", "device"],                                                    # no --attack
                  ["--sample-rng", "philox", "--sample-type", "balanced-full"],
                  ["--sample-build", "device", "--sample-rng", "philox", "--sample-type", "balanced-full"]):
        with pytest.raises(NotImplementedError, match="need --attack"):
            lt_main.main(common + extra)
    for st in ("unbalanced", "unbalanced-lo", "unbalanced-hi", "balanced"):
        with pytest.raises(NotImplementedError, match="--sample-rng philox needs --sample-type balanced-full"):
            lt_main.main(common + ["--attack", "--sample-rng", "philox", "--sample-type", st])
    lt_main.check_sample_build(lt_main.get_arguments(["--attack", "--sample-build", "device", "--sample-type", "unbalanced"]))
    lt_main.check_sample_build(lt_main.get_arguments(["--attack", "--sample-rng", "philox", "--sample-type", "balanced-full"]))
    lt_main.check_sample_build(lt_main.get_arguments([]))
    lt_main.check_sample_build(argparse.Namespace(attack=False))                                   # a Namespace without the flags: host


def _attacker(sample_type):
    import torch
    from linkteller_amd import synth
    from linkteller_amd.attacker import Attacker
    adj = synth.erdos_renyi_graph(50, 120, seed=1)
    w = types.SimpleNamespace(features_2=torch.zeros(50, 4), adj_2=None, adj_ori=adj, n_nodes=50)
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type=sample_type, n_test=10, sample_seed=42, influence=1e-4,
                              mode="vanilla-clean", attack_mode="efficient")
    return Attacker(args, None, w)


def test_device_routes_fail_loudly_without_a_gpu_and_the_defaults_are_the_host_route():
    import torch
    from linkteller_amd import _lib, engine, sampling
    atk = _attacker("unbalanced")
    with pytest.raises(ValueError, match="balanced-full only"):
        atk.prepare_test_data(rng="philox")
    with pytest.raises(ValueError):
        atk.prepare_test_data(pairs="gpu")
    with pytest.raises(ValueError):
        atk.prepare_test_data(rng="mt19937")
    if not torch.cuda.is_available():
        with pytest.raises(_lib.LinkTellerHipError):
            atk.prepare_test_data(pairs="device")
        with pytest.raises(_lib.LinkTellerHipError):
            _attacker("balanced-full").prepare_test_data(rng="philox")
        with pytest.raises(_lib.LinkTellerHipError):
            sampling.device_pattern_csr(atk.worker.adj_ori)
        with pytest.raises(_lib.LinkTellerHipError):
            sampling.upper_edge_count((torch.zeros(3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0))
    with pytest.raises(_lib.LinkTellerHipError):                   # host tensors are refused whether or not a GPU is there
        engine.group_pairs_device(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    # defaults and explicit host arguments: the same sample, the host lists
    atk.prepare_test_data()
    ex, nex, nodes = atk.exist_edges, atk.nonexist_edges, atk.test_nodes
    atk.prepare_test_data(pairs="host", rng="numpy")
    assert np.array_equal(atk.exist_edges, ex) and np.array_equal(atk.nonexist_edges, nex) and np.array_equal(atk.test_nodes, nodes)
    np.random.seed(42)
    (ex2, nex2), nodes2 = sampling.construct_edge_sets_from_random_subgraph("twitch/ES/RU", "unbalanced", atk.worker.adj_ori, 10)
    assert np.array_equal(ex, ex2) and np.array_equal(nex, nex2) and np.array_equal(nodes, nodes2)
    # balanced-full with device pairs and numpy's stream is the host route
    b = _attacker("balanced-full")
    b.prepare_test_data(pairs="device")
    np.random.seed(42)
    (bex, bnex), _ = sampling.construct_balanced_edge_sets("twitch/ES/RU", "balanced-full", b.worker.adj_ori, 50)
    assert np.array_equal(b.exist_edges, bex) and np.array_equal(b.nonexist_edges, bnex)


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    import ctypes as C
    from linkteller_amd import _lib
    h = _lib.lib()
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    assert h.lt_sample_square_workspace_bytes(100, 1) == 0 and h.lt_sample_square_workspace_bytes(0, 5) == 0
    assert h.lt_sample_square_workspace_bytes(101, 5) == 408
    sq = lambda **k: h.lt_sample_square_labels(*[{**dict(n=10, rp=p, col=p, nnz=0, nodes=p, k=3, lds=3, lab=p, idx=None, info=p, ws=p,
                                                        wsb=512, st=None), **k}[x]
                                                 for x in ("n", "rp", "col", "nnz", "nodes", "k", "lds", "lab", "idx", "info", "ws", "wsb", "st")])
    for bad in (dict(rp=None), dict(col=None), dict(nodes=None), dict(lab=None), dict(info=None), dict(ws=None), dict(k=1),
                dict(lds=2), dict(n=0), dict(wsb=8), dict(ws=p + 4), dict(nnz=-1)):
        assert sq(**bad) == -1, bad
    assert b"lt_sample_square_labels" in h.lt_last_error()
    assert h.lt_group_pairs_workspace_bytes(0) == 0 and h.lt_group_pairs_workspace_bytes((1 << 31) - 1) == 0
    need = h.lt_group_pairs_workspace_bytes(5)
    assert need > 0
    gp = lambda **k: h.lt_group_pairs(*[{**dict(n=10, pr=p, ob=p, m=5, a=p, b=p, c=p, d=p, info=p, ws=p, wsb=need, st=None), **k}[x]
                                        for x in ("n", "pr", "ob", "m", "a", "b", "c", "d", "info", "ws", "wsb", "st")])
    for bad in (dict(pr=None), dict(ob=None), dict(a=None), dict(b=None), dict(c=None), dict(d=None), dict(info=None), dict(ws=None),
                dict(m=0), dict(m=(1 << 31) - 1), dict(wsb=need - 8), dict(ws=p + 4), dict(n=0)):
        assert gp(**bad) == -1, bad
    assert h.lt_upper_edge_count(10, None, p, 0, p, None) == -1 and h.lt_upper_edge_count(0, p, p, 0, p, None) == -1
    assert h.lt_sample_balanced_workspace_bytes(10, -1, 0) == 0 and h.lt_sample_balanced_workspace_bytes(10, 5, -1) == 0
    assert h.lt_sample_balanced_workspace_bytes(10, 1 << 30, 0) == 0
    need = h.lt_sample_balanced_workspace_bytes(10, 5, 64)
    bp = lambda **k: h.lt_sample_balanced_philox(*[{**dict(n=10, rp=p, col=p, nnz=0, E=5, seed=1, md=0, rd=64, u=p, v=p, info=p, ws=p,
                                                          wsb=need, st=None), **k}[x]
                                                   for x in ("n", "rp", "col", "nnz", "E", "seed", "md", "rd", "u", "v", "info", "ws", "wsb", "st")])
    for bad in (dict(rp=None), dict(col=None), dict(u=None), dict(v=None), dict(info=None), dict(ws=None), dict(n=0), dict(E=-1),
                dict(md=-1), dict(rd=-1), dict(wsb=need - 8), dict(ws=p + 4)):
        assert bp(**bad) == -1, bad

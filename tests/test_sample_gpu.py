"""The attack's node pairs on the GPU (linkteller_amd/csrc/lt_sample.hip) against the host functions they replace and the numpy
restatements of tests/sample_restate.py.  Every comparison is array_equal: labels, indices, orders and pair lists are integers."""
import argparse
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import sample_restate as S

pytestmark = pytest.mark.gpu


def _complete(n, loops):
    return sp.csr_matrix(np.ones((n, n)) - (0 if loops else 1) * np.eye(n))


def _host_square(adj, nodes, lds):
    """(index, labels, count) from edge_sets_among_nodes and the arithmetic of Attacker._metric_lists, in triangle order."""
    from linkteller_amd import sampling
    nodes = np.asarray(nodes, dtype=np.int64)
    k = len(nodes)
    ex, nex = sampling.edge_sets_among_nodes(sp.csr_matrix(adj), nodes)
    iu, ju = np.triu_indices(k, k=1)
    pairs = np.stack([nodes[iu], nodes[ju]], axis=1)
    present = set(map(tuple, ex.tolist()))
    labels = np.array([tuple(p) in present for p in pairs.tolist()], dtype=np.uint8)
    assert np.array_equal(pairs[labels == 1], ex) and np.array_equal(pairs[labels == 0], nex)
    node2ind = np.full(int(nodes.max()) + 1, -1, dtype=np.int64)
    node2ind[nodes] = np.arange(k)
    index = node2ind[pairs[:, 1]] * int(lds) + node2ind[pairs[:, 0]]
    return index, labels, len(ex)


def _check_square(adj, nodes, lds, tag):
    from linkteller_amd import sampling
    csr = sampling.device_pattern_csr(adj)
    index, labels, info = sampling.square_labels_device(csr, nodes, lds)
    w_index, w_labels, w_count = _host_square(adj, nodes, lds)
    assert np.array_equal(labels.cpu().numpy(), w_labels), tag
    assert np.array_equal(index.cpu().numpy(), w_index), tag
    assert info.tolist() == [w_count, 0, 0, 0], tag
    assert sampling.check_square_info(info) == w_count
    index2, labels2, info2 = sampling.square_labels_device(csr, torch.as_tensor(np.asarray(nodes, dtype=np.int32)).cuda(), lds)
    assert torch.equal(index, index2) and torch.equal(labels, labels2) and torch.equal(info, info2), tag     # identical bytes
    none, labels3, _ = sampling.square_labels_device(csr, nodes, lds, index=False)
    assert none is None and torch.equal(labels, labels3)
    return w_labels


@pytest.fixture(scope="module")
def er1301():
    from linkteller_amd import synth
    return synth.erdos_renyi_graph(1301, 9000, seed=3)


@pytest.mark.parametrize("k", [2, 3, 64, 65, 257])
def test_square_labels_random_order(gpu, er1301, k):
    nodes = np.random.RandomState(k).choice(1301, k, replace=False)
    assert k < 3 or (np.diff(nodes) < 0).any()                      # not sorted
    for lds in (k, k + 3):
        labels = _check_square(er1301, nodes, lds, (k, lds))
    if k == 257:
        assert labels.any()


def test_square_labels_directed(gpu):
    from train_cases import directed_graph
    adj = directed_graph(513, 0)
    nodes = np.random.RandomState(1).permutation(513)[:200]
    labels = _check_square(adj, nodes, 203, "directed")
    dense = adj.toarray() != 0
    iu, ju = np.triu_indices(200, k=1)
    one_way = dense[nodes[iu], nodes[ju]] != dense[nodes[ju], nodes[iu]]
    assert one_way.any()                                            # some pair is present in one direction only ...
    assert np.array_equal(labels != 0, dense[nodes[iu], nodes[ju]])  # ... and the label reads row nodes[i] alone
    assert (labels[one_way] == 0).any() and (labels[one_way] == 1).any()


def test_square_labels_hub_rows(gpu):
    """Rows of 0, 1, 127 / 128 / 129, 1023 / 1024 / 1025 and 2049 entries: one trip of the block's walk, a partial trip, many."""
    from boundary_cases import hub_ladder
    g = hub_ladder()
    lengths = (0, 1, 127, 128, 129, 1023, 1024, 1025, 2049)
    rng = np.random.RandomState(7)
    rows = np.diff(g.a.indptr)
    picked = [g.u[d] for d in lengths]
    assert [int(rows[u]) for u in picked] == list(lengths)
    pool = np.unique(np.concatenate([g.row_sets[1]] + [rng.choice(g.row_sets[d], min(d, 30), replace=False) for d in lengths[2:]]))
    hubs_first = np.concatenate([picked, rng.permutation(pool)])     # every hub row stands in front of its columns: all its labels show
    labels = _check_square(g.a, hubs_first, len(hubs_first), "hubs first")
    assert labels.sum() >= 30 * 7
    _check_square(g.a, rng.permutation(hubs_first), len(hubs_first) + 3, "hubs shuffled")


def test_square_labels_stored_zeros_self_loops_and_tiny(gpu):
    from linkteller_amd import sampling
    from test_sample_cpu import _with_zeros_and_loops
    adj = _with_zeros_and_loops()
    nodes = np.random.RandomState(2).permutation(adj.shape[0])
    labels = _check_square(adj, nodes, len(nodes), "zeros")
    dropped = sp.csr_matrix(adj, copy=True)
    dropped.eliminate_zeros()
    assert labels.sum() > _host_square(dropped, nodes, len(nodes))[2]      # stored zeros among the sampled pairs count
    csr = sampling.device_pattern_csr(adj)
    assert csr[2] == adj.nnz                                        # the upload kept them
    two = sp.csr_matrix(np.array([[0.0, 1.0], [0.0, 0.0]]))
    assert _check_square(two, [0, 1], 2, "n=2").tolist() == [1]
    assert _check_square(two, [1, 0], 2, "n=2 reversed").tolist() == [0]
    empty = sp.csr_matrix((5, 5))
    assert _check_square(empty, [3, 1, 4], 3, "empty").tolist() == [0, 0, 0]
    # a (rowptr, col) pair of device tensors is taken as it is
    pair = sampling.device_pattern_csr(csr[:2])
    assert pair[2] == csr[2] and torch.equal(pair[0], csr[0])
    _, l2, _ = sampling.square_labels_device(pair, nodes, len(nodes))
    assert np.array_equal(l2.cpu().numpy(), labels)


def test_square_labels_bad_nodes_are_reported_not_faulted(gpu, er1301):
    from linkteller_amd import sampling
    csr = sampling.device_pattern_csr(er1301)
    _, _, info = sampling.square_labels_device(csr, [5, 9, 5, 700, 9, 5], 6)
    assert info.tolist()[1:] == [0, 3, 0]
    with pytest.raises(ValueError, match="repeat"):
        sampling.check_square_info(info)
    _, _, info = sampling.square_labels_device(csr, [5, 1301, -1, 700, 2 ** 31 - 1], 5)
    assert info.tolist()[1:] == [3, 0, 0]
    with pytest.raises(IndexError, match="outside"):
        sampling.check_square_info(info)
    with pytest.raises(ValueError):
        sampling.square_labels_device(csr, [5], 1)
    with pytest.raises(ValueError):
        sampling.square_labels_device(csr, [5, 6, 7], 2)
    torch.cuda.synchronize()


# ---- group_pairs_device ------------------------------------------------------------------------------------------------------
def _check_groups(probe, observed, n=None):
    from linkteller_amd import engine
    want = engine.group_pairs(probe, observed)
    assert all(np.array_equal(a, b) for a, b in zip(S.group_pairs(probe, observed), want))
    dev = torch.device("cuda:0")
    p = torch.as_tensor(np.asarray(probe, dtype=np.int32)).to(dev)
    o = torch.as_tensor(np.asarray(observed, dtype=np.int32)).to(dev)
    got = engine.group_pairs_device(p, o, n)
    assert [t.dtype for t in got] == [torch.int32, torch.int64, torch.int32, torch.int32] and all(t.is_cuda for t in got)
    for name, a, b in zip(("nodes", "ptr", "obs", "order"), got, want):
        assert np.array_equal(a.cpu().numpy(), b), name
    again = engine.group_pairs_device(p, o, n)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("m", [1, 257, 65537])
def test_group_pairs_device_sizes(gpu, m):
    rng = np.random.RandomState(m)
    _check_groups(rng.randint(0, 4385, m), rng.randint(0, 4385, m), 4385)
    _check_groups(np.full(m, 77), rng.randint(0, 4385, m), 4385)             # one probe only
    if m == 257:
        _check_groups(rng.randint(0, 256, m), rng.randint(0, 256, m), 256)   # one digit pass


def test_group_pairs_device_wide_ids_and_repeats(gpu):
    from linkteller_amd import engine
    rng = np.random.RandomState(0)
    probe, observed = rng.randint(0, 70000, 300), rng.randint(0, 70000, 300)
    probe[:40] = rng.randint(1 << 16, 70000, 40)                    # probes beyond two digits
    probe[50:300:5], observed[50:300:5] = probe[50], observed[50]   # repeated pairs
    assert (probe >= 1 << 16).sum() >= 40
    _check_groups(probe, observed, 70000)                           # three passes
    _check_groups(probe, observed)                                  # four
    p = torch.as_tensor(probe.astype(np.int32)).cuda()
    with pytest.raises(IndexError):
        engine.group_pairs_device(p, p, 60000)
    with pytest.raises(ValueError):
        engine.group_pairs_device(p[:0], p[:0])
    with pytest.raises(TypeError):
        engine.group_pairs_device(p.long(), p.long())
    torch.cuda.synchronize()


# ---- balanced pairs from the philox stream ---------------------------------------------------------------------------------------
def _balanced(adj, seed, **kw):
    from linkteller_amd import sampling
    csr = sampling.device_pattern_csr(adj)
    u, v, e, info = sampling.balanced_pairs_philox(csr, seed, **kw)
    return np.stack([u.cpu().numpy(), v.cpu().numpy()], axis=1).astype(np.int64), e, info


def _check_balanced(adj, seed, **kw):
    from linkteller_amd import sampling
    want = S.balanced_pairs(adj, seed)
    assert want["ok"]
    uv, e, info = _balanced(adj, seed, **kw)
    assert e == len(want["edges"]) == sampling.upper_edge_count(sampling.device_pattern_csr(adj))
    assert np.array_equal(uv[:e], want["edges"]) and np.array_equal(uv[e:], want["non_edges"])
    assert info[0] == e and info[1] == want["draws"] and info[3] == want["self_pairs"] and not info[4:].any()
    return uv, info


def test_balanced_pairs_equal_the_restatement(gpu):
    from linkteller_amd import synth
    from train_cases import directed_graph
    _, info = _check_balanced(synth.erdos_renyi_graph(300, 1500, seed=1), 42)
    assert info[1] == 1553
    _, info = _check_balanced(_complete(12, loops=False), 42)
    assert info[1] == 882 and info[3] == 66
    _check_balanced(directed_graph(513, 0), (9 << 32) | 7)          # both key words; u in row v and v in row u differ here
    b = synth.erdos_renyi_graph(40, 390, seed=2)
    results = [_check_balanced(b, 42, round_draws=r) for r in (64, 256, 0)]
    assert all(np.array_equal(results[0][0], r[0]) for r in results[1:])
    assert [int(r[1][1]) for r in results] == [786] * 3 and [int(r[1][3]) for r in results] == [14] * 3
    assert [int(r[1][2]) for r in results] == [13, 4, 1]             # ceil(786 / 64), ceil(786 / 256), one default round


def test_balanced_pairs_refusals_and_empty(gpu):
    from linkteller_amd import _lib, sampling, synth
    b = synth.erdos_renyi_graph(40, 390, seed=2)
    with pytest.raises(_lib.LinkTellerHipError, match=r"status -3.* of 390 non-edges accepted within 700 draws"):
        _balanced(b, 42, max_draws=700)
    with pytest.raises(_lib.LinkTellerHipError, match=r"status -3.*0 of 66 non-edges accepted within 8320 draws"):
        _balanced(_complete(12, loops=True), 42)
    csr = sampling.device_pattern_csr(b)
    for wrong in (389, 391):
        with pytest.raises(_lib.LinkTellerHipError, match="status -1.*stores 390"):
            sampling.balanced_pairs_philox(csr, 42, n_edges=wrong)
    uv, e, info = _balanced(sp.csr_matrix((9, 9)), 42)
    assert e == 0 and uv.shape == (0, 2) and not info.any()
    loops_only = sp.identity(9, format="csr")
    uv, e, info = _balanced(loops_only, 42)
    assert e == 0 and uv.shape == (0, 2)
    torch.cuda.synchronize()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def er_world(gpu):
    from linkteller_amd import graph, synth
    adj = synth.erdos_renyi_graph(300, 1500, seed=3)
    x = torch.from_numpy(synth.gaussian_features(300, 32, seed=4)).to(gpu)
    adj_t = graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(adj)).to(gpu)
    return adj, types.SimpleNamespace(features_2=x, adj_2=adj_t, adj_ori=adj, n_nodes=300)


def _args(**kw):
    base = dict(dataset="twitch/x", sample_type="unbalanced", n_test=64, sample_seed=42, influence=1e-4, mode="vanilla-clean",
                attack_mode="efficient", influence_mode="delta")
    base.update(kw)
    return argparse.Namespace(**base)


def _same_curves(a, b):
    for k in ("n_thresholds", "n_pos", "n_neg"):
        assert a[k] == b[k], k
    assert np.float64(a["ap"]).tobytes() == np.float64(b["ap"]).tobytes() and a["auc"] == b["auc"]
    for side, keys in (("auc", ("fpr", "tpr", "thresholds")), ("pr", ("precision", "recall", "thresholds"))):
        for k in keys:
            assert np.array_equal(a["curves"][side][k], b["curves"][side][k]), (side, k)


@pytest.mark.parametrize("kind", ["gcn2", "gcn3"])
def test_device_prepared_square_end_to_end(gpu, er_world, tmp_path, monkeypatch, kind):
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN, GCN3
    adj, w = er_world
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(11)
    model = (GCN(32, 16, 2, 0.5) if kind == "gcn2" else GCN3(32, 16, 8, 2, 0.5)).to(gpu).eval()
    host, dev = Attacker(_args(), model, w), Attacker(_args(), model, w)
    host.prepare_test_data()
    dev.prepare_test_data(pairs="device")
    assert np.array_equal(host.test_nodes, dev.test_nodes)
    assert "_exist_edges" not in dev.__dict__
    _same_curves(host.evaluate(curves=True), dev.evaluate(curves=True))
    a, b = host.recover_edges(), dev.recover_edges()
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert b["is_edge"].dtype == bool and b["is_edge"].any() and b["n_edges"] == len(host.exist_edges)
    rec = dev.recover_edges(beliefs=[0.5, 0.01])
    ref = host.recover_edges(beliefs=[0.5, 0.01])
    assert np.array_equal(rec["is_edge"], ref["is_edge"]) and np.array_equal(rec["tp"], ref["tp"])
    assert "_exist_edges" not in dev.__dict__                        # neither evaluate nor recover_edges built the host lists
    assert isinstance(dev.exist_edges, np.ndarray) and dev.exist_edges.dtype == host.exist_edges.dtype
    assert np.array_equal(dev.exist_edges, host.exist_edges) and np.array_equal(dev.nonexist_edges, host.nonexist_edges)
    if kind == "gcn2":
        host.link_prediction_attack_efficient()
        name = host.result_filename()
        want = torch.load(name, weights_only=False)["result"]
        os.remove(name)
        fresh = Attacker(_args(), model, w)
        fresh.prepare_test_data(pairs="device")
        fresh.link_prediction_attack_efficient()                    # asks for the host lists: materialised from the triangle
        got = torch.load(name, weights_only=False)["result"]
        assert got["y"] == want["y"] and np.array_equal(np.asarray(got["pred"]), np.asarray(want["pred"]))
        # naive attack on a device-prepared square falls back to the host lists
        nh, nd = Attacker(_args(attack_mode="naive", n_test=20), model, w), Attacker(_args(attack_mode="naive", n_test=20), model, w)
        nh.prepare_test_data()
        nd.prepare_test_data(pairs="device")
        _same_curves(nh.evaluate(curves=True), nd.evaluate(curves=True))
    # a host preparation after a device one is the host route again
    dev.prepare_test_data()
    assert dev._sample_dev is None and "_exist_edges" in dev.__dict__


def test_philox_balanced_end_to_end(gpu, er_world):
    from linkteller_amd import engine
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN
    adj, w = er_world
    torch.manual_seed(11)
    model = GCN(32, 16, 2, 0.5).to(gpu).eval()
    want = S.balanced_pairs(adj, 42)
    for am in ("efficient", "naive"):
        atk = Attacker(_args(sample_type="balanced-full", attack_mode=am), model, w)
        assert atk.args.n_test == 300
        with pytest.raises(ValueError):
            Attacker(_args(), model, w).prepare_test_data(rng="philox")
        atk.prepare_test_data(rng="philox")
        assert atk.test_nodes == list(range(300)) and "_exist_edges" not in atk.__dict__
        out = atk.evaluate(curves=True)
        assert "_exist_edges" not in atk.__dict__                    # the lists stayed on the device
        ex, nex = atk.exist_edges, atk.nonexist_edges
        assert np.array_equal(ex, want["edges"]) and np.array_equal(nex, want["non_edges"])
        p, o = (1, 0) if am == "naive" else (0, 1)
        scores = atk.pair_scores(np.concatenate([ex[:, p], nex[:, p]]), np.concatenate([ex[:, o], nex[:, o]]))
        labels = np.zeros(len(scores), dtype=np.uint8)
        labels[:len(ex)] = 1
        curve = engine.score_curve(torch.from_numpy(scores.astype(np.float32)).to(gpu), torch.from_numpy(labels).to(gpu))
        ref = curve.summary()
        from linkteller_amd import metrics as lt_metrics
        ref["curves"] = lt_metrics.curves_from_counts(*curve.counts())
        _same_curves(out, ref)
        assert out["n_pos"] == out["n_neg"] == 1500


def test_cli_sample_switches_end_to_end(gpu, tmp_path, monkeypatch, capsys):
    """--sample-build device prints the host route's auc / ap (the same sample, the same labels); --sample-rng philox runs
    balanced-full; neither builds a host pair list."""
    import re
    from test_cli_worker_dp import _write_musae
    from linkteller_amd import attacker as lt_attacker, main as lt_main, synth
    from linkteller_amd.gcn import GCN
    a1, a2 = synth.powerlaw_graph(260, 1200, seed=1), synth.powerlaw_graph(320, 1500, seed=2)
    _write_musae(str(tmp_path), "ES", a1, 400, 1)
    _write_musae(str(tmp_path), "RU", a2, 400, 2)
    torch.manual_seed(0)
    torch.save(GCN(3170, 256, 2, 0.5).state_dict(), tmp_path / "model.pt")
    monkeypatch.chdir(tmp_path)
    base = (f"--mode vanilla-clean --dataset twitch/ES/RU --hidden 256 --norm FirstOrderGCN --test --model-path {tmp_path}/model.pt "
            f"--attack --attack-mode efficient --n-test 60 --data-root {tmp_path} --metrics-only").split()

    def numbers(argv):
        lt_main.main(argv)
        out = capsys.readouterr().out
        return [float(re.search(rf"^{k} = (\S+)$", out, flags=re.M).group(1)) for k in ("auc", "ap")]

    host = numbers(base + ["--sample-type", "unbalanced"])
    monkeypatch.setattr(lt_attacker.Attacker, "_materialise_pairs", lambda self: pytest.fail("the host lists were built"))
    assert numbers(base + ["--sample-type", "unbalanced", "--sample-build", "device"]) == host
    got = numbers(base + ["--sample-type", "balanced-full", "--sample-rng", "philox"])
    assert 0.5 < got[0] <= 1.0 and 0.5 < got[1] <= 1.0
    assert not os.path.exists("eval_twitch")

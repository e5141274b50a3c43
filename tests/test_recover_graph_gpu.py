"""Edge recovery through the streaming selector: ``Attacker.recover_edges(chunk=K)`` against the one-shot route array for
array, ``Attacker.recover_graph`` against ``recover_edges`` on an attacker whose sample is the whole graph (or the same
subset), and the command line's --recover-chunk / --recover-nodes."""
import argparse
import os
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def er_world(gpu):
    from linkteller_amd import graph, synth
    adj = synth.erdos_renyi_graph(300, 1500, seed=3)
    x = torch.from_numpy(synth.gaussian_features(300, 32, seed=4)).to(gpu)
    adj_t = graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(adj)).to(gpu)
    return adj, types.SimpleNamespace(features_2=x, adj_2=adj_t, adj_ori=adj, n_nodes=300)


def _model(kind, gpu):
    from linkteller_amd.gcn import GCN, GCN3
    torch.manual_seed(11)
    m = {"gcn2": lambda: GCN(32, 16, 2, 0.5), "gcn3": lambda: GCN3(32, 16, 8, 2, 0.5),
         "gcn2-wide": lambda: GCN(32, 320, 12, 0.5), "gcn3-wide-class": lambda: GCN3(32, 16, 12, 41, 0.5)}[kind]()
    return m.to(gpu).eval()


def _attacker(kind, w, gpu, n_test=300):
    from linkteller_amd.attacker import Attacker
    args = argparse.Namespace(dataset="twitch/x", sample_type="unbalanced", n_test=n_test, sample_seed=42, influence=1e-4,
                              mode="vanilla-clean", attack_mode="efficient", influence_mode="delta")
    return Attacker(args, _model(kind, gpu), w)


def _same(a, b, tag):
    assert set(a) == set(b), tag
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (tag, k)
        else:
            assert type(x) is type(y) and x == y, (tag, k, x, y)


def _whole_graph_sample(atk, adj):
    """The sample that names every node: what prepare_test_data would leave for test_nodes = arange(N)."""
    import scipy.sparse as sp
    n = adj.shape[0]
    up = sp.triu(sp.csr_matrix(adj), 1).tocoo()
    atk.test_nodes = list(range(n))
    atk.exist_edges = [(int(a), int(b)) for a, b in zip(up.row, up.col)]
    atk.nonexist_edges = []
    return len(atk.exist_edges)


@pytest.mark.parametrize("kind", ["gcn2", "gcn3", "gcn2-wide", "gcn3-wide-class"])
def test_recover_edges_chunked_equals_one_shot(gpu, er_world, kind):
    adj, w = er_world
    atk = _attacker(kind, w, gpu)
    _whole_graph_sample(atk, adj)
    want = dict(atk.recover_edges())
    assert len(want["pairs"]) == int(max(want["counts"])) > 0
    for chunk in (1, 37, 300, 1000):
        got = atk.recover_edges(chunk=chunk)
        _same(got, want, f"{kind} chunk={chunk}")
        assert atk.recover_stream_stats["pushes"] == -(-300 // min(chunk, 300))
    with pytest.raises(ValueError):
        atk.recover_edges(chunk=0)


@pytest.mark.parametrize("kind", ["gcn2", "gcn3"])
def test_recover_graph_equals_recover_edges_on_the_whole_graph(gpu, er_world, kind):
    adj, w = er_world
    atk = _attacker(kind, w, gpu)
    n_edges = _whole_graph_sample(atk, adj)
    for beliefs in (None, [0.5, 0.01]):
        want = dict(atk.recover_edges(beliefs=beliefs))
        fresh = _attacker(kind, w, gpu)              # no prepare_test_data(), no pair lists
        got = fresh.recover_graph(beliefs=beliefs, chunk=64)
        assert got is fresh.recovered
        _same(got, want, f"{kind} beliefs={beliefs}")
        assert got["n_edges"] == n_edges and got["n_total"] == 300 * 299 // 2
        is_edge = np.asarray(adj[got["pairs"][:, 0], got["pairs"][:, 1]]).reshape(-1) != 0
        assert np.array_equal(got["is_edge"], is_edge) and 0 < int(is_edge.sum()) < len(is_edge)
    _same(fresh.recover_graph(beliefs=[0.5, 0.01], chunk=1024), want, "one chunk")


def test_recover_graph_on_a_subset_equals_the_sampled_route(gpu, er_world):
    adj, w = er_world
    atk = _attacker("gcn2", w, gpu, n_test=64)
    atk.prepare_test_data()
    want = dict(atk.recover_edges())
    fresh = _attacker("gcn2", w, gpu, n_test=64)
    got = fresh.recover_graph(nodes=atk.test_nodes, chunk=17)
    _same(got, want, "subset")
    assert got["n_edges"] == len(atk.exist_edges) and got["n_total"] == 64 * 63 // 2
    with pytest.raises(ValueError):
        fresh.recover_graph(nodes=[5])


def test_cli_recover_chunk_and_all_nodes(gpu, tmp_path, monkeypatch, capsys):
    import scipy.sparse as sp
    from test_cli_worker_dp import _write_musae
    from linkteller_amd import main as lt_main, synth
    from linkteller_amd.gcn import GCN
    a1, a2 = synth.powerlaw_graph(260, 1200, seed=1), synth.powerlaw_graph(320, 1500, seed=2)
    _write_musae(str(tmp_path), "ES", a1, 400, 1)
    _write_musae(str(tmp_path), "RU", a2, 400, 2)
    torch.manual_seed(0)
    torch.save(GCN(3170, 256, 2, 0.5).state_dict(), tmp_path / "model.pt")
    monkeypatch.chdir(tmp_path)
    base = (f"--mode vanilla-clean --dataset twitch/ES/RU --hidden 256 --norm FirstOrderGCN --test --model-path {tmp_path}/model.pt "
            f"--attack --attack-mode efficient --sample-type unbalanced --n-test 60 --data-root {tmp_path}").split()
    recover_file = "eval_twitch/ES/RU/recover_efficient_unbalanced_60_42.pt"
    all_file = "eval_twitch/ES/RU/recover_all_efficient_unbalanced_60_42.pt"

    lt_main.main(base + ["--recover"])
    capsys.readouterr()
    one_shot = torch.load(recover_file, weights_only=False)
    os.remove(recover_file)
    lt_main.main(base + ["--recover", "--recover-chunk", "64"])
    out = capsys.readouterr().out
    assert f"recovered edges saved to: {recover_file}" in out and not os.path.exists(all_file)
    _same(torch.load(recover_file, weights_only=False), one_shot, "--recover-chunk 64")
    os.remove(recover_file)

    lt_main.main(base + ["--recover", "--recover-nodes", "all", "--recover-chunk", "64"])
    out = capsys.readouterr().out
    assert "the sampled AUC attack is skipped" in out and "attack results saved" not in out
    assert f"recovered edges saved to: {all_file}" in out and os.path.exists(all_file) and not os.path.exists(recover_file)
    rec = torch.load(all_file, weights_only=False)
    assert set(rec) == set(one_shot)
    n = 320
    assert rec["n_total"] == n * (n - 1) // 2 and rec["n_edges"] == sp.triu(sp.csr_matrix(a2), 1).nnz
    assert len(rec["beliefs"]) == 5 and len(rec["pairs"]) == int(max(rec["counts"]))
    lines = re.findall(r"belief = (\S+), m = (\d+), tp = (\d+), precision = (\S+), recall = (\S+), f1 = (\S+)", out)
    assert len(lines) == 5
    for k, (b, m, tp, p, r, f) in enumerate(lines):
        assert b == f"{rec['beliefs'][k]:.6g}" and int(m) == int(rec["counts"][k]) and int(tp) == int(rec["tp"][k])
        assert (p, r, f) == (f"{rec['precision'][k]:.4f}", f"{rec['recall'][k]:.4f}", f"{rec['f1'][k]:.4f}")
    is_edge = np.asarray(sp.csr_matrix(a2)[rec["pairs"][:, 0], rec["pairs"][:, 1]]).reshape(-1) != 0      # (the Worker's adj_ori is a2)
    assert rec["is_edge"].dtype == bool and np.array_equal(rec["is_edge"], is_edge) and 0 < int(is_edge.sum()) < len(is_edge)
    assert np.array_equal(rec["tp"], np.array([int(is_edge[:int(c)].sum()) for c in rec["counts"]]))

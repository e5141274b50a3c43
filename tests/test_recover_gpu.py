"""Edge recovery on the GPU: lt_top_pairs_lower against its host restatement (exact: indices, score bits, tie counts), through
the attacker on 2- and 3-layer models, and through the command line.

The restatement used throughout, with ``M`` the matrix brought back from the device:
    ii, jj = np.tril_indices(n, -1); flat = ii * n + jj; v = M[ii, jj] + np.float32(0)
    order = np.lexsort((flat, -v.astype(np.float64))); expect = np.sort(flat[order[:m]])
"""
import argparse
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ranked(M):
    """(flat, v, order) of the restatement: the strict lower triangle's cells in flat order, their canonical values, rank order."""
    n = M.shape[0]
    ii, jj = np.tril_indices(n, -1)
    flat = ii.astype(np.int64) * n + jj
    v = M[ii, jj] + np.float32(0)
    order = np.lexsort((flat, -v.astype(np.float64)))
    return flat, v, order


def _expect(flat, v, order, m):
    thr = v[order[m - 1]]
    above = int((v > thr).sum())
    return np.sort(flat[order[:m]]), thr, above, m - above, int((v == thr).sum())


def _matrix(n, lds, values):
    """[n, lds] with +inf on the diagonal, in the upper triangle and in the padding columns: any read outside the region wins
    the selection.  ``values``: the n (n - 1) / 2 cells of the strict lower triangle in flat order."""
    buf = np.full((n, lds), np.inf, dtype=np.float32)
    ii, jj = np.tril_indices(n, -1)
    buf[ii, jj] = values
    return buf


def _values(cls, total, rng):
    if cls == "a":      # distinct normal draws with negatives
        # fp32 draws repeat once there are ~1e5 of them: oversample, drop the repeats, keep `total` in shuffled order
        pool = np.unique(rng.standard_normal(2 * total + 16).astype(np.float32))
        assert pool.size >= total
        return rng.permutation(pool)[:total]
    if cls == "b":      # 93 % exact +0, positive draws elsewhere
        v = np.zeros(total, dtype=np.float32)
        pos = rng.random_sample(total) < 0.07
        if total > 1 and not pos.any():
            pos[rng.randint(total)] = True
        v[pos] = (rng.random_sample(int(pos.sum())) + 0.05).astype(np.float32)
        return v
    if cls == "c":      # every cell equal
        return np.full(total, 0.25, dtype=np.float32)
    pool = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 3e-39, 1.5, 1.5, -2.0, 3.25, 3.25, -np.inf, np.inf], dtype=np.float32)
    prob = np.array([20, 20, 8, 8, 8, 8, 6, 6, 6, 4, 4, 1, 1], dtype=np.float64)
    return pool[rng.choice(pool.size, size=total, p=prob / prob.sum())]


def _check_case(gpu, engine, dev_scores, M, ranked, m, tag):
    n = M.shape[0]
    idx, val, info = engine.top_pairs_lower(dev_scores, m)
    idx2, val2, info2 = engine.top_pairs_lower(dev_scores, m)
    got_idx, got_val, raw = idx.cpu().numpy(), val.cpu().numpy(), info["raw"].cpu().numpy()
    exp_idx, thr, above, tied_taken, tied_total = _expect(*ranked, m)
    assert got_idx.shape == (m,) and np.array_equal(got_idx, exp_idx), tag
    assert np.all(np.diff(got_idx) > 0), tag
    assert np.array_equal(got_val.view(np.int32), M.reshape(-1)[exp_idx].view(np.int32)), tag      # bitwise, -0.0 stays -0.0
    assert int(raw[0]) == int(np.array([thr], dtype=np.float32).view(np.uint32)[0]), tag
    assert (int(raw[1]), int(raw[2]), int(raw[3])) == (above, tied_taken, tied_total), tag
    assert (int(info["above"]), int(info["tied_taken"]), int(info["tied_total"])) == (above, tied_taken, tied_total), tag
    assert torch.equal(idx, idx2) and torch.equal(val.view(torch.int32), val2.view(torch.int32)), tag
    assert torch.equal(info["raw"], info2["raw"]), tag


@pytest.mark.parametrize("n", [2, 3, 64, 65, 257, 500])
def test_top_pairs_lower_synthetic(gpu, n):
    from linkteller_amd import engine
    total = n * (n - 1) // 2
    rng = np.random.RandomState(1000 + n)
    base_ms = sorted({mm for mm in (1, 2, total // 2, total - 1, total) if 1 <= mm <= total})
    for cls in "abcd":
        values = _values(cls, total, rng)
        ms = list(base_ms)
        if cls == "b":
            P = int((values > 0).sum())
            ms = sorted(set(ms) | {mm for mm in (P - 1, P, P + 1, P + (total - P) // 2) if 1 <= mm <= total})
        ranked = None
        for lds in (n, n + 3):
            host = _matrix(n, lds, values)
            dev = torch.from_numpy(host).to(gpu)
            M = np.ascontiguousarray(host[:, :n])
            if ranked is None:
                ranked = _ranked(M)
            for m in ms:
                _check_case(gpu, engine, dev[:, :n], M, ranked, m, f"n={n} class={cls} lds={lds} m={m}")


def test_top_pairs_lower_view_into_larger_buffer(gpu):
    from linkteller_amd import engine
    n = 65
    total = n * (n - 1) // 2
    rng = np.random.RandomState(7)
    M = _matrix(n, n, _values("b", total, rng))
    big = torch.full((n + 5, n + 7), float("inf"), dtype=torch.float32, device=gpu)
    big[:n, :n] = torch.from_numpy(M).to(gpu)
    contiguous = torch.from_numpy(M).to(gpu)
    ranked = _ranked(M)
    P = int((M[np.tril_indices(n, -1)] > 0).sum())
    for m in (1, P, P + 7, total // 2, total):
        a = engine.top_pairs_lower(big[:n, :n], m)
        b = engine.top_pairs_lower(contiguous, m)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        assert torch.equal(a[2]["raw"], b[2]["raw"])
        assert np.array_equal(a[0].cpu().numpy(), _expect(*ranked, m)[0])
    with pytest.raises(ValueError):
        engine.top_pairs_lower(contiguous, 0)
    with pytest.raises(ValueError):
        engine.top_pairs_lower(contiguous, total + 1)
    with pytest.raises(ValueError):
        engine.top_pairs_lower(contiguous.t(), 3)                  # last-dimension stride != 1
    from linkteller_amd import _lib
    with pytest.raises(_lib.LinkTellerHipError):
        engine.top_pairs_lower(torch.from_numpy(M), 3)             # a CPU tensor


@pytest.fixture(scope="module")
def er_world(gpu):
    from linkteller_amd import graph, synth
    adj = synth.erdos_renyi_graph(300, 1500, seed=3)
    x = torch.from_numpy(synth.gaussian_features(300, 32, seed=4)).to(gpu)
    adj_t = graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(adj)).to(gpu)
    return adj, types.SimpleNamespace(features_2=x, adj_2=adj_t, adj_ori=adj, n_nodes=300)


def _check_recovered(atk, rec, M, adj, beliefs_expected=None):
    from linkteller_amd import recover
    nodes = np.asarray(atk.test_nodes, dtype=np.int64)
    n = len(nodes)
    flat, v, order = _ranked(M)
    counts = np.asarray(rec["counts"])
    if beliefs_expected is not None:
        assert list(rec["beliefs"]) == list(beliefs_expected)
    assert np.array_equal(counts, recover.belief_counts(rec["beliefs"], n * (n - 1) // 2))
    m = int(counts.max())
    top = flat[order[:m]]
    i, j = top // n, top % n
    assert rec["pairs"].dtype == np.int64 and np.array_equal(rec["pairs"], np.stack([nodes[j], nodes[i]], axis=1))
    assert rec["scores"].dtype == np.float64 and np.array_equal(rec["scores"], M[i, j].astype(np.float64))
    is_edge = np.asarray(adj[nodes[j], nodes[i]]).reshape(-1) != 0
    assert rec["is_edge"].dtype == bool and np.array_equal(rec["is_edge"], is_edge)
    stats = recover.recovery_stats(is_edge, len(atk.exist_edges), counts)
    for k in ("tp", "precision", "recall", "f1"):
        assert np.array_equal(rec[k], stats[k]), k
    assert rec["threshold"] == float(v[order[m - 1]])
    for mk in counts:                                               # every belief's prediction is a prefix of the ranked list
        exp_idx = _expect(flat, v, order, int(mk))[0]
        pref = rec["pairs"][:int(mk)]
        back = np.searchsorted(nodes[np.argsort(nodes)], pref)
        pos = np.argsort(nodes)[back]
        assert np.array_equal(np.sort(pos[:, 1] * n + pos[:, 0]), exp_idx)
    return m, int((v != 0).sum())


@pytest.mark.parametrize("kind", ["gcn2", "gcn3"])
def test_recover_edges_through_the_models(gpu, er_world, kind):
    """``recover_edges`` against the restatement applied to ``_rows`` brought to the host, for the reference's ladder and for an
    explicit belief list.  On this graph (300 nodes, 1500 edges, 64 sampled) the ladder's 4r rung takes 242 of the 2016 pairs while
    ~590 pairs lie within two hops, so the ladder alone stops short of the zero block; the belief 0.5 (1008 pairs) is what cuts
    inside it on the 2-layer model, and the test asserts that it does."""
    from linkteller_amd import recover
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN, GCN3
    adj, w = er_world
    torch.manual_seed(11)
    model = (GCN(32, 16, 2, 0.5) if kind == "gcn2" else GCN3(32, 16, 8, 2, 0.5)).to(gpu).eval()
    reached_zero_block = False
    for mode in ("delta", "sparse"):
        args = argparse.Namespace(dataset="twitch/x", sample_type="unbalanced", n_test=64, sample_seed=42, influence=1e-4,
                                  mode="vanilla-clean", attack_mode="efficient", influence_mode=mode)
        atk = Attacker(args, model, w)
        atk.prepare_test_data()
        nodes = np.asarray(atk.test_nodes, dtype=np.int64)
        M = atk._rows(nodes, nodes).cpu().numpy()
        assert M.dtype == np.float32 and M.shape == (64, 64)
        ladder = recover.density_ladder(len(atk.exist_edges), 64)
        for beliefs in (None, [0.5, 0.01, 0.25]):
            rec = atk.recover_edges(beliefs=beliefs)
            assert rec is atk.recovered
            m, nonzero = _check_recovered(atk, rec, M, adj, ladder if beliefs is None else beliefs)
            print(f"{kind} {mode} beliefs={'ladder' if beliefs is None else beliefs}: m={m} of 2016, nonzero cells={nonzero}")
            if m > nonzero:
                assert rec["threshold"] == 0.0 and rec["tied_total"] > rec["tied_taken"] > 0
                reached_zero_block = True
    if kind == "gcn2":
        assert reached_zero_block, "no case cut inside the zero block: the tie path was not exercised"
    args.sample_type = "balanced-full"
    with pytest.raises(NotImplementedError):
        Attacker(args, model, w).recover_edges()


def test_cli_recover_end_to_end(gpu, tmp_path, monkeypatch, capsys):
    from test_cli_worker_dp import _write_musae
    from linkteller_amd import main as lt_main, synth
    from linkteller_amd.gcn import GCN
    from linkteller_amd.sampling import construct_edge_sets_from_random_subgraph
    from linkteller_amd.worker import Worker
    a1, a2 = synth.powerlaw_graph(260, 1200, seed=1), synth.powerlaw_graph(320, 1500, seed=2)
    _write_musae(str(tmp_path), "ES", a1, 400, 1)
    _write_musae(str(tmp_path), "RU", a2, 400, 2)
    torch.manual_seed(0)
    torch.save(GCN(3170, 256, 2, 0.5).state_dict(), tmp_path / "model.pt")
    monkeypatch.chdir(tmp_path)
    base = (f"--mode vanilla-clean --dataset twitch/ES/RU --hidden 256 --norm FirstOrderGCN --test --model-path {tmp_path}/model.pt "
            f"--attack --attack-mode efficient --sample-type unbalanced --n-test 60 --data-root {tmp_path}").split()
    result_file = "eval_twitch/ES/RU/efficient_unbalanced_60_42.pt"
    recover_file = "eval_twitch/ES/RU/recover_efficient_unbalanced_60_42.pt"
    lt_main.main(base)
    out = capsys.readouterr().out
    assert "recovered edges saved" not in out
    import os
    assert not os.path.exists(recover_file)
    plain = open(result_file, "rb").read()

    lt_main.main(base + ["--recover"])
    out = capsys.readouterr().out
    assert f"attack results saved to: {result_file}" in out and f"recovered edges saved to: {recover_file}" in out
    assert open(result_file, "rb").read() == plain                 # the attack's own file: byte for byte
    rec = torch.load(recover_file, weights_only=False)
    for k in ("pairs", "scores", "is_edge", "beliefs", "counts", "precision", "recall", "f1", "tp", "threshold"):
        assert k in rec, k
    assert len(rec["beliefs"]) == 5 and out.count("belief = ") == 5

    # the restatement on the saved score list: pair (nodes[a], nodes[b]), a < b, is cell (b, a)
    saved = torch.load(result_file, weights_only=False)
    pred, y = np.asarray(saved["result"]["pred"]), np.asarray(saved["result"]["y"])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    w = Worker(argparse.Namespace(norm="FirstOrderGCN"), "twitch/ES/RU", "vanilla-clean", data_root=str(tmp_path))
    monkeypatch.undo(); monkeypatch.chdir(tmp_path)
    np.random.seed(42)
    (ex, nex), nodes = construct_edge_sets_from_random_subgraph("twitch/ES/RU", "unbalanced", w.adj_ori, 60)
    capsys.readouterr()
    pairs = np.concatenate([np.asarray(ex).reshape(-1, 2), np.asarray(nex).reshape(-1, 2)])
    assert len(pairs) == len(pred) == 1770 and int(y.sum()) == len(ex)
    ind = {int(v): k for k, v in enumerate(nodes)}
    cell = np.array([ind[int(b)] * 60 + ind[int(a)] for a, b in pairs], dtype=np.int64)
    order = np.lexsort((cell, -pred))
    for k, m in enumerate(rec["counts"]):
        assert int(rec["tp"][k]) == int(y[order[:int(m)]].sum())
    top = order[:int(max(rec["counts"]))]
    assert np.array_equal(rec["pairs"], pairs[top]) and np.array_equal(rec["scores"], pred[top])
    assert np.array_equal(rec["is_edge"], y[top].astype(bool))

    lt_main.main(base + ["--recover", "--density-belief", "0.01"])
    out = capsys.readouterr().out
    one = torch.load(recover_file, weights_only=False)
    assert list(one["beliefs"]) == [0.01] and list(one["counts"]) == [18] and out.count("belief = ") == 1
    assert len(one["pairs"]) == 18 and int(one["tp"][0]) == int(y[order[:18]].sum())
    assert open(result_file, "rb").read() == plain

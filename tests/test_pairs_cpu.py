"""The pair-list primitive (lt_influence_pairs) and the naive attack, as far as they go without a GPU: the ABI's host-side
refusals, ``engine.group_pairs`` against a brute-force regrouping, and ``GCNTrainer.eval_output`` with ``--attack-mode naive``
down to the result file, with the one device step (``Attacker.pair_scores``) replaced by the fp64 oracle."""
import argparse
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from conftest import csr_from, load_golden


@pytest.fixture(scope="module")
def lt():
    from linkteller_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_pairs_symbols_and_host_side_refusals(lt):
    h = lt.lib()
    for name in ("lt_influence_pairs", "lt_influence_pairs_workspace_bytes"):
        assert hasattr(h, name) and name in lt.SIGNATURES
    assert h.lt_abi_version() == 5
    ptr = (C.c_int64 * 2)(0, 1)
    assert h.lt_influence_pairs(None, None, 1, ptr, None, 1, 1e-4, 2, None, None, 0, None) == -1
    assert b"baseline" in h.lt_last_error()
    assert h.lt_influence_pairs_workspace_bytes(None, 10, 100, 2) == 0


def _brute_force(probe, observed):
    """The grouped layout by definition: distinct probes ascending; each probe's partners in input order."""
    nodes = sorted(set(int(p) for p in probe))
    ptr, obs, src = [0], [], []
    for v in nodes:
        for k, (p, u) in enumerate(zip(probe, observed)):
            if int(p) == v:
                obs.append(int(u))
                src.append(k)
        ptr.append(len(obs))
    return nodes, ptr, obs, src


@pytest.mark.parametrize("case", ["random", "duplicates", "one_probe", "sorted", "empty"])
def test_group_pairs_against_brute_force(case):
    from linkteller_amd import engine
    rng = np.random.RandomState({"random": 1, "duplicates": 2, "one_probe": 3, "sorted": 4, "empty": 5}[case])
    if case == "random":
        probe, observed = rng.randint(0, 50, 300), rng.randint(0, 50, 300)
    elif case == "duplicates":
        probe, observed = rng.randint(0, 4, 200), rng.randint(0, 3, 200)       # every pair several times over
    elif case == "one_probe":
        probe, observed = np.full(17, 9), rng.randint(0, 50, 17)
    elif case == "sorted":
        probe, observed = np.sort(rng.randint(0, 50, 100)), rng.randint(0, 50, 100)
    else:
        probe, observed = np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64)
    nodes, ptr, obs, order = engine.group_pairs(probe, observed)
    r_nodes, r_ptr, r_obs, r_src = _brute_force(probe, observed)
    assert nodes.dtype == np.int32 and obs.dtype == np.int32 and ptr.dtype == np.int64
    assert nodes.tolist() == r_nodes and ptr.tolist() == r_ptr and obs.tolist() == r_obs
    assert order.tolist() == r_src                                  # stable: a probe's pairs keep their input order
    assert ptr[0] == 0 and ptr[-1] == len(probe) and len(ptr) == len(nodes) + 1
    # round trip through `order`: grouped scores back into input order
    grouped = np.array([1000.0 * r_nodes[np.searchsorted(r_ptr, k, side="right") - 1] + obs[k] for k in range(len(obs))])
    scores = np.empty(len(order))
    scores[order] = grouped
    assert np.array_equal(scores, 1000.0 * np.asarray(probe, dtype=np.float64) + np.asarray(observed, dtype=np.float64))
    with pytest.raises(ValueError):
        engine.group_pairs([1, 2], [1])


@pytest.mark.parametrize("mode", ["vanilla-clean", "vanilla"])
def test_naive_attack_through_eval_output(mode, monkeypatch, tmp_path, capsys):
    """``--attack-mode naive`` reaches ``Attacker.link_prediction_attack`` (attacker.py:143-201): all existing pairs, then all
    non-existing ones, each (u, v) scored as probe v / observed u, the reference's two timing prints, auc / ap, and the naive
    file name -- ``oracle.result_filename`` without the attack-mode prefix -- with the shared schema."""
    from oracle import linkteller_oracle as O
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.trainer import GCNTrainer
    g = load_golden("next_rows.npz")
    a = csr_from(g, "adj")
    x = torch.from_numpy(g["x"])
    P64 = {k: g[f"sd.{n}"].astype(np.float64) for k, n in (("W1", "gc1.weight"), ("b1", "gc1.bias"), ("W2", "gc2.weight"), ("b2", "gc2.bias"))}
    ro = O.RestrictedOracle(g["x"], O.first_order_gcn(a), P64)
    calls = []

    def oracle_pair_scores(self, probe, observed, mode=None):
        probe, observed = np.asarray(probe, dtype=np.int64), np.asarray(observed, dtype=np.int64)
        calls.append((probe.copy(), observed.copy()))
        return np.array([ro.rows([v], [u], 1e-4)[0, 0] for v, u in zip(probe, observed)])

    monkeypatch.setattr(Attacker, "pair_scores", oracle_pair_scores)
    monkeypatch.chdir(tmp_path)
    n = a.shape[0]
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=24, sample_seed=42, influence=1e-4,
                              mode=mode, attack_mode="naive", attack=True, perturb_type="discrete", epsilon=5.0, noise_seed=7)
    labels = torch.from_numpy((np.arange(n) % 2).astype(np.int64))
    w = types.SimpleNamespace(features_2=x, adj_2=None, adj_ori=a, n_nodes=n, mode=mode, dataset="twitch/ES/RU",
                              labels_2=labels, transfer=True)
    tr = GCNTrainer(args, worker=w)
    tr.model = None
    out = torch.zeros((n, 2))
    out[:, 0] = 1.0
    tr.eval_output(out)                    # NotImplementedError before the naive attack existed
    atk = tr.attacker
    ex = np.asarray(atk.exist_edges, dtype=np.int64).reshape(-1, 2)
    nex = np.asarray(atk.nonexist_edges, dtype=np.int64).reshape(-1, 2)
    assert len(ex) > 0 and len(nex) > 0
    # two calls: every existing pair, then every non-existing one; probe = v (second node), observed = u (first node)
    assert len(calls) == 2
    assert np.array_equal(calls[0][0], ex[:, 1]) and np.array_equal(calls[0][1], ex[:, 0])
    assert np.array_equal(calls[1][0], nex[:, 1]) and np.array_equal(calls[1][1], nex[:, 0])
    text = capsys.readouterr().out
    i_ex, i_nex = text.index("time for predicting existing edges: "), text.index("time for predicting non-existing edges: ")
    assert i_ex < i_nex < text.index("auc =") < text.index("ap =") < text.index("attacks done using")
    assert "attack results saved" not in text
    full = O.result_filename("twitch/ES/RU", mode, "naive", "unbalanced", 24, 42, "discrete", 5.0, 7)
    folder, name = os.path.split(full)
    assert name.startswith("naive_")
    naive_name = os.path.join(folder, name[len("naive_"):])
    assert atk.naive_result_filename() == naive_name
    assert os.path.exists(naive_name) and not os.path.exists(full)
    saved = torch.load(naive_name, weights_only=False)
    assert set(saved) == {"auc", "pr", "result"} and set(saved["auc"]) == {"fpr", "tpr", "thresholds"}
    assert set(saved["pr"]) == {"precision", "recall", "thresholds"} and set(saved["result"]) == {"y", "pred"}
    assert saved["result"]["y"] == [1] * len(ex) + [0] * len(nex)
    # the scores are the oracle's, pair by pair, in list order -- and the metrics those of the reference's own pair lookup
    nodes = np.asarray(atk.test_nodes, dtype=np.int64)
    infl = ro.rows(nodes, nodes, 1e-4)
    ne, nn = O.pair_scores(infl, list(nodes), ex.tolist(), nex.tolist())
    assert np.allclose(np.asarray(saved["result"]["pred"]), np.asarray(ne + nn), rtol=1e-12, atol=0)
    m = O.attack_metrics(ne, nn)
    assert abs(atk.auc - m["auc"]) <= 1e-12 and abs(atk.ap - m["ap"]) <= 1e-12


def test_get_gradient_eps_is_a_row_of_the_matrix(monkeypatch):
    """attacker.py:89-97 for API parity: row u of get_gradient_eps_mat(v)."""
    from linkteller_amd.attacker import Attacker
    a = Attacker.__new__(Attacker)
    mat = torch.arange(12.0).reshape(6, 2)
    seen = []
    monkeypatch.setattr(Attacker, "get_gradient_eps_mat", lambda self, v: (seen.append(v), mat)[1])
    assert torch.equal(a.get_gradient_eps(4, 1), mat[4]) and seen == [1]

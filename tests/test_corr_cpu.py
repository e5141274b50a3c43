"""The baseline attacks' device scores without a GPU: the shared restatement (tests/corr_restate.py) against the reference's golden
scores, the argument checks of lt_corr_square / lt_corr_pairs that happen before any device call, and the command line's
--baseline-scores with the checks it relaxes.

The golden scores are the reference's fp32 arithmetic; the restatement is fp64.  Their distance is bounded by the reference's own
fp32 error, measured in the test -- the same fp32 arithmetic restated in torch on the CPU against the restatement -- with no
factor and no slack: not a fixed number.  (The golden scores are what torch's fp32 arithmetic gives for these inputs bit for bit,
as tests/test_oracle_golden.py asserts of the oracle; a torch build that summed in another order would fail there first.)"""
import argparse
import os
import types

import numpy as np
import pytest
import torch

import corr_restate as R
from conftest import csr_from, load_golden

DS = "twitch/ES/RU"


@pytest.fixture(scope="module")
def lt():
    from linkteller_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def golden_world():
    """(g, adjacency, {mode: vectors}, sampled nodes, exist, nonexist) of the unbalanced golden sample (n_test = 40, seed 42)."""
    from oracle import linkteller_oracle as O
    from linkteller_amd.sampling import construct_edge_sets_from_random_subgraph
    g = load_golden("next_rows.npz")
    a = csr_from(g, "adj")
    x = torch.from_numpy(g["x"])
    adj = O.to_torch_sparse(O.first_order_gcn(a))
    P = {k: torch.from_numpy(g[f"sd.{n}"]) for k, n in (("W1", "gc1.weight"), ("b1", "gc1.bias"), ("W2", "gc2.weight"), ("b2", "gc2.bias"))}
    np.random.seed(42)
    (ex, nex), nodes = construct_edge_sets_from_random_subgraph(DS, "unbalanced", a, 40)
    vec = {m: O.baseline_vectors(m, x, adj, P, DS).numpy() for m in ("baseline", "baseline-feat")}
    return g, a, vec, np.asarray(nodes, dtype=np.int64), np.asarray(ex).reshape(-1, 2), np.asarray(nex).reshape(-1, 2)


def pair_cells(sq, nodes, pairs):
    ind = np.full(int(nodes.max()) + 1, -1, dtype=np.int64)
    ind[nodes] = np.arange(len(nodes))
    i, j = ind[pairs[:, 0]], ind[pairs[:, 1]]
    return sq[np.minimum(i, j), np.maximum(i, j)]


@pytest.mark.parametrize("mode", ["baseline", "baseline-feat"])
def test_restatement_against_the_golden_square(mode):
    g, a, vec, nodes, ex, nex = golden_world()
    assert np.array_equal(nodes, g[f"{mode}.test_nodes"])
    V = vec[mode]
    assert V.dtype == np.float32 and R.well_conditioned(V, nodes)
    sq = R.square(V, nodes)
    assert np.array_equal(sq, sq.T) or np.abs(sq - sq.T).max() <= R.ORDER_SLACK
    ref_err = float(np.abs(R.fp32_square(V, nodes) - sq).max())          # the reference's own fp32 error on this sample
    bound = ref_err
    for pairs, key in ((ex, "norm_exist"), (nex, "norm_nonexist")):
        gold = g[f"{mode}.{key}"]
        got = pair_cells(sq, nodes, pairs)
        assert got.shape == gold.shape
        err = float(np.abs(got - gold).max())
        print(mode, key, "golden - restatement =", err, "fp32 error =", ref_err, "bound =", bound)
        assert err <= bound
    if mode == "baseline":            # two classes: the centred posteriors are (t, -t), every score is +-1
        assert V.shape[1] == 2 and np.abs(np.abs(sq) - 1.0).max() <= 1e-6


def test_restatement_against_the_golden_pair_list():
    from oracle import linkteller_oracle as O
    g = load_golden("next_rows.npz")
    ab = csr_from(g, "bf.adj")
    xb = torch.from_numpy(g["bf.x"])
    adjb = O.to_torch_sparse(O.first_order_gcn(ab))
    P = {k: torch.from_numpy(g[f"sd.{n}"]) for k, n in (("W1", "gc1.weight"), ("b1", "gc1.bias"), ("W2", "gc2.weight"), ("b2", "gc2.bias"))}
    vec = O.baseline_vectors("baseline", xb, adjb, P, DS)
    V = vec.numpy()
    assert R.well_conditioned(V)
    d = vec - torch.mean(vec, dim=0)                                      # the reference's fp32 arithmetic (attacker.py:337-375)
    nrm = torch.norm(d, dim=1)
    for key, pk in (("norm_exist", "bf.exist"), ("norm_nonexist", "bf.nonexist")):
        pairs = np.asarray(g[pk], dtype=np.int64).reshape(-1, 2)
        u, v = torch.from_numpy(pairs[:, 0]), torch.from_numpy(pairs[:, 1])
        f32 = ((d[u] * d[v]).sum(dim=1) / nrm[u] / nrm[v]).numpy().astype(np.float64)
        got = R.pairs(V, pairs[:, 0], pairs[:, 1])
        ref_err = float(np.abs(f32 - got).max())
        bound = ref_err
        err = float(np.abs(got - g[f"bf.baseline.{key}"]).max())
        print("bf.baseline", key, "golden - restatement =", err, "fp32 error =", ref_err, "bound =", bound)
        assert err <= bound


def test_restatement_inputs_and_degenerate_rows():
    rng = np.random.RandomState(3)
    V = R.normal_rows(rng, 40, 5)
    nodes = np.array([3, 7, 7, 11, 0])
    s = R.square(V, nodes)
    assert s[1, 2] == pytest.approx(1.0, abs=1e-15) and np.array_equal(s[1], s[2])       # a repeated id is a repeated row
    assert np.isnan(R.square(np.full((4, 3), 0.25, dtype=np.float32), np.arange(4))).all()
    assert np.isnan(R.square(V, np.array([5]))).all()                                   # k = 1: the row IS the mean
    p = R.pairs(V, np.array([1, 2]), np.array([1, 5]))
    assert p[0] == pytest.approx(1.0, abs=1e-15) and abs(p[1]) < 1
    for X in (R.softmax_rows(rng, 50, 2), R.softmax_rows(rng, 50, 7), R.indicator_rows(rng, 50, 65)):
        assert X.dtype == np.float32 and np.isfinite(X).all()
    assert not R.well_conditioned(np.array([[1.0, 1.0], [1.0, 1.0 + 1e-6], [1.0, 1.0 - 1e-6], [3.0, -1.0], [-1.0, 3.0]], dtype=np.float32))


def test_corr_argument_errors(lt):
    h = lt.lib()
    q = h.lt_corr_workspace_bytes
    assert q(300, 64, 40, 0) > 0 and q(4385, 3170, 2000, 0) >= 528 * 4096 * 8 and q(4385, 3170, 0, 1000) >= 4385 * 8
    assert q(4385, 7, 0, 0) > 0                                          # empty input: still a valid (minimal) size
    assert q(4385, 3170, 2000, 1000) == max(q(4385, 3170, 2000, 0), q(4385, 3170, 0, 1000))
    assert q(0, 4, 1, 0) == 0 and q(4, 0, 1, 0) == 0 and q(4, 4, -1, 0) == 0 and q(4, 4, 0, -1) == 0 and q(-1, 4, 1, 1) == 0
    # host memory stands in for the device pointers: every check below returns before anything is enqueued or dereferenced
    buf = np.zeros(1 << 17, dtype=np.int64)
    p = buf.ctypes.data
    need = q(100, 8, 10, 0)

    def sq(V=p, ldv=8, n=100, D=8, nodes=p, k=10, out=p, ldo=10, info=p, ws=p, ws_bytes=buf.nbytes):
        return h.lt_corr_square(V, ldv, n, D, nodes, k, out, ldo, info, ws, ws_bytes, None)

    for kw in (dict(V=None), dict(nodes=None), dict(out=None), dict(info=None), dict(ws=None)):
        assert sq(**kw) == -1 and b"NULL" in h.lt_last_error(), kw
    assert sq(ldv=7) == -1 and b"ldv" in h.lt_last_error()
    assert sq(ldo=9) == -1 and b"ldo" in h.lt_last_error()
    assert sq(k=-1) == -1 and sq(n=0) == -1 and sq(n=-3) == -1 and sq(D=0) == -1 and sq(D=-1, ldv=-1) == -1
    assert sq(ws_bytes=need - 1) == -1 and b"workspace" in h.lt_last_error()
    assert sq(ws=p + 4) == -1 and b"aligned" in h.lt_last_error()
    assert sq(ws_bytes=0) == -1
    assert sq(k=0, ldo=0) == 0                                           # empty: a successful no-op, nothing is enqueued
    need = q(100, 8, 0, 50)

    def pr(V=p, ldv=8, n=100, D=8, u=p, v=p, m=50, out=p, info=p, ws=p, ws_bytes=buf.nbytes):
        return h.lt_corr_pairs(V, ldv, n, D, u, v, m, out, info, ws, ws_bytes, None)

    for kw in (dict(V=None), dict(u=None), dict(v=None), dict(out=None), dict(info=None), dict(ws=None)):
        assert pr(**kw) == -1 and b"NULL" in h.lt_last_error(), kw
    assert pr(ldv=7) == -1 and b"ldv" in h.lt_last_error()
    assert pr(m=-1) == -1 and pr(m=2 ** 31) == -1 and pr(n=0) == -1 and pr(D=0) == -1
    assert pr(ws_bytes=need - 1) == -1 and b"workspace" in h.lt_last_error()
    assert pr(ws=p + 4) == -1 and b"aligned" in h.lt_last_error()
    assert pr(m=0) == 0


# ---- the command line -----------------------------------------------------------------------------------------------------------
def _args(s):
    from linkteller_amd import main as lt_main
    return lt_main.get_arguments(s.split())


def test_cli_baseline_scores_flag_and_checks():
    from linkteller_amd import main as lt_main
    assert lt_main.get_arguments([]).baseline_scores == "host"
    with pytest.raises(SystemExit):
        _args("--baseline-scores gpu")
    for am in ("baseline", "baseline-feat"):
        a = _args(f"--test --attack --attack-mode {am} --sample-type unbalanced --baseline-scores device --metrics-only --recover")
        assert a.baseline_scores == "device"
        lt_main.check_baseline_scores(a)
        lt_main.check_metrics_only(a)
        lt_main.check_recover(a)
        b = _args(f"--test --attack --attack-mode {am} --sample-type balanced-full --baseline-scores device --metrics-only")
        lt_main.check_baseline_scores(b)
        lt_main.check_metrics_only(b)
        # --recover stays an unbalanced* thing
        with pytest.raises(NotImplementedError, match="--recover"):
            lt_main.check_recover(_args(f"--attack --attack-mode {am} --sample-type balanced-full --baseline-scores device --recover"))
        # host (explicit or absent) refuses exactly as before
        for flag in ("", " --baseline-scores host"):
            with pytest.raises(NotImplementedError, match="--metrics-only"):
                lt_main.check_metrics_only(_args(f"--attack --attack-mode {am} --sample-type unbalanced --metrics-only" + flag))
            with pytest.raises(NotImplementedError, match="--recover"):
                lt_main.check_recover(_args(f"--attack --attack-mode {am} --sample-type unbalanced --recover" + flag))
            lt_main.check_baseline_scores(_args(f"--attack --attack-mode {am}" + flag))
    # device without a baseline attack / without --attack
    for s in ("--attack --attack-mode efficient --baseline-scores device", "--attack --attack-mode naive --baseline-scores device",
              "--attack-mode baseline --baseline-scores device"):
        with pytest.raises(NotImplementedError, match="--baseline-scores"):
            lt_main.check_baseline_scores(_args(s))
    # a namespace without the attribute (the reference's) is the host route
    ns = argparse.Namespace(attack=True, attack_mode="baseline", sample_type="unbalanced", metrics_only=True, recover=True, density_belief=0.0)
    lt_main.check_baseline_scores(ns)
    with pytest.raises(NotImplementedError):
        lt_main.check_metrics_only(ns)
    with pytest.raises(NotImplementedError):
        lt_main.check_recover(ns)


@pytest.mark.parametrize("argv,match", [
    ("--test --attack --attack-mode efficient --sample-type unbalanced --baseline-scores device", "--baseline-scores"),
    ("--test --attack-mode baseline --sample-type unbalanced --baseline-scores device", "--baseline-scores"),
    ("--test --attack --metrics-only --attack-mode baseline --sample-type unbalanced --baseline-scores host", "--metrics-only"),
    ("--test --attack --recover --attack-mode baseline-feat --sample-type unbalanced", "--recover"),
    ("--test --attack --recover --attack-mode baseline --sample-type balanced-full --baseline-scores device", "--recover"),
])
def test_cli_refusals_come_before_a_worker_is_built(argv, match, monkeypatch):
    from linkteller_amd import main as lt_main, worker

    def boom(*a, **k):
        raise AssertionError("a Worker was built")
    monkeypatch.setattr(worker, "Worker", boom)
    monkeypatch.setattr(lt_main, "init_distributed", boom)
    with pytest.raises(NotImplementedError, match=match):
        lt_main.main(argv.split())


def test_trainer_recover_line_follows_the_flag(monkeypatch):
    """GCNTrainer.eval_output refuses --recover for a baseline attack unless baseline_scores = device (the refusal comes before
    an Attacker is built: the namespace below has nothing else)."""
    from linkteller_amd import trainer as lt_trainer
    t = lt_trainer.GCNTrainer.__new__(lt_trainer.GCNTrainer)
    t.args = argparse.Namespace(attack=True, recover=True, attack_mode="baseline", sample_type="unbalanced")
    with pytest.raises(NotImplementedError, match="recover"):
        t.eval_output(None)
    t.args = argparse.Namespace(attack=True, recover=True, attack_mode="baseline", sample_type="balanced-full", baseline_scores="device")
    with pytest.raises(NotImplementedError, match="recover"):
        t.eval_output(None)

    # ... and admits it with the flag on an unbalanced* sample: the line is passed, the next thing built is the Attacker
    class Reached(Exception):
        pass

    def attacker(**kw):
        raise Reached()
    monkeypatch.setattr(lt_trainer, "Attacker", attacker)
    t.model = t.worker = None
    for am in ("baseline", "baseline-feat"):
        for st in ("unbalanced", "unbalanced-lo", "unbalanced-hi"):
            t.args = argparse.Namespace(attack=True, recover=True, attack_mode=am, sample_type=st, baseline_scores="device")
            with pytest.raises(Reached):
                t.eval_output(None)
            t.args.baseline_scores = "host"
            with pytest.raises(NotImplementedError, match="recover"):
                t.eval_output(None)


def test_device_route_refuses_cpu_features():
    import scipy.sparse as sp
    from linkteller_amd._lib import LinkTellerHipError
    from linkteller_amd.attacker import Attacker
    w = types.SimpleNamespace(features_2=torch.zeros(4, 3), adj_2=None, adj_ori=sp.identity(4, format="csr"), n_nodes=4)
    for am in ("baseline", "baseline-feat"):
        args = argparse.Namespace(dataset="twitch/x", sample_type="unbalanced", n_test=4, attack_mode=am, baseline_scores="device")
        atk = Attacker(args, None, w)
        atk.test_nodes = [0, 1, 2]
        with pytest.raises(LinkTellerHipError):
            atk._baseline_vectors_device()
        with pytest.raises(LinkTellerHipError):
            atk.evaluate()
        with pytest.raises(LinkTellerHipError):
            atk.baseline_attack()
        args.baseline_scores = "host"                                    # host: the refusal of before
        with pytest.raises(NotImplementedError, match="evaluate"):
            atk.evaluate()
    args.baseline_scores = "gpu"
    with pytest.raises(ValueError, match="baseline_scores"):
        atk.evaluate()

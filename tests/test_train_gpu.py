"""Training of the 2-layer GCN on the GPU (engine.GCN2Trainer / lt_gcn2_trainer_*, lt_adam_step) against the numpy
restatements (train_restate.py), fp64 autograd and the reference's 40-epoch trajectories (golden/train.npz)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from conftest import REPO, load_golden
import train_restate as T

pytestmark = pytest.mark.gpu

LR, DECAY = 0.01, 5e-4


@pytest.fixture(scope="module")
def gold():
    return load_golden("train.npz")


def _csr(g, norm, tag):
    n = g[f"{norm}.{tag}.indptr"].shape[0] - 1
    return sp.csr_matrix((g[f"{norm}.{tag}.data"], g[f"{norm}.{tag}.indices"], g[f"{norm}.{tag}.indptr"]), shape=(n, n))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _init(g, norm, h):
    return [_dev(g[f"{norm}.h{h}.init.{k}"].copy()) for k in ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias")]


def _trainer(adj, x, y, params, dropout=0.0, seed=42):
    from linkteller_amd import engine
    return engine.GCN2Trainer(adj, _dev(x), _dev(y), *params, lr=LR, weight_decay=DECAY, dropout=dropout, seed=seed)


def test_adam_step_bitwise_against_restatement():
    from linkteller_amd import _lib
    rng = np.random.RandomState(1)
    n = 10007
    p = (rng.standard_normal(n) * 0.1).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    dp, dm, dv = _dev(p), _dev(m), _dev(v)
    for step in range(1, 6):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 1, n)).astype(np.float32)
        dg = _dev(g)
        _lib.check(_lib.lib().lt_adam_step(n, dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), step, LR, 0.9, 0.999,
                                           1e-8, DECAY, None), "lt_adam_step")
        p, m, v = T.adam_step(p, g, m, v, step, LR, weight_decay=DECAY)
        torch.cuda.synchronize()
        assert np.array_equal(dp.cpu().numpy(), p), step
        assert np.array_equal(dm.cpu().numpy(), m), step
        assert np.array_equal(dv.cpu().numpy(), v), step


def _twitch_shape():
    from linkteller_amd import synth
    n, e, f = 4648, 59382, 3170
    adj = synth.erdos_renyi_graph(n, e, seed=3)
    from linkteller_amd import graph
    return graph.first_order_gcn(adj), synth.twitch_like_features(n, f, seed=4, density=0.006), \
        (np.arange(n) % 2).astype(np.int64)


@pytest.mark.parametrize("case", ["fixture", "twitch"])
def test_first_epoch_logits_equal_forward(gold, case):
    """p = 0: epoch 0's train-mode logits are lt_gcn2_forward's bits (same GEMM slicing, same row chains)."""
    from linkteller_amd import engine, synth
    if case == "fixture":
        adj, x, y = _csr(gold, "AugRWalk", "adj1"), gold["x1"], gold["y1"]
        params = _init(gold, "AugRWalk", 64)
    else:
        adj, x, y = _twitch_shape()
        w = synth.gcn_weights(x.shape[1], 256, 2, seed=5)
        params = [_dev(w[k]) for k in ("W1", "b1", "W2", "b2")]
    ref = engine.gcn2_forward(adj, _dev(x), *params)
    tr = _trainer(adj, x, y, params)
    tr.run(1)
    assert torch.equal(tr.logits(), ref)


def _autograd(adj, x, y, params, keep, scale, dtype):
    coo = adj.tocoo()
    a = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]), coo.data.astype(np.float64), adj.shape).to(dtype).coalesce()
    ps = [torch.from_numpy(np.asarray(p, dtype=np.float64)).to(dtype).requires_grad_() for p in params]
    w1, b1, w2, b2 = ps
    xt = torch.from_numpy(x).to(dtype)
    h = torch.relu(torch.sparse.mm(a, xt @ w1) + b1)
    h = h * torch.from_numpy(keep.astype(np.float64) * float(scale)).to(dtype)
    z = torch.sparse.mm(a, h @ w2) + b2
    F.cross_entropy(z, torch.from_numpy(y)).backward()
    return [p.grad.numpy().astype(np.float64) for p in ps]


@pytest.mark.parametrize("norm", ["FirstOrderGCN", "AugRWalk"])
def test_first_epoch_gradients_against_fp64(gold, norm):
    torch.set_num_threads(1)
    h, p, seed = 64, 0.5, 1234
    adj, x, y = _csr(gold, norm, "adj1"), gold["x1"], gold["y1"]
    init = [gold[f"{norm}.h{h}.init.{k}"] for k in ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias")]
    tr = _trainer(adj, x, y, [_dev(a.copy()) for a in init], dropout=p, seed=seed)
    tr.run(1)
    got = [t.cpu().numpy().astype(np.float64) for t in tr.grads()]
    keep = T.dropout_keep(x.shape[0], h, 0, seed, p)
    scale = T.dropout_scale(p)
    g64 = _autograd(adj, x, y, init, keep, scale, torch.float64)
    g32 = _autograd(adj, x, y, init, keep, scale, torch.float32)
    for name, a, b64, b32 in zip(("dW1", "db1", "dW2", "db2"), got, g64, g32):
        e_hip, e_32 = np.abs(a - b64).max(), np.abs(b32 - b64).max()
        assert e_hip <= 2 * e_32 + 1e-6 * np.abs(b64).max() + 1e-12, (name, e_hip, e_32)


@pytest.mark.parametrize("norm", ["FirstOrderGCN", "AugRWalk"])
@pytest.mark.parametrize("h", [16, 64])
def test_trajectory_against_reference(gold, norm, h):
    from linkteller_amd import engine
    key = f"{norm}.h{h}"
    adj1, adj2 = _csr(gold, norm, "adj1"), _csr(gold, norm, "adj2")
    params = _init(gold, norm, h)
    tr = _trainer(adj1, gold["x1"], gold["y1"], params)
    loss, correct = tr.run(int(gold["epochs"]))
    l64, l32 = gold[f"{key}.loss64"], gold[f"{key}.loss32"]
    assert np.abs(loss - l64).max() <= 2 * np.abs(l32 - l64).max() + 1e-5, (np.abs(loss - l64).max(), np.abs(l32 - l64).max())
    assert np.all(np.abs(correct - gold[f"{key}.correct64"]) <= gold[f"{key}.tiny64"])
    z = engine.gcn2_forward(adj2, _dev(gold["x2"]), *params).cpu().numpy().astype(np.float64)
    z64, z32 = gold[f"{key}.logits2_64"], gold[f"{key}.logits2_32"]
    assert np.abs(z - z64).max() <= 2 * np.abs(z32 - z64).max() + 1e-5 * np.abs(z64).max(), \
        (np.abs(z - z64).max(), np.abs(z32 - z64).max())


def test_deterministic_and_resumable(gold):
    adj, x, y = _csr(gold, "AugRWalk", "adj1"), gold["x1"], gold["y1"]
    runs = []
    for chunks in ([40], [40], [10, 10, 10, 10]):
        params = _init(gold, "AugRWalk", 64)
        tr = _trainer(adj, x, y, params, dropout=0.5, seed=7)
        recs = [tr.run(k) for k in chunks]
        assert tr.epoch == 40
        runs.append((np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs]),
                     [p.cpu().numpy() for p in params]))
    for other in runs[1:]:
        assert np.array_equal(runs[0][0], other[0]) and np.array_equal(runs[0][1], other[1])
        for a, b in zip(runs[0][2], other[2]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("h,c", [(16, 2), (256, 2), (16, 8), (256, 8), (30, 3)])
def test_shapes_run(h, c):
    from linkteller_amd import graph, synth
    n, f = 700, 300
    adj = graph.aug_random_walk(synth.powerlaw_graph(n, 4000, seed=2))
    x = synth.twitch_like_features(n, f, seed=3, density=0.05)
    y = (np.arange(n) * 7 % c).astype(np.int64)
    w = synth.gcn_weights(f, h, c, seed=4)
    params = [_dev(w[k]) for k in ("W1", "b1", "W2", "b2")]
    tr = _trainer(adj, x, y, params, dropout=0.5)
    loss, correct = tr.run(5)
    assert np.all(np.isfinite(loss)) and np.all((correct >= 0) & (correct <= n))
    assert all(bool(torch.isfinite(p).all()) for p in params)


def test_refusals():
    from linkteller_amd import _lib, synth
    n, f = 50, 20
    adj = synth.erdos_renyi_graph(n, 100, seed=1)
    x = synth.gaussian_features(n, f, seed=1)
    y = np.zeros(n, np.int64)
    w = synth.gcn_weights(f, 257, 2, seed=1)
    with pytest.raises(_lib.LinkTellerHipError):
        _trainer(adj, x, y, [_dev(w[k]) for k in ("W1", "b1", "W2", "b2")])
    w = synth.gcn_weights(f, 16, 2, seed=1)
    bad = x.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError):
        _trainer(adj, bad, y, [_dev(w[k]) for k in ("W1", "b1", "W2", "b2")])
    with pytest.raises(ValueError):
        _trainer(adj, x, np.full(n, 2), [_dev(w[k]) for k in ("W1", "b1", "W2", "b2")])


def _main(cwd, args):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "linkteller_amd.main"] + args, cwd=cwd, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("mode", [["--mode", "vanilla-clean"], ["--mode", "vanilla", "--eps", "5"]])
def test_cli_train_then_attack(tmp_path, mode):
    from linkteller_amd import synth
    data = tmp_path / "data"
    synth.write_musae_dataset(str(data), "ES", synth.erdos_renyi_graph(200, 800, seed=21), 3170, 21)
    synth.write_musae_dataset(str(data), "RU", synth.erdos_renyi_graph(150, 600, seed=22), 3170, 22)
    common = ["--dataset", "twitch/ES/RU", "--norm", "FirstOrderGCN", "--attack", "--sample-type", "unbalanced",
              "--n-test", "40"] + mode
    out = _main(str(tmp_path), ["--train", "--num-epochs", "20"] + common)
    assert "Optimization Finished!" in out and "Total time elapsed" in out
    models = glob.glob(str(tmp_path / "model_twitch" / "ES" / "RU" / "*" / "model.pt"))
    logs = glob.glob(str(tmp_path / "logs_twitch" / "ES" / "RU" / "*.log"))
    results = glob.glob(str(tmp_path / "eval_twitch" / "ES" / "RU" / "*.pt"))
    assert len(models) == 1 and len(logs) == 1 and len(results) == 1
    log = open(logs[0]).read()
    assert "('Epoch: 0001', 'loss_train: " in log and "('Epoch: 0020', " in log
    sd = torch.load(models[0], map_location="cpu")
    assert sorted(sd) == ["gc1.bias", "gc1.weight", "gc2.bias", "gc2.weight"]
    assert sd["gc1.weight"].shape == (3170, 16) and sd["gc2.weight"].shape == (16, 2)
    first = torch.load(results[0], weights_only=False)["result"]["pred"]
    _main(str(tmp_path), ["--test", "--model-path", models[0]] + common)
    again = torch.load(results[0], weights_only=False)["result"]["pred"]
    assert np.array_equal(np.asarray(first), np.asarray(again))

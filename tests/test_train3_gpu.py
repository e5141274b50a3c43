"""Training of the 3-layer GCN on the GPU (engine.GCN3Trainer / lt_gcn3_trainer_*) against the reference's 40-epoch GCN3
trajectories (golden/train3.npz, on the graphs of golden/train.npz), at the extreme shapes, and end to end: train through
GCNTrainer, save model.pt, serve it to the attack from the command line."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu

LR, DECAY = 0.01, 5e-4
KEYS = ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias", "gc3.weight", "gc3.bias")


def _csr(g, norm, tag):
    n = g[f"{norm}.{tag}.indptr"].shape[0] - 1
    return sp.csr_matrix((g[f"{norm}.{tag}.data"], g[f"{norm}.{tag}.indices"], g[f"{norm}.{tag}.indptr"]), shape=(n, n))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _trainer(adj, x, y, params, dropout=0.0, seed=42):
    from linkteller_amd import engine
    return engine.GCN3Trainer(adj, _dev(x), _dev(y), *params, lr=LR, weight_decay=DECAY, dropout=dropout, seed=seed)


@pytest.mark.parametrize("norm", ["FirstOrderGCN", "AugRWalk"])
@pytest.mark.parametrize("h1,h2", [(16, 16), (64, 32)])
def test_trajectory_against_reference(norm, h1, h2):
    """The gates of test_train_gpu.test_trajectory_against_reference, unchanged."""
    from linkteller_amd.gcn import GCN3
    gold, g3 = load_golden("train.npz"), load_golden("train3.npz")
    key = f"{norm}.h{h1}_{h2}"
    adj1, adj2 = _csr(gold, norm, "adj1"), _csr(gold, norm, "adj2")
    params = [_dev(g3[f"{key}.init.{k}"].copy()) for k in KEYS]
    tr = _trainer(adj1, gold["x1"], gold["y1"], params)
    loss, correct = tr.run(int(g3["epochs"]))
    l64, l32 = g3[f"{key}.loss64"], g3[f"{key}.loss32"]
    print(f"  {key}: max|loss - loss64| {np.abs(loss - l64).max():.3e}, reference fp32 {np.abs(l32 - l64).max():.3e}")
    assert np.abs(loss - l64).max() <= 2 * np.abs(l32 - l64).max() + 1e-5, (np.abs(loss - l64).max(), np.abs(l32 - l64).max())
    assert np.all(np.abs(correct - g3[f"{key}.correct64"]) <= g3[f"{key}.tiny64"])
    model = GCN3(nfeat=gold["x1"].shape[1], nhid1=h1, nhid2=h2, nclass=2, dropout=0.0).cuda().eval()
    model.load_state_dict(dict(zip(KEYS, params)))
    from linkteller_amd import graph
    with torch.no_grad():
        z = model(_dev(gold["x2"]), graph.as_hip_graph(adj2)).cpu().numpy().astype(np.float64)
    z64, z32 = g3[f"{key}.logits2_64"], g3[f"{key}.logits2_32"]
    print(f"  {key}: max|z - z64| {np.abs(z - z64).max():.3e}, reference fp32 {np.abs(z32 - z64).max():.3e}")
    assert np.abs(z - z64).max() <= 2 * np.abs(z32 - z64).max() + 1e-5 * np.abs(z64).max(), \
        (np.abs(z - z64).max(), np.abs(z32 - z64).max())


@pytest.mark.parametrize("h1,h2,c", [(1, 1, 1), (5, 3, 2), (256, 256, 8), (33, 7, 5)])
def test_shapes_run(h1, h2, c):
    from linkteller_amd import graph, synth
    import train3_cases as K3
    n, f = 211, 37
    adj = graph.aug_random_walk(synth.powerlaw_graph(n, 1200, seed=2))
    x = synth.twitch_like_features(n, f, seed=3, density=0.05)
    y = (np.arange(n) * 7 % c).astype(np.int64)
    params = [_dev(p) for p in K3.init_params(f, h1, h2, c, seed=4)]
    tr = _trainer(adj, x, y, params, dropout=0.5)
    loss, correct = tr.run(5)
    assert np.all(np.isfinite(loss)) and np.all((correct >= 0) & (correct <= n))
    assert all(bool(torch.isfinite(p).all()) for p in params)
    assert all(bool(torch.isfinite(t).all()) for t in tr.grads())


@pytest.mark.parametrize("mode", [["--mode", "vanilla-clean"], ["--mode", "vanilla", "--eps", "5"]])
def test_train_three_layers_then_attack(tmp_path, monkeypatch, mode):
    """The documented way to train a GCN3: get_arguments -> Worker -> GCNTrainer.init_model(); train(); test() in process
    (the calls of main's _train), then the saved model.pt through `main --test --n-layer 3` in a subprocess: same pred."""
    import datetime
    import logging
    from linkteller_amd import main as lt_main, synth
    from linkteller_amd.trainer import GCNTrainer
    from linkteller_amd.worker import Worker
    data = tmp_path / "data"
    synth.write_musae_dataset(str(data), "ES", synth.erdos_renyi_graph(200, 800, seed=21), 3170, 21)
    synth.write_musae_dataset(str(data), "RU", synth.erdos_renyi_graph(150, 600, seed=22), 3170, 22)
    common = ["--dataset", "twitch/ES/RU", "--norm", "FirstOrderGCN", "--attack", "--sample-type", "unbalanced",
              "--n-test", "40", "--n-layer", "3", "--hidden1", "16", "--hidden2", "8"] + mode
    monkeypatch.chdir(tmp_path)
    args = lt_main.get_arguments(["--train", "--num-epochs", "20"] + common)
    import random
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    subdir = "gcn3_" + datetime.datetime.now().strftime("%m-%d-%H:%M:%S.%f")
    handler = lt_main.init_logger("./logs_{}".format(args.dataset), subdir)
    try:
        worker = Worker(args, dataset=args.dataset, mode=args.mode, data_root=args.data_root)
        trainer = GCNTrainer(args, subdir=subdir, worker=worker)
        trainer.init_model()
        trainer.train()
        trainer.test(args.eval_degree)
    finally:
        logging.getLogger().removeHandler(handler)
        handler.close()
    models = glob.glob(str(tmp_path / "model_twitch" / "ES" / "RU" / "*" / "model.pt"))
    logs = glob.glob(str(tmp_path / "logs_twitch" / "ES" / "RU" / "*.log"))
    results = glob.glob(str(tmp_path / "eval_twitch" / "ES" / "RU" / "*.pt"))
    assert len(models) == 1 and len(logs) == 1 and len(results) == 1
    log = open(logs[0]).read()
    assert log.count("('Epoch: ") == 20 and "('Epoch: 0001', 'loss_train: " in log and "('Epoch: 0020', " in log
    losses = [float(s.split("'")[0]) for s in log.split("loss_train: ")[1:]]
    assert len(losses) == 20 and np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    sd = torch.load(models[0], map_location="cpu")
    assert sorted(sd) == sorted(KEYS)
    assert [tuple(sd[k].shape) for k in KEYS] == [(3170, 16), (16,), (16, 8), (8,), (8, 2), (2,)]
    first = torch.load(results[0], weights_only=False)["result"]["pred"]
    os.remove(results[0])      # the subprocess must write the result file itself
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "linkteller_amd.main", "--test", "--model-path", models[0]] + common,
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert glob.glob(str(tmp_path / "eval_twitch" / "ES" / "RU" / "*.pt")) == results
    again = torch.load(results[0], weights_only=False)["result"]["pred"]
    assert np.array_equal(np.asarray(first), np.asarray(again))

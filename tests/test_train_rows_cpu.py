"""``--train-setting`` and the row-list training entry points without a GPU: the flag's default and choices, every refusal of
``check_train_setting`` before a Worker is built or anything is written, ``GCNTrainer.init_model`` choosing the graph and the
list from the setting (the engine class replaced by a recorder), the two new symbols in the header and the bindings, and the
masked restatement of test_train_rows_gpu.py against the restatements it is written on."""
import argparse
import os
import re
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import train_restate as T
import train_rows_restate as R
import train_wide_restate as TW
from linkteller_amd import _lib, engine, main as lt_main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_default_and_choices(capsys):
    args = lt_main.get_arguments(["--test"])
    assert args.train_setting == "inductive"
    assert lt_main.get_arguments(["--train", "--train-setting", "transductive"]).train_setting == "transductive"
    with pytest.raises(SystemExit):
        lt_main.get_arguments(["--train", "--train-setting", "semi"])
    assert "invalid choice: 'semi'" in capsys.readouterr().err
    lt_main.check_train_setting(args)                                                     # the default asks for nothing
    lt_main.check_train_setting(argparse.Namespace(train=False, test=True))               # a caller's Namespace without the flag
    with pytest.raises(ValueError, match="inductive or transductive"):
        lt_main.check_train_setting(argparse.Namespace(train=True, test=False, dataset="flickr", train_setting="semi"))
    ok = argparse.Namespace(train=True, test=False, train_setting="transductive")
    for name in ("flickr", "reddit", "ppi", "ppi-large"):
        ok.dataset = name
        lt_main.check_train_setting(ok)


@pytest.mark.parametrize("argv,match", [
    (["--test", "--dataset", "flickr"], "needs --train without --test"),
    (["--dataset", "flickr"], "needs --train without --test"),
    (["--train", "--test", "--dataset", "flickr"], "needs --train without --test"),
    (["--train", "--dataset", "twitch/ES/RU"], "a transfer dataset trains on every node of its first graph"),
    (["--train", "--dataset", "cora"], "needs a dataset with one graph and a split"),
    (["--train", "--dataset", "flickr", "--n-layer", "3"], "--train: training is implemented for the 2-layer GCN only"),
])
def test_refused_before_a_worker(argv, match, tmp_path, monkeypatch):
    from linkteller_amd import worker as W
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was loaded before the refusal"))
    monkeypatch.setattr(W, "Worker", lambda *a, **k: pytest.fail("a Worker was built before the refusal"))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match=match):
        lt_main.main(argv + ["--train-setting", "transductive", "--hidden", "8", "--norm", "FirstOrderGCN", "--data-root", str(tmp_path)])
    assert not os.listdir(tmp_path)


class _Recorder:
    """Stands in for engine.GCN2Trainer / GCN3Trainer: keeps the constructor's arguments."""
    calls = []

    def __init__(self, *args, **kwargs):
        type(self).calls.append((args, kwargs))


def _worker(n_full=9, n_train=4, f=5):
    idx = np.array([7, 1, 4, 2])[:n_train]
    labels = torch.arange(n_full).reshape(-1, 1) % 3
    return types.SimpleNamespace(mode="vanilla-clean", dataset="flickr", n_features=f, n_classes=3, multi_label=1, transfer=False,
                                 adj_train=sp.identity(n_train, format="csr"), adj_full=sp.identity(n_full, format="csr"),
                                 features_train=torch.zeros(n_train, f), features=torch.ones(n_full, f), labels=labels,
                                 idx_train=idx, idx_val=np.array([0, 3]))


@pytest.mark.parametrize("n_layer", [2, 3])
def test_init_model_follows_the_setting(n_layer, monkeypatch):
    from linkteller_amd.trainer import GCNTrainer
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(engine, "GCN2Trainer", _Recorder)
    monkeypatch.setattr(engine, "GCN3Trainer", _Recorder)
    base = dict(n_layer=n_layer, hidden=8, hidden1=8, hidden2=4, dropout=0.5, lr=0.01, weight_decay=5e-4, seed=1)
    w = _worker()
    seen = {}
    for tag, extra in (("absent", {}), ("inductive", {"train_setting": "inductive"}), ("transductive", {"train_setting": "transductive"})):
        _Recorder.calls = []
        tr = GCNTrainer(types.SimpleNamespace(**base, **extra), subdir="", worker=w)
        tr.init_model()
        assert len(_Recorder.calls) == 1 and isinstance(tr.gpu_trainer, _Recorder)
        seen[tag] = _Recorder.calls[0]
    for tag in ("absent", "inductive"):      # today's call: the induced subgraph, its features, the labels of idx_train, no list
        args, kwargs = seen[tag]
        assert args[0] is w.adj_train and args[1] is w.features_train and torch.equal(args[2], w.labels[torch.as_tensor(w.idx_train)])
        assert sorted(kwargs) == ["dropout", "lr", "seed", "weight_decay"]
        assert len(args) == 3 + 2 * n_layer
    args, kwargs = seen["transductive"]
    assert args[0] is w.adj_full and args[1] is w.features and args[2] is w.labels
    assert sorted(kwargs) == ["dropout", "lr", "seed", "train_rows", "weight_decay"] and kwargs["train_rows"] is w.idx_train
    assert len(args) == 3 + 2 * n_layer
    # a transfer dataset has nothing to list: refused here too, for callers that do not come through main
    w.transfer, w.adj_1, w.features_1, w.labels_1 = True, w.adj_full, w.features, w.labels
    tr = GCNTrainer(types.SimpleNamespace(**base, train_setting="transductive"), subdir="", worker=w)
    with pytest.raises(NotImplementedError, match="nothing to list"):
        tr.init_model()


def test_acc_train_is_over_the_listed_rows(monkeypatch, caplog):
    """The log's acc_train divides by n_train (times C for a multi-label trainer), not by the rows forwarded."""
    import logging
    from linkteller_amd.trainer import GCNTrainer
    tr = GCNTrainer(types.SimpleNamespace(), subdir="", worker=types.SimpleNamespace(mode="vanilla-clean", dataset="flickr"))
    r = dict(loss=np.array([0.5], np.float32), correct=np.array([30]), val_loss=np.array([0.25], np.float32),
             val_counts=np.array([[[2, 0], [1, 1]]]), best_epoch=0, stop_epoch=-1)
    for gpu, want in ((types.SimpleNamespace(n=100, n_train=40, c=2, head="narrow", loss="ce"), "0.7500"),
                      (types.SimpleNamespace(n=100, c=2, head="narrow", loss="ce"), "0.3000"),
                      (types.SimpleNamespace(n=100, n_train=40, c=3, head="narrow", loss="bce"), "0.2500")):
        tr.gpu_trainer = gpu
        with caplog.at_level(logging.INFO):
            caplog.clear()
            tr._log_validated(r, 0.0, 4, restore=False)
        assert f"acc_train: {want}" in caplog.text, caplog.text


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "linkteller_hip.h")).read()
    for layers in (2, 3):
        name = f"lt_gcn{layers}_trainer_set_train_rows"
        assert re.search(rf"int {name}\(lt_gcn{layers}_trainer \*t, const int32_t \*rows, int32_t m, void \*stream\);", header)
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and args == [_lib.C.c_void_p, _lib.C.c_void_p, _lib.C.c_int32, _lib.C.c_void_p]
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for cls in (engine.GCN2Trainer, engine.GCN3Trainer):
        assert cls.set_train_rows is engine._GCNTrainer.set_train_rows
        import inspect
        assert inspect.signature(cls.__init__).parameters["train_rows"].default is None


def test_engine_checks_the_list_on_the_host(monkeypatch):
    """set_train_rows' own checks, on an instance that has only what they read: nothing reaches the library."""
    tr = object.__new__(engine.GCN2Trainer)
    tr.n, tr.n_train = 10, 10
    tr._call = lambda *a: pytest.fail("the library was called with a bad list")
    for bad, exc, match in (([0, 10, -1, 3], IndexError, "2 ids outside the graph"), ([3, 1, 3, 3], ValueError, "2 ids repeat"),
                            (list(range(10)) + [4], ValueError, "1 ids repeat"), (np.array([0.0, 1.0]), ValueError, "integer ids"),
                            (torch.tensor([True, False]), ValueError, "integer ids"), (np.zeros((2, 2), np.int64), ValueError, "1-d"),
                            ([], ValueError, "empty"), (np.zeros(0, np.int64), ValueError, "empty")):
        with pytest.raises(exc, match=match):
            tr.set_train_rows(bad)
        assert tr.n_train == 10
    sent = []
    tr._call = lambda name, ptr, m, stream: sent.append((name, m))
    monkeypatch.setattr(engine, "_stream", lambda: None)
    tr.set_train_rows(np.array([9, 0, 4], dtype=np.uint8))
    assert sent == [("set_train_rows", 3)] and tr.n_train == 3
    tr.set_train_rows(None)
    assert sent[-1] == ("set_train_rows", 0) and tr.n_train == 10


def test_masked_restatement_against_its_parents():
    """epoch_reference_rows with the list 0 .. n - 1 is epoch_reference_wide (and, for ce, train_restate.epoch_reference); with
    a short list its loss is the mean over the listed rows, dZ2 is zero off the list and sums to db2; torch's fp64 autograd
    of ``F.cross_entropy(out[idx], y[idx])`` gives the same gradients."""
    import torch.nn.functional as F
    n, f, h, c = 40, 6, 8, 5
    from linkteller_amd import graph, synth
    adj = sp.csr_matrix(graph.first_order_gcn(synth.erdos_renyi_graph(n, 90, seed=1))).astype(np.float64)
    x = synth.gaussian_features(n, f, seed=2)
    w = synth.gcn_weights(f, h, c, seed=3)
    params = [w[k] for k in ("W1", "b1", "W2", "b2")]
    keep, scale = T.dropout_keep(n, h, 1, 77, 0.5), T.dropout_scale(0.5)
    y = np.random.RandomState(4).randint(0, c, n)
    yb = (np.random.RandomState(5).uniform(size=(n, c)) < 0.3).astype(np.uint8)
    for loss, lab in (("ce", y), ("bce", yb)):
        full = R.epoch_reference_rows(adj, x, lab, params, keep, scale, loss, np.arange(n))
        want = TW.epoch_reference_wide(adj, x, lab, params, keep, scale, loss)
        for k in R.NAMES + ("Z2", "dZ2", "counts"):
            assert np.array_equal(full[k], want[k]), (loss, k)
        assert full["loss"] == want["loss"]
    narrow = T.epoch_reference(adj, x, y, params, keep, scale)
    full = R.epoch_reference_rows(adj, x, y, params, keep, scale, "ce", np.arange(n))
    assert all(np.array_equal(full[k], narrow[k]) for k in R.NAMES) and full["correct"] == int((narrow["argmax"] == y).sum())
    rows = R.row_list(n, 7, seed=0)
    got = R.epoch_reference_rows(adj, x, y, params, keep, scale, "ce", rows)
    off = np.setdiff1d(np.arange(n), rows)
    assert not got["dZ2"][off].any() and np.allclose(got["dZ2"][rows].sum(axis=0), got["db2"], rtol=0, atol=1e-15)
    tp = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in params]
    a = torch.tensor(adj.toarray())
    hid = torch.relu(a @ (torch.tensor(x, dtype=torch.float64) @ tp[0]) + tp[1]) * torch.tensor(keep * float(scale), dtype=torch.float64)
    out = a @ (hid @ tp[2]) + tp[3]
    idx = torch.tensor(rows)
    val = F.cross_entropy(out[idx], torch.tensor(y)[idx])
    val.backward()
    assert abs(float(val.detach()) - got["loss"]) <= 1e-12
    for k, p in zip(R.NAMES, tp):
        assert np.abs(p.grad.numpy() - got[k]).max() <= 1e-12, k
    # the lists of the GPU test: distinct, unsorted, with both boundary rows
    for m in (2, 17, 255, 256, 257, 513):
        r = R.row_list(600, m, seed=m)
        assert len(np.unique(r)) == m and 0 in r and 599 in r and r.min() >= 0 and r.max() < 600
    assert R.row_list(600, 1, seed=0).tolist() == [0]

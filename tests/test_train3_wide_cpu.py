"""Without a GPU: the wide GCN3 restatement (train3_wide_restate.py) against torch's fp64 autograd for both losses, the
conditions of the GPU cases at epoch 0 and after two Adam steps simulated on the CPU, the constructor's argument checks,
``GCNTrainer.init_model`` with three layers and the wide head reaching the GPU trainer, and ``main``'s two refusals, which still
come before a Worker is built."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_restate as T
import train3_wide_cases as KT
import train3_wide_restate as TW3
from linkteller_amd import _lib
from linkteller_amd import main as lt_main


def _autograd(case, keep1, keep2, scale):
    """The epoch through torch fp64 autograd: (Z3, loss, the six gradients)."""
    a = case["adj"].astype(np.float64).tocoo()
    adj = torch.sparse_coo_tensor(np.vstack([a.row, a.col]), a.data, a.shape, dtype=torch.float64).coalesce()
    x = torch.from_numpy(case["x"].astype(np.float64))
    params = [torch.from_numpy(p.astype(np.float64)).requires_grad_(True) for p in case["params"]]
    w1, b1, w2, b2, w3, b3 = params
    d1, d2 = (torch.from_numpy(k.astype(np.float64) * np.float64(scale)) for k in (keep1, keep2))
    h1 = torch.relu(torch.sparse.mm(adj, x @ w1) + b1) * d1
    h2 = torch.relu(torch.sparse.mm(adj, h1 @ w2) + b2) * d2
    z3 = torch.sparse.mm(adj, h2 @ w3) + b3
    if case["loss"] == "ce":
        loss = F.cross_entropy(z3, torch.from_numpy(case["y"]))
    else:
        loss = F.binary_cross_entropy_with_logits(z3, torch.from_numpy(case["y"].astype(np.float64)))
    loss.backward()
    return z3.detach().numpy(), float(loss.detach()), [p.grad.numpy() for p in params]


@pytest.mark.parametrize("name", ["T9", "T65"])
def test_restatement_equals_autograd(name):
    torch.set_num_threads(1)
    case = KT.make(name)
    keep1, keep2 = KT.masks(case, 0)
    scale = T.dropout_scale(case["p"])
    z3, loss, grads = _autograd(case, keep1, keep2, scale)
    r = TW3.epoch_reference3_wide(case["adj"], case["x"], case["y"], case["params"], keep1, keep2, scale, case["loss"], np.float64)
    assert keep1.shape == (case["n"], case["H1"]) and keep2.shape == (case["n"], case["H2"]) and not np.array_equal(keep1[:, :12], keep2[:, :12])
    for k, want, got in [("Z3", z3, r["Z3"]), ("loss", np.float64(loss), np.float64(r["loss"]))]:
        assert float(np.abs(got - want).max()) <= 1e-12 * max(float(np.abs(want).max()), 1.0), (name, k)
    for k, want in zip(KT.NAMES, grads):
        err, ref = float(np.abs(r[k] - want).max()), float(np.abs(want).max())
        print(f"  {name} {k}: |restatement - autograd| {err:.3e} of {ref:.3e}")
        assert ref > 0 and err <= 1e-10 * ref, (name, k, err, ref)


@pytest.mark.parametrize("name", list(KT.SHAPES))
def test_case_conditions_at_epoch_0_and_after_two_steps(name):
    torch.set_num_threads(1)
    case = KT.make(name)
    n, f, h1, h2, c, loss, p = KT.SHAPES[name]
    assert case["x"].shape == (n, f) and [q.shape for q in case["params"]] == [(f, h1), (h1,), (h1, h2), (h2,), (h2, c), (c,)]
    if loss == "bce":
        assert case["y"].shape == (n, c) and not case["y"][0].any() and case["y"][1].all()
        assert np.abs(case["params"][5]).min() >= 1 and np.abs(case["params"][5]).max() <= 3
    KT.conditions_hold(case)
    if name == "T41":
        assert (case["adj"] != case["adj"].T).nnz > 0
    if name == "T121":
        assert np.diff(case["adj"].indptr).max() > 128 and np.diff(case["adj"].tocsc().indptr).max() > 128
    if name == "T65":
        assert c > h2 and c % 64 == 1
    if name == "T256":
        assert h2 % 4 and c == 256
    if name == "P1":
        r = KT.analyse(case, case["params"], 0)["r64"]
        assert all(not r[k].any() for k in KT.NAMES[:5]) and np.abs(r["db3"]).max() > 0
        assert np.array_equal(r["Z3"], np.broadcast_to(case["params"][5].astype(np.float64), r["Z3"].shape))


def test_the_seeds_are_the_first_that_meet_the_conditions():
    for name in ("T256", "T1"):      # (the other cases take seed 0; T256's search passes over it)
        assert KT.find_seed(name) == KT.SEEDS[name]
    assert all(KT.SEEDS[k] == 0 for k in KT.SHAPES if k != "T256")


def test_trainer_arguments_are_checked_without_a_gpu():
    import scipy.sparse as sp
    from linkteller_amd import engine
    z = torch.zeros
    shapes = (sp.identity(4, format="csr"), z(4, 3))
    params = (z(3, 2), z(2), z(2, 2), z(2), z(2, 5), z(5))
    kw = dict(lr=0.01, weight_decay=0.0, dropout=0.5, seed=0)
    for bad, match in ((dict(head="broad"), "head must be"), (dict(loss="mse"), "loss must be"),
                       (dict(head="narrow", loss="bce"), "narrow head has the cross-entropy loss only")):
        with pytest.raises(ValueError, match=match):
            engine.GCN3Trainer(*shapes, [0, 1, 0, 1], *params, **kw, **bad)
    # the label preparation both classes share (the constructor reaches it behind the graph, which needs the device): on an
    # instance that has only what it reads
    ok = np.zeros((4, 5), dtype=np.int64)
    for cls in (engine.GCN2Trainer, engine.GCN3Trainer):
        assert cls._prepare_labels is engine._GCNTrainer._prepare_labels and cls._set_head is engine._GCNTrainer._set_head
        tr = object.__new__(cls)
        tr.c, tr.x = 5, z(4, 3)
        tr._set_head("wide", "bce")
        for labels, match in (([0, 1, 0, 1], r"must be \[4, 5\]"), (np.zeros((4, 4), dtype=np.int64), r"must be \[4, 5\]"),
                              (ok.astype(np.float32), "integer or bool dtype"), (ok + 2, "0 / 1"), (ok - 1, "0 / 1")):
            with pytest.raises(ValueError, match=match):
                tr._prepare_labels(labels, 4, "labels")
        got = tr._prepare_labels(ok.astype(bool), 4, "labels")
        assert got.dtype == torch.uint8 and tuple(got.shape) == (4, 5)
        tr._set_head("wide", "ce")
        with pytest.raises(ValueError, match="outside"):
            tr._prepare_labels([0, 1, 0, 5], 4, "labels")
        assert tr._prepare_labels([0, 1, 0, 4], 4, "labels").dtype == torch.int32
    if not torch.cuda.is_available():      # well-formed arguments go on to the library
        with pytest.raises(_lib.LinkTellerHipError):
            engine.GCN3Trainer(*shapes, ok, *params, **kw, head="wide", loss="bce")


@pytest.mark.parametrize("multi_label,n_classes", [(1, 41), (121, 121)])
def test_init_model_three_layers_wide_reaches_the_trainer(multi_label, n_classes):
    """GCNTrainer.init_model() with n_layer = 3 and train_head = "wide" builds GCN3 and goes on to the GPU trainer's constructor
    (the method of test_train3_cpu.py): without a GPU that is LinkTellerHipError, not a NotImplementedError."""
    import scipy.sparse as sp
    from linkteller_amd.gcn import GCN3
    from linkteller_amd.trainer import GCNTrainer
    n, f = 6, 5
    labels = torch.zeros((n, n_classes), dtype=torch.int64) if multi_label > 1 else torch.zeros(n, dtype=torch.int64)
    worker = types.SimpleNamespace(mode="vanilla-clean", dataset="ppi" if multi_label > 1 else "reddit", n_features=f,
                                   n_classes=n_classes, multi_label=multi_label, transfer=False, adj_train=sp.identity(n, format="csr"),
                                   features_train=torch.zeros(n, f), labels=labels, idx_train=np.arange(n))
    args = types.SimpleNamespace(n_layer=3, hidden=16, hidden1=8, hidden2=4, dropout=0.5, lr=0.01, weight_decay=5e-4, seed=1,
                                 train_head="wide", fastmode=False)
    tr = GCNTrainer(args, subdir="", worker=worker)
    if torch.cuda.is_available():
        worker.features_train, worker.labels = worker.features_train.cuda(), worker.labels.cuda()
        tr.init_model()
        assert type(tr.gpu_trainer).__name__ == "GCN3Trainer" and tr.gpu_trainer.head == "wide"
        assert tr.gpu_trainer.loss == ("bce" if multi_label > 1 else "ce")
    else:
        with pytest.raises(_lib.LinkTellerHipError):
            tr.init_model()
    assert isinstance(tr.model, GCN3)
    assert [tuple(p.shape) for p in tr.model.parameters()] == [(f, 8), (8,), (8, 4), (4,), (4, n_classes), (n_classes,)]


def test_main_keeps_both_refusals_before_a_worker(tmp_path, monkeypatch):
    from linkteller_amd import worker as W
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was loaded before the refusal"))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(W, "Worker", lambda *a, **k: pytest.fail("a Worker was built before the refusal"))
    train = ["--train", "--hidden", "8", "--norm", "FirstOrderGCN", "--num-epochs", "2", "--data-root", str(tmp_path)]
    with pytest.raises(NotImplementedError, match="--train-head wide is implemented for the 2-layer GCN only"):
        lt_main.main(train + ["--dataset", "ppi", "--train-head", "wide", "--n-layer", "3"])
    with pytest.raises(NotImplementedError, match="--train: training is implemented for the 2-layer GCN only"):
        lt_main.main(train + ["--dataset", "twitch/ES/RU", "--n-layer", "3"])
    assert not os.listdir(tmp_path)

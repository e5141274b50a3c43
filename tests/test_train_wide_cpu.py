"""Without a GPU: the wide head's restatement (train_wide_restate.py) against torch's fp64 autograd for both losses,
``engine.f1_from_counts`` against sklearn, the conditions of the GPU cases at their initial parameters, and the refusals of
``--train-head``, which come before a Worker is built or the library is loaded."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_restate as T
import train_wide_cases as KW
import train_wide_restate as TW
from linkteller_amd import _lib
from linkteller_amd import main as lt_main


def _autograd(case, keep, scale):
    """The epoch through torch fp64 autograd: (Z2, loss, the four gradients)."""
    a = case["adj"].astype(np.float64).tocoo()
    adj = torch.sparse_coo_tensor(np.vstack([a.row, a.col]), a.data, a.shape, dtype=torch.float64).coalesce()
    x = torch.from_numpy(case["x"].astype(np.float64))
    params = [torch.from_numpy(p.astype(np.float64)).requires_grad_(True) for p in case["params"]]
    w1, b1, w2, b2 = params
    drop = torch.from_numpy(keep.astype(np.float64) * np.float64(scale))
    h = torch.relu(torch.sparse.mm(adj, x @ w1) + b1) * drop
    z2 = torch.sparse.mm(adj, h @ w2) + b2
    if case["loss"] == "ce":
        loss = F.cross_entropy(z2, torch.from_numpy(case["y"]))
    else:
        loss = F.binary_cross_entropy_with_logits(z2, torch.from_numpy(case["y"].astype(np.float64)))
    loss.backward()
    return z2.detach().numpy(), float(loss.detach()), [p.grad.numpy() for p in params]


@pytest.mark.parametrize("name", ["W9", "W41", "W65", "W256bce", "W1"])
def test_restatement_equals_autograd(name):
    torch.set_num_threads(1)
    case = KW.make(name)
    keep = T.dropout_keep(case["n"], case["H"], 0, KW.SEED, case["p"])
    scale = T.dropout_scale(case["p"])
    z2, loss, grads = _autograd(case, keep, scale)
    r = TW.epoch_reference_wide(case["adj"], case["x"], case["y"], case["params"], keep, scale, case["loss"], np.float64)
    for k, want, got in [("Z2", z2, r["Z2"]), ("loss", np.float64(loss), np.float64(r["loss"]))] + \
            [(k, g, r[k]) for k, g in zip(KW.NAMES, grads)]:
        err, ref = float(np.abs(got - want).max()), float(np.abs(want).max())
        print(f"  {name} {k}: |restatement - autograd| {err:.3e} of {ref:.3e}")
        assert err <= 1e-12 * max(ref, 1.0), (name, k, err, ref)


def test_bce_restatement_is_stable_at_large_logits():
    """|z| up to 200: the loss is finite, sigma - y is exactly 0 or +-1 / (m C) where fp64 rounds it so, nothing is NaN."""
    z = np.array([[200.0, -200.0, 95.0, -95.0, 0.0, 1e-30]])
    y = np.array([[1, 0, 0, 1, 1, 0]])
    for dtype in (np.float64, np.float32):
        loss, dz, counts = TW.head_reference(z, y, "bce", dtype)
        assert np.isfinite(loss) and np.isfinite(dz).all()
        assert dz[0, 0] == 0 and abs(dz[0, 1]) < 1e-40 and dz[0, 2] == dtype(1) / dtype(6) and dz[0, 3] == -dtype(1) / dtype(6)
        assert counts.tolist() == [[1, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1], [0, 1, 0]]


def test_f1_from_counts_equals_sklearn():
    from sklearn.metrics import f1_score
    from linkteller_amd import engine
    rng = np.random.RandomState(0)
    # multiclass, 7 classes: class 5 has no support, class 6 is never predicted
    y = rng.randint(0, 5, 400)
    y[:20] = 6
    pred = rng.randint(0, 6, 400)
    _, _, counts = TW.head_reference(np.eye(7)[pred] * 5.0, y, "ce")
    got = engine.f1_from_counts(counts)
    want = tuple(f1_score(y, pred, average=k, labels=list(range(7)), zero_division=0) for k in ("micro", "macro", "weighted"))
    assert all(isinstance(v, float) for v in got)
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12, (got, want)
    assert np.abs(np.array(got) - np.array(TW.f1_reference(counts))).max() <= 1e-12
    assert counts[5, 0] + counts[5, 2] == 0 and counts[6, 0] + counts[6, 1] == 0
    # multilabel, 9 labels: label 3 has no support, label 4 is never predicted, label 8 neither
    yb = (rng.uniform(size=(300, 9)) < 0.4).astype(int)
    zb = rng.standard_normal((300, 9))
    yb[:, 3] = 0
    zb[:, 4] = -1.0
    yb[:, 8] = 0
    zb[:, 8] = -1.0
    _, _, counts = TW.head_reference(zb, yb, "bce")
    got = engine.f1_from_counts(torch.from_numpy(counts))
    want = tuple(f1_score(yb, (zb > 0).astype(int), average=k, zero_division=0) for k in ("micro", "macro", "weighted"))
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12, (got, want)
    assert engine.f1_from_counts(np.zeros((4, 3), int)) == (0.0, 0.0, 0.0)
    # present_only: sklearn on single-label inputs WITHOUT the class list leaves out classes 7, 8 and 9 of 10, which are neither a
    # label nor a prediction; class 5 (no support) and class 6 (never predicted) stay in
    _, _, counts = TW.head_reference(np.eye(10)[pred] * 5.0, y, "ce")
    assert not counts[7:].any()
    got = engine.f1_from_counts(counts, present_only=True)
    want = tuple(f1_score(y, pred, average=k, zero_division=0) for k in ("micro", "macro", "weighted"))
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12, (got, want)
    assert abs(engine.f1_from_counts(counts)[1] - got[1] * 7 / 10) <= 1e-12      # the default averages over all 10
    for bad in (np.zeros((3, 3, 3)), np.zeros((4, 4)), np.zeros(3)):
        with pytest.raises(ValueError):
            engine.f1_from_counts(bad)


@pytest.mark.parametrize("name", list(KW.SHAPES))
def test_case_conditions_at_the_initial_parameters(name):
    torch.set_num_threads(1)
    case = KW.make(name)
    n, f, h, c, loss, p = KW.SHAPES[name]
    assert case["x"].shape == (n, f) and case["params"][2].shape == (h, c) and case["loss"] == loss and case["p"] == p
    if loss == "bce":
        assert case["y"].shape == (n, c) and not case["y"][0].any() and case["y"][1].all()
    KW.check_conditions(case, KW.analyse(case, case["params"], 0))


def _no_gpu(monkeypatch):
    """Any use of the library or of a CUDA tensor fails the test: the refusals come first."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was loaded before the refusal"))


_TRAIN = ["--train", "--hidden", "8", "--norm", "FirstOrderGCN", "--num-epochs", "2"]


def test_train_head_refusals_come_before_the_library(tmp_path, monkeypatch):
    from linkteller_amd import worker as W
    _no_gpu(monkeypatch)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(W, "Worker", lambda *a, **k: pytest.fail("a Worker was built before the refusal"))
    root = ["--data-root", str(tmp_path)]
    with pytest.raises(NotImplementedError, match="--train-head wide is implemented for the 2-layer GCN only"):
        lt_main.main(_TRAIN + ["--dataset", "ppi", "--train-head", "wide", "--n-layer", "3"] + root)
    with pytest.raises(NotImplementedError, match="--train-head wide needs --train"):
        lt_main.main(["--test", "--dataset", "ppi", "--train-head", "wide"] + root)
    with pytest.raises(NotImplementedError, match="--fastmode"):
        lt_main.main(_TRAIN + ["--dataset", "reddit", "--train-head", "wide", "--fastmode"] + root)
    with pytest.raises(ValueError, match="--patience"):
        lt_main.main(_TRAIN + ["--dataset", "ppi-large", "--train-head", "wide", "--early", "--patience", "0"] + root)
    with pytest.raises(SystemExit):
        lt_main.get_arguments(["--train-head", "broad"])
    # the flag absent, or narrow: the old messages
    for extra in ([], ["--train-head", "narrow"]):
        for name in ("ppi", "ppi-large", "reddit"):
            with pytest.raises(NotImplementedError, match="single label and at most 8"):
                lt_main.main(_TRAIN + ["--dataset", name] + extra + root)
    assert not os.listdir(tmp_path)
    assert lt_main.get_arguments([]).train_head == "narrow"
    for name in ("ppi", "ppi-large", "reddit"):      # wide lets them through the flag checks
        args = lt_main.get_arguments(_TRAIN + ["--dataset", name, "--train-head", "wide"])
        lt_main.check_train_head(args)
        lt_main.check_split_dataset(args)


def test_trainer_arguments_are_checked_without_a_gpu():
    import scipy.sparse as sp
    from linkteller_amd import engine
    z = torch.zeros
    args = (sp.identity(4, format="csr"), z(4, 3), [0, 1, 0, 1], z(3, 2), z(2), z(2, 2), z(2))
    for kw in (dict(head="broad"), dict(loss="mse"), dict(head="narrow", loss="bce")):
        with pytest.raises(ValueError):
            engine.GCN2Trainer(*args, lr=0.01, weight_decay=0.0, dropout=0.5, seed=0, **kw)

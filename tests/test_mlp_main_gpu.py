"""``main_simple --mode mlp`` end to end on synthetic fixtures written to a temporary data root: a twitch transfer pair
(3170 one-hot features) and 300-node GraphSAINT datasets (``ppi``: 121 labels per node; ``reddit``: 41 classes).  Train three
epochs with ``--batch``, find ``model.pt``, run ``--test --model-path`` in a fresh child process and compare its test line, check
the printed F1 values against sklearn on the saved model's predictions, and load the file into plain ``nn.Linear`` stacks."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NF = 300, 24
SHAPES = {"ppi": 121, "reddit": 41}


def _graphsaint(root, name):
    from linkteller_amd import synth
    c = SHAPES[name]
    rng = np.random.RandomState(31 + c)
    adj = synth.erdos_renyi_graph(N, 900, seed=32).astype(np.float64)
    if name == "ppi":
        proto = rng.randint(0, 6, N)
        y = (rng.uniform(size=(6, c)) < 0.3)[proto].astype(np.int64)
        y = np.where(rng.uniform(size=y.shape) < 0.05, 1 - y, y)
    else:
        proto = y = rng.randint(0, c, N)
    feats = rng.standard_normal((c, NF))[proto] * 1.5 + rng.standard_normal((N, NF))
    perm = rng.permutation(N)
    synth.write_graphsaint_dataset(str(root), name, adj, feats, y, {"tr": perm[:150].tolist(), "va": perm[150:225].tolist(),
                                                                   "te": perm[225:].tolist()})


def _twitch(root):
    from linkteller_amd import synth
    synth.write_musae_dataset(str(root), "ES", synth.erdos_renyi_graph(200, 800, seed=21), 3170, 21)
    synth.write_musae_dataset(str(root), "RU", synth.erdos_renyi_graph(150, 600, seed=22), 3170, 22)


def _plain_logits(sd, x, depth):
    """The saved file in plain nn.Linear stacks with the reference's key names (fp64)."""
    names = ("W1", "W2") if depth == 2 else ("W",)
    layers = []
    for nm in names:
        w = sd[f"{nm}.weight"]
        lin = torch.nn.Linear(w.shape[1], w.shape[0]).double()
        lin.load_state_dict({"weight": w.double(), "bias": sd[f"{nm}.bias"].double()})
        layers.append(lin)
    with torch.no_grad():
        h = x.double()
        for k, lin in enumerate(layers):
            h = lin(h)
            if k + 1 < len(layers):
                h = torch.relu(h)
    return h


# (twitch with 20 epochs: after 3 the model still predicts the majority class on nearly every test row, and the rare-class
# figures are then all zero; after 20 it predicts the rare class on some rows and the figures are worth comparing)
@pytest.mark.parametrize("dataset,depth,epochs", [("twitch/ES/RU", 2, 3), ("twitch/ES/RU", 2, 20), ("ppi", 2, 3), ("reddit", 2, 3),
                                                  ("reddit", 1, 3)])
def test_main_simple_end_to_end(dataset, depth, epochs, tmp_path, monkeypatch, capsys):
    from sklearn.metrics import f1_score
    from linkteller_amd import main_simple
    data = tmp_path / "data"
    _twitch(data) if dataset.startswith("twitch") else _graphsaint(data, dataset)
    run0 = tmp_path / "run0"
    run0.mkdir()
    monkeypatch.chdir(run0)
    argv = f"--mode mlp --depth {depth} --hidden 16 --batch --batch-size 64 --num-epochs {epochs} --lr 0.01 --dataset {dataset} " \
           f"--data-root {data}".split()
    tr = main_simple.main(argv)
    out = capsys.readouterr().out
    models = glob.glob(str(run0 / f"model_{dataset}" / "*" / "model.pt"))
    logs = glob.glob(str(run0 / f"logs_{dataset}" / "*.log"))
    assert len(models) == 1 and len(logs) == 1
    assert os.path.basename(os.path.dirname(models[0])).startswith("mode-mlp_hidden-16_lr-0.01_decay-5e-06_dropout-0.5_bs-64_")
    log = open(logs[0]).read()
    assert all(f"[epoch {e}]" in log for e in range(epochs)) and f"[epoch {epochs}]" not in log
    assert "Total time elapsed: " in out
    w = tr.worker
    n_train = w.n_nodes_1 if w.transfer else len(w.idx_train)
    assert tr.gpu_trainer.epoch == epochs and tr.gpu_trainer.step == epochs * -(-n_train // 64)
    loss, _ = tr.record
    assert np.isfinite(loss).all() and loss[-3:].mean() < loss[:3].mean()      # it trained

    sd = torch.load(models[0], map_location="cpu")
    assert sorted(sd) == (["W.bias", "W.weight", "W1.bias", "W1.weight", "W2.bias", "W2.weight"] if depth == 2
                          else ["W.bias", "W.weight"])
    assert all(torch.isfinite(t).all() for t in sd.values())
    test_lines = [ln for ln in out.splitlines() if ln.startswith("Test set results: ")]
    assert len(test_lines) == 1

    # the saved file in plain nn.Linear stacks: the library's test logits, and the printed F1 values from sklearn
    if w.transfer:
        x, truth = w.features_2.cpu(), w.labels_2.cpu()
    else:
        idx = torch.as_tensor(w.idx_test)
        x, truth = w.features.cpu()[idx], w.labels.cpu()[idx]
    z = _plain_logits(sd, x, depth)
    got = tr.test_output.cpu().double()
    assert got.shape == z.shape and float((got - z).abs().max()) <= 2e-5 * float(z.abs().max()) + 1e-6
    if w.transfer:
        # F1 / precision / recall of the minority class of labels_2 and the reference's AP (the predicted class's confidence
        # against "is the rare class"), all from sklearn on the saved file's fp64 logits
        from sklearn.metrics import average_precision_score, precision_score, recall_score
        y = truth.numpy()
        rare = int((y == 0).sum() > (y == 1).sum())
        assert 0 < (y == rare).sum() < (y != rare).sum()
        pred = z.argmax(1).numpy()
        # the library's fp32 logits are within tol of z (asserted above): a margin above 2 tol leaves no prediction to rounding
        tol = 2e-5 * float(z.abs().max()) + 1e-6
        assert (z[:, 0] - z[:, 1]).abs().min().item() > 2 * tol
        want = (f1_score(y, pred, pos_label=rare), precision_score(y, pred, pos_label=rare),
                recall_score(y, pred, pos_label=rare),
                # AP ranks the float32 confidences the reference's definition forms (softmax of the float32 logits): several
                # saturate to the same float32 value, and sklearn treats ties as one threshold, so the fp64 confidences give
                # another figure (0.3657 against 0.3676 after 20 epochs).  The logits themselves are compared with z above.
                average_precision_score(y if rare == 1 else 1 - y, torch.softmax(tr.test_output.cpu(), dim=1).max(1)[0].numpy()))
        f1 = tr.test_results["f1_test"]      # (sklearn gives 0 where nothing is predicted rare, as the trainer prints)
        assert len(f1) == 4 and all(abs(a - b) <= 1e-12 for a, b in zip(f1, want)), (f1, want)
        if epochs == 20:
            assert (pred == rare).any() and 0 < want[0] < 1 and 0 < want[1] < 1 and 0 < want[2] < 1
        assert test_lines[0].endswith(f"rare_class_f1 = {want[0]:.4f} prec = {want[1]:.4f} reca = {want[2]:.4f} "
                                      f"ap_score = {want[3]:.4f}")
    else:
        multi = w.multi_label > 1
        pred = (got > 0) if multi else got.argmax(1)
        want = [f1_score(truth if multi else truth.squeeze(1), pred, average=k) for k in ("micro", "macro", "weighted")]
        f1 = tr.test_results["f1_test"]
        assert all(abs(a - b) <= 1e-12 for a, b in zip(f1, want)), (f1, want)
        assert test_lines[0].endswith(f"f1_score [micro, macro, weighted] = {f1[0]:.4f} {f1[1]:.4f} {f1[2]:.4f}")
        assert sum(ln.startswith("Valid set results: ") for ln in out.splitlines()) == 1

    # --test --model-path in a fresh child process prints the same test line
    run1 = tmp_path / "run1"
    run1.mkdir()
    child = subprocess.run([sys.executable, os.path.join(REPO, "main_simple.py"), "--mode", "mlp", "--depth", str(depth), "--hidden",
                            "16", "--dataset", dataset, "--data-root", str(data), "--test", "--model-path", models[0]],
                           cwd=run1, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    assert test_lines[0] in child.stdout.splitlines(), child.stdout[-2000:]
    assert os.listdir(run1) == []


def test_training_in_chunks_of_epochs_changes_nothing(tmp_path, monkeypatch, capsys):
    """``MLPTrainer.train`` holds the orders of a bounded number of epochs at a time: with one epoch per chunk (``--batch`` on
    reddit, and the full-batch branch on twitch) the saved parameters and the per-step record equal the one-chunk run's bits."""
    from linkteller_amd import main_simple, mlp_trainer
    data = tmp_path / "data"
    _graphsaint(data, "reddit")
    _twitch(data)
    for dataset, extra in (("reddit", "--batch --batch-size 64"), ("twitch/ES/RU", "")):
        runs = []
        for k, entries in enumerate((mlp_trainer.MLPTrainer.ORDER_ENTRIES, 1)):
            monkeypatch.setattr(mlp_trainer.MLPTrainer, "ORDER_ENTRIES", entries)
            cwd = tmp_path / f"{dataset.split('/')[0]}{k}"
            cwd.mkdir()
            monkeypatch.chdir(cwd)
            tr = main_simple.main(f"--mode mlp --depth 2 --hidden 16 {extra} --num-epochs 4 --lr 0.01 --dataset {dataset} "
                                  f"--data-root {data}".split())
            sd = torch.load(glob.glob(str(cwd / f"model_{dataset}" / "*" / "model.pt"))[0], map_location="cpu")
            log = open(glob.glob(str(cwd / f"logs_{dataset}" / "*.log"))[0]).read()
            assert [f"[epoch {e}]" in log for e in range(5)] == [True] * 4 + [False]
            runs.append((tr.record, sd))
        (r0, sd0), (r1, sd1) = runs
        assert len(r0[0]) == (12 if extra else 4) and np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1])
        assert all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    capsys.readouterr()

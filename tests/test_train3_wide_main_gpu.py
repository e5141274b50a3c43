"""The 3-layer GCN3 trained with the wide head through the in-process sequence README documents (``get_arguments`` -> ``Worker``
-> ``GCNTrainer``; ``main --train --n-layer 3`` stays refused) on the synthetic GraphSAINT fixtures of
test_train_wide_main_gpu.py: a 300-node ``ppi`` with 121 labels per node (binary cross-entropy with logits) and a 300-node
``reddit`` with 41 classes (cross-entropy), with ``--early``.  The printed losses against torch fp64 on the saved parameters,
the F1 values against sklearn on the saved model's predictions; then ``main --test --n-layer 3 --model-path`` in a fresh process
prints the same test line and its attack gives the fp64 oracle's AUC / AP."""
import glob
import logging
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_train_wide_main_gpu as M2

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF, SHAPES, SAMPLE_SEED = M2.NF, M2.SHAPES, M2.SAMPLE_SEED
H1, H2 = 16, 12
MODEL = f"--n-layer 3 --hidden1 {H1} --hidden2 {H2} --norm FirstOrderGCN"
ATTACK = "--attack --attack-mode efficient --sample-type unbalanced --n-test 20"


def _train_in_process(cwd, data, name, monkeypatch):
    """README's sequence with ``--train-head wide``, the seeds and the log file as ``main`` sets them; returns the GCNTrainer."""
    from linkteller_amd import main as lt_main
    from linkteller_amd.trainer import GCNTrainer
    from linkteller_amd.worker import Worker
    cwd.mkdir(exist_ok=True)
    monkeypatch.chdir(cwd)
    args = lt_main.get_arguments(f"--train --train-head wide {MODEL} --early --patience 10 --num-epochs 40 --dataset {name} "
                                 f"--data-root {data}".split())
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    handler = lt_main.init_logger(f"./logs_{name}", "gcn3_wide")
    try:
        worker = Worker(args, dataset=args.dataset, mode=args.mode, data_root=args.data_root)
        trainer = GCNTrainer(args, subdir="gcn3_wide", worker=worker)
        trainer.init_model()
        trainer.train()
        trainer.test()
    finally:
        logging.getLogger().removeHandler(handler)
        handler.close()
    return trainer


def _torch_logits(sd, x, adj, dtype):
    a = adj.to_dense().to(dtype)
    h = x.to(dtype)
    for k in (1, 2):
        h = torch.relu(a @ (h @ sd[f"gc{k}.weight"].to(dtype)) + sd[f"gc{k}.bias"].to(dtype))
    return a @ (h @ sd["gc3.weight"].to(dtype)) + sd["gc3.bias"].to(dtype)


@pytest.mark.parametrize("name", ["ppi", "reddit"])
def test_gcn3_wide_end_to_end(name, tmp_path, monkeypatch, capsys):
    from sklearn.metrics import f1_score
    import sklearn.metrics as skm
    from oracle import linkteller_oracle as O
    c, multi = SHAPES[name], name == "ppi"
    data = tmp_path / "data"
    M2._dataset(data, name)
    run0 = tmp_path / "run0"
    tr = _train_in_process(run0, data, name, monkeypatch)
    out = capsys.readouterr().out
    model = run0 / f"model_{name}" / "gcn3_wide" / "model.pt"
    sd = torch.load(model, map_location="cpu")
    assert sorted(sd) == ["gc1.bias", "gc1.weight", "gc2.bias", "gc2.weight", "gc3.bias", "gc3.weight"]
    assert sd["gc1.weight"].shape == (NF, H1) and sd["gc2.weight"].shape == (H1, H2) and sd["gc3.weight"].shape == (H2, c)
    w = tr.worker
    assert w.n_classes == c and w.multi_label == (c if multi else 1)
    assert type(tr.gpu_trainer).__name__ == "GCN3Trainer"
    assert tr.gpu_trainer.head == "wide" and tr.gpu_trainer.loss == ("bce" if multi else "ce")

    # it trained: every epoch's line carries loss_val / acc_val, and the training loss fell
    log = open(glob.glob(str(run0 / f"logs_{name}" / "*.log"))[0]).read()
    lines = re.findall(r"'loss_train: ([0-9.]+)', 'acc_train: [0-9.]+', 'loss_val: ([0-9.]+)', 'acc_val: ([01]\.[0-9]{4})'", log)
    state = tr.gpu_trainer.val_state()
    ran = state["stop_epoch"] + 1 if state["stop_epoch"] >= 0 else 40
    assert len(lines) == ran and float(lines[-1][0]) < float(lines[0][0])

    # the printed losses against torch fp64 on the saved parameters: within 1e-5 relative
    x, adj, y = w.features.cpu(), w.adj_full.cpu(), w.labels.cpu()
    z64 = _torch_logits(sd, x, adj, torch.float64)
    res = tr.split_results
    for label, idx, got in (("Validation", w.idx_val, res["loss_valid"]), ("Test", w.idx_test, res["loss_test"])):
        idx = torch.as_tensor(idx)
        want = float(F.binary_cross_entropy_with_logits(z64[idx], y[idx].double()) if multi
                     else F.cross_entropy(z64[idx], y[idx].squeeze(1)))
        print(f"{name} {label}: library {got:.9g}, torch fp64 {want:.9g}")
        assert abs(got - want) <= 1e-5 * abs(want)
        assert f"[clean] {label} set results: loss = {got:.4f} " in out

    # the three F1 values against sklearn on the saved model's predictions
    with torch.no_grad():
        logits = tr.forward(mode="test").cpu()
    pred = (torch.sigmoid(logits) > 0.5) if multi else logits.argmax(1)
    truth = y if multi else y.squeeze(1)
    for idx, got in ((w.idx_val, res["f1_valid"]), (w.idx_test, res["f1_test"])):
        want = [f1_score(truth[idx], pred[idx], average=k) for k in ("micro", "macro", "weighted")]
        assert all(abs(g - s) <= 1e-12 for g, s in zip(got, want)), (got, want)
    f1 = res["f1_test"]
    test_line = (f"[clean] Test set results: loss = {res['loss_test']:.4f} f1_score [micro, macro, weighted] = "
                 f"{f1[0]:.4f} {f1[1]:.4f} {f1[2]:.4f}")
    assert test_line in out

    # main --test --n-layer 3 --model-path in a fresh process: the same test line, and the attack against the fp64 oracle
    run1 = tmp_path / "run1"
    run1.mkdir()
    done = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--test", *MODEL.split(), "--model-path", str(model),
                           "--dataset", name, "--data-root", str(data), *ATTACK.split()], cwd=run1, capture_output=True, text=True,
                          timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
    assert test_line in done.stdout
    saved_name = f"eval_{name}/efficient_unbalanced_20_{SAMPLE_SEED}.pt"
    assert f"attack results saved to: {saved_name}" in done.stdout
    saved = torch.load(run1 / saved_name, weights_only=False)
    np.random.seed(SAMPLE_SEED)
    (ex, nex), nodes = O.sample_subgraph_pairs(name, "unbalanced", w.adj_ori, 20)
    assert len(ex) > 0 and len(nex) > 0
    P = {k: sd[n].double() for k, n in zip(("W1", "b1", "W2", "b2", "W3", "b3"),
                                           ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias", "gc3.weight", "gc3.bias"))}
    infl = O.influence_matrix(x.double(), adj.double(), P, nodes, 1e-4, forward=O.gcn3_forward)
    m = O.attack_metrics(*O.pair_scores(infl, nodes, ex, nex))
    assert saved["result"]["y"] == m["y"]
    auc = skm.auc(saved["auc"]["fpr"], saved["auc"]["tpr"])
    ap = skm.average_precision_score(saved["result"]["y"], saved["result"]["pred"])
    print(f"{name}: auc {auc:.6f} (oracle {m['auc']:.6f}), ap {ap:.6f} (oracle {m['ap']:.6f}), {len(ex)} edges / {len(nex)} non-edges")
    assert abs(auc - m["auc"]) <= 1e-4 and abs(ap - m["ap"]) <= 1e-4

"""Datasets with one graph and a split of its nodes (flickr) on the GPU: both trainers validated over a row list
(lt_gcn*_trainer_attach_validation_rows) against the same trainer validated over every row, ``main --dataset flickr --train
--early`` end to end against stock torch, sklearn and the fp64 oracle, and the two DP builds of ``Worker``."""
import argparse
import glob
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import validate_restate as V

pytestmark = pytest.mark.gpu

N_TRAIN, N_FULL, NF, NC, M_ROWS, EPOCHS, PATIENCE = 150, 600, 20, 7, 257, 12, 3
LR = 0.3          # large on purpose: the validation loss goes up and down within the 12 epochs (asserted below)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(tr):
    return [p.cpu().numpy().copy() for p in tr.params]


class _Problem:
    def __init__(self):
        from linkteller_amd import graph, synth
        rng = np.random.RandomState(5)
        self.adj_train = graph.first_order_gcn(synth.erdos_renyi_graph(N_TRAIN, 450, seed=1))
        self.adj_full = graph.first_order_gcn(synth.erdos_renyi_graph(N_FULL, 1800, seed=2))
        self.y_train, self.y_full = rng.randint(0, NC, N_TRAIN), rng.randint(0, NC, N_FULL)
        centres = rng.standard_normal((NC, NF)).astype(np.float32)
        self.x_train = (centres[self.y_train] + rng.standard_normal((N_TRAIN, NF))).astype(np.float32)
        self.x_full = (centres[self.y_full] + rng.standard_normal((N_FULL, NF))).astype(np.float32)
        self.rows = rng.permutation(N_FULL)[:M_ROWS].astype(np.int64)          # shuffled, two blocks of the head

    def trainer(self, layers):
        from linkteller_amd import engine, synth
        if layers == 2:
            w = synth.gcn_weights(NF, 16, NC, seed=4)
            params = [_dev(w[k].copy()) for k in ("W1", "b1", "W2", "b2")]
            cls = engine.GCN2Trainer
        else:
            w, w3 = synth.gcn_weights(NF, 16, 8, seed=4), synth.gcn_weights(8, NC, NC, seed=8)
            params = [_dev(w[k].copy()) for k in ("W1", "b1", "W2", "b2")] + [_dev(w3["W1"].copy()), _dev(w3["b1"].copy())]
            cls = engine.GCN3Trainer
        return cls(self.adj_train, _dev(self.x_train), _dev(self.y_train), *params, lr=LR, weight_decay=5e-4, dropout=0.5, seed=9)


@pytest.fixture(scope="module")
def problem():
    return _Problem()


@pytest.mark.parametrize("layers", [2, 3])
def test_trainer_validated_over_a_row_list(problem, layers):
    from linkteller_amd import engine
    p = problem
    x_full, y_full, rows_dev = _dev(p.x_full), _dev(p.y_full), _dev(p.rows)
    a = p.trainer(layers)
    a.attach_validation(p.adj_full, x_full, y_full, keep_best=True, patience=PATIENCE, rows=p.rows)
    b = p.trainer(layers)
    b.attach_validation(p.adj_full, x_full, y_full, keep_best=False, patience=0)
    losses, record, models = [], [], []
    for e in range(EPOCHS):
        rb = b.run_validated(1)
        models.append(_bits(b))
        want_loss, want_conf = engine.eval_head(b.val_logits()[rows_dev].contiguous(), y_full[rows_dev])
        # B itself is today's trainer: its own record is the existing head over every row of its logits
        all_loss, all_conf = engine.eval_head(b.val_logits(), y_full)
        assert rb["val_loss"].view(np.int32)[0] == int(all_loss.view(torch.int32).cpu())
        assert np.array_equal(rb["val_counts"][0], all_conf.cpu().numpy())
        ra = a.run_validated(1)
        if len(ra["val_loss"]) == 0:                       # A stopped at an earlier epoch: nothing runs any more
            assert V.decide(np.asarray(losses, dtype=np.float32), PATIENCE)[1] >= 0
            break
        assert ra["val_loss"].view(np.int32)[0] == int(want_loss.view(torch.int32).cpu()), (e, ra["val_loss"], float(want_loss))
        assert np.array_equal(ra["val_counts"][0], want_conf.cpu().numpy()) and ra["val_counts"][0].sum() == M_ROWS
        assert torch.equal(a.val_logits(), b.val_logits())
        losses.append(ra["val_loss"][0])
        record.append((ra["loss"][0], ra["correct"][0]))
        best, stop = V.decide(np.asarray(losses, dtype=np.float32), PATIENCE)        # EarlyStopping on the host over those losses
        state = a.val_state()
        assert (state["best_epoch"], state["stop_epoch"]) == (best, stop) == (ra["best_epoch"], ra["stop_epoch"]), (e, state)
    losses = np.asarray(losses, dtype=np.float32)
    print(f"layers={layers}: validation losses over the list {losses.tolist()}, decision {V.decide(losses, PATIENCE)}")
    assert np.any(np.diff(losses) > 0) and np.any(np.diff(losses) < 0)          # a condition on the fixture: not monotone
    best, stop = V.decide(losses, PATIENCE)
    a.restore_best()
    for got, want in zip(_bits(a), models[best]):
        assert np.array_equal(got, want)
    # the train record of A is plain run's, and so is B's (validation attached without rows: today's bits)
    plain = p.trainer(layers)
    want = plain.run(EPOCHS)
    k = len(record)
    assert np.array_equal(np.asarray([r[0] for r in record], dtype=np.float32), want[0][:k])
    assert np.array_equal(np.asarray([r[1] for r in record]), want[1][:k])
    if len(models) == EPOCHS:
        for got, w_ in zip(models[-1], _bits(plain)):
            assert np.array_equal(got, w_)


def test_attach_rows_refusals(problem):
    from linkteller_amd import _lib, engine
    p = problem
    x_full, y_full = _dev(p.x_full), _dev(p.y_full)
    tr = p.trainer(2)
    bad = p.rows.copy()
    bad[100] = N_FULL
    for rows in (bad, _dev(bad), np.array([-1, 0]), torch.tensor([0, 2 ** 30])):
        with pytest.raises(IndexError):
            tr.attach_validation(p.adj_full, x_full, y_full, rows=rows)
    with pytest.raises(ValueError):
        tr.attach_validation(p.adj_full, x_full, y_full, rows=np.zeros(0, dtype=np.int64))
    # the C entry point checks the borrowed list itself and names the first offender
    h, g2, y32 = _lib.lib(), engine.as_hip_graph(p.adj_full), y_full.to(torch.int32)
    bad32 = _dev(bad.astype(np.int32))
    bad32[200] = -7
    for name, t in (("lt_gcn2_trainer_attach_validation_rows", tr), ("lt_gcn3_trainer_attach_validation_rows", p.trainer(3))):
        call = lambda rows, m: getattr(h, name)(t._h, g2.handle, x_full.data_ptr(), NF, N_FULL, y32.data_ptr(), 1, 0,
                                                None if rows is None else rows.data_ptr(), m, None)
        assert call(bad32, M_ROWS) == -1 and f"rows[100]={N_FULL} outside [0, {N_FULL})" in h.lt_last_error().decode()
        assert call(bad32, 0) == -1 and call(None, M_ROWS) == -1
        assert call(torch.from_numpy(p.rows.astype(np.int32)), M_ROWS) == -1                 # a host list
    with pytest.raises(ValueError):
        tr.run_validated(1)                                                                   # nothing was attached
    tr.attach_validation(p.adj_full, x_full, y_full, rows=p.rows[:1], keep_best=True)         # a list of one row
    r = tr.run_validated(2)
    assert r["val_counts"].sum(axis=(1, 2)).tolist() == [1, 1]
    with pytest.raises(ValueError):
        tr.attach_validation(p.adj_full, x_full, y_full, rows=p.rows)                         # a second attach


# ---------------------------------------------------------------------------------------------------------------------
# main --dataset flickr
# ---------------------------------------------------------------------------------------------------------------------
FLICKR_N, FLICKR_F = 300, 24
SAMPLE_SEED = 42        # the default --sample-seed: checked on the CPU to give 40 nodes with both edges and non-edges among them


def _flickr(root):
    """A synthetic flickr of 300 nodes, F = 24, 7 classes, mean degree 6, split 50 / 25 / 25; learnable (class centres)."""
    from linkteller_amd import synth
    rng = np.random.RandomState(31)
    adj = synth.erdos_renyi_graph(FLICKR_N, 900, seed=32).astype(np.float64)
    y = rng.randint(0, NC, FLICKR_N)
    feats = rng.standard_normal((NC, FLICKR_F))[y] * 1.5 + rng.standard_normal((FLICKR_N, FLICKR_F))
    perm = rng.permutation(FLICKR_N)
    roles = {"tr": perm[:150].tolist(), "va": perm[150:225].tolist(), "te": perm[225:].tolist()}
    synth.write_graphsaint_dataset(str(root), "flickr", adj, feats, y, roles)
    return adj


COMMAND = ("--dataset flickr --train --early --patience 5 --num-epochs 30 --hidden 16 --norm FirstOrderGCN --attack "
           "--attack-mode efficient --sample-type unbalanced --n-test 40").split()


def _run_main(cwd, data, monkeypatch, argv):
    """``main`` in process from ``cwd``; returns the ``GCNTrainer`` it built (caught at its ``test`` call)."""
    from linkteller_amd import main as lt_main, trainer as T
    caught = []
    real = T.GCNTrainer.test
    monkeypatch.setattr(T.GCNTrainer, "test", lambda self, *a, **k: (caught.append(self), real(self, *a, **k))[1])
    cwd.mkdir(exist_ok=True)
    monkeypatch.chdir(cwd)
    lt_main.main(argv + ["--data-root", str(data)])
    monkeypatch.setattr(T.GCNTrainer, "test", real)
    assert len(caught) == 1
    return caught[0]


def _torch_logits(sd, x, adj, dtype):
    a = adj.to_dense().to(dtype)
    h = torch.relu(a @ (x.to(dtype) @ sd["gc1.weight"].to(dtype)) + sd["gc1.bias"].to(dtype))
    return a @ (h @ sd["gc2.weight"].to(dtype)) + sd["gc2.bias"].to(dtype)


def test_main_flickr_end_to_end(tmp_path, monkeypatch, capsys):
    from sklearn.metrics import f1_score
    import sklearn.metrics as skm
    from oracle import linkteller_oracle as O
    data = tmp_path / "data"
    _flickr(data)
    tr = _run_main(tmp_path / "run0", data, monkeypatch, COMMAND)
    out = capsys.readouterr().out
    run0 = tmp_path / "run0"
    models, logs = glob.glob(str(run0 / "model_flickr" / "*" / "model.pt")), glob.glob(str(run0 / "logs_flickr" / "*.log"))
    assert len(models) == 1 and len(logs) == 1
    sd = torch.load(models[0], map_location="cpu")
    assert sorted(sd) == ["gc1.bias", "gc1.weight", "gc2.bias", "gc2.weight"]
    assert sd["gc1.weight"].shape == (FLICKR_F, 16) and sd["gc2.weight"].shape == (16, NC)

    # the log: loss_val / acc_val for every epoch run, and the early stop as the state on the device decided it
    log = open(logs[0]).read()
    lines = re.findall(r"\('Epoch: (\d+)', (.*?), 'time: [0-9.]+s'\)", log)
    fields = [re.fullmatch(r"'loss_train: ([0-9.]+)', 'acc_train: ([01]\.[0-9]{4})', 'loss_val: ([0-9.]+)', 'acc_val: ([01]\.[0-9]{4})'", b)
              for _, b in lines]
    state = tr.gpu_trainer.val_state()
    ran = state["stop_epoch"] + 1 if state["stop_epoch"] >= 0 else 30
    assert all(fields) and [int(e) for e, _ in lines] == list(range(1, ran + 1)), lines[:2]
    assert re.findall(r"early stop at epoch (\d+)", log) == ([str(state["stop_epoch"])] if state["stop_epoch"] >= 0 else [])

    # --early has the reference's meaning: the best model at a stop, the last model otherwise -- what a run of that many epochs
    # without --early leaves, and a second identical run leaves the same four tensors
    again = _run_main(tmp_path / "run1", data, monkeypatch, COMMAND)
    sd1 = torch.load(glob.glob(str(tmp_path / "run1" / "model_flickr" / "*" / "model.pt"))[0], map_location="cpu")
    assert all(torch.equal(sd[k], sd1[k]) for k in sd)
    keep = state["best_epoch"] + 1 if state["stop_epoch"] >= 0 else 30
    plain = [a for a in COMMAND if a not in ("--early", "--attack")]
    plain[plain.index("--num-epochs") + 1] = str(keep)
    _run_main(tmp_path / "run2", data, monkeypatch, plain)
    sd2 = torch.load(glob.glob(str(tmp_path / "run2" / "model_flickr" / "*" / "model.pt"))[0], map_location="cpu")
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    capsys.readouterr()
    print(f"{ran} epochs ran, state {state}")

    # losses against stock torch on the saved state dict; bound: the one between the library's numbers and fp64 elsewhere in the
    # suite, twice torch's own fp32 distance to fp64 plus 1e-5
    w = tr.worker
    x, adj, y = w.features.cpu(), w.adj_full.cpu(), w.labels.cpu().squeeze()
    z64, z32 = _torch_logits(sd, x, adj, torch.float64), _torch_logits(sd, x, adj, torch.float32)
    res = tr.split_results
    for name, idx, got in (("Validation", w.idx_val, res["loss_valid"]), ("Test", w.idx_test, res["loss_test"])):
        idx = torch.as_tensor(idx)
        l64, l32 = float(F.cross_entropy(z64[idx], y[idx])), float(F.cross_entropy(z32[idx], y[idx]))
        print(f"{name}: library {got:.9g}, torch fp64 {l64:.9g}, fp32 {l32:.9g}")
        assert abs(got - l64) <= 2 * abs(l32 - l64) + 1e-5
        assert f"[clean] {name} set results: loss = {got:.4f} " in out
    # F1 against sklearn on torch's argmax of the library's logits
    with torch.no_grad():
        logits = again.forward(mode="test")
        assert torch.equal(logits, tr.forward(mode="test"))
    pred = logits.argmax(1).cpu()
    for idx, got in ((w.idx_val, res["f1_valid"]), (w.idx_test, res["f1_test"])):
        want = [f1_score(y[idx], pred[idx], average=k) for k in ("micro", "macro", "weighted")]
        assert all(abs(g - s) <= 1e-12 for g, s in zip(got, want)), (got, want)
    f1 = res["f1_test"]
    assert f"f1_score = {res['f1_valid'][0]:.4f}" in out
    assert f"f1_score [micro, macro, weighted] = {f1[0]:.4f} {f1[1]:.4f} {f1[2]:.4f}" in out
    assert out.index("attacks done using") < out.index("Validation set results") < out.index("Test set results")
    assert res["f1_test"][0] > 2.0 / NC                                                   # it learned something

    # the attack's result file: the reference's schema, AUC / AP of the fp64 oracle on the same inputs
    name = f"eval_flickr/efficient_unbalanced_40_{SAMPLE_SEED}.pt"
    assert f"attack results saved to: {name}" in out
    saved = torch.load(run0 / name, weights_only=False)
    assert sorted(saved) == ["auc", "pr", "result"] and sorted(saved["auc"]) == ["fpr", "thresholds", "tpr"]
    assert sorted(saved["pr"]) == ["precision", "recall", "thresholds"] and sorted(saved["result"]) == ["pred", "y"]
    np.random.seed(SAMPLE_SEED)
    (ex, nex), nodes = O.sample_subgraph_pairs("flickr", "unbalanced", w.adj_ori, 40)
    assert len(ex) > 0 and len(nex) > 0
    P = {k: sd[n].double() for k, n in zip(("W1", "b1", "W2", "b2"), ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias"))}
    infl = O.influence_matrix(x.double(), adj.double(), P, nodes, 1e-4)
    m = O.attack_metrics(*O.pair_scores(infl, nodes, ex, nex))
    assert saved["result"]["y"] == m["y"]
    auc, ap = skm.auc(saved["auc"]["fpr"], saved["auc"]["tpr"]), skm.average_precision_score(saved["result"]["y"], saved["result"]["pred"])
    print(f"auc {auc:.6f} (oracle {m['auc']:.6f}), ap {ap:.6f} (oracle {m['ap']:.6f}), {len(ex)} edges / {len(nex)} non-edges")
    assert abs(auc - m["auc"]) <= 1e-4 and abs(ap - m["ap"]) <= 1e-4


def test_worker_dp_builds_agree(tmp_path):
    """``--mode vanilla --perturb-type continuous --epsilon 5 --noise-rng philox``: ``--dp-build device`` serves the graphs of
    ``--dp-build host`` (stored zeros dropped, values in float32) for both graphs of the family, and ``adj_ori`` stays clean."""
    from linkteller_amd.worker import Worker
    clean = _flickr(tmp_path)
    workers = []
    for build in ("host", "device"):
        args = argparse.Namespace(norm="FirstOrderGCN", perturb_type="continuous", epsilon=5.0, noise_seed=42, noise_type="laplace",
                                  delta=1e-5, noise_rng="philox", dp_build=build)
        workers.append(Worker(args, dataset="flickr", mode="vanilla", data_root=str(tmp_path)))
    host, dev = workers
    for w in workers:
        assert (sp.csr_matrix(w.adj_ori) != clean).nnz == 0 and w.adj_ori.nnz == clean.nnz
        assert w.features.is_cuda and w.features_train.is_cuda and w.labels.is_cuda
    assert torch.equal(host.features, dev.features) and torch.equal(host.labels, dev.labels)
    for name, n in (("adj_train", 150), ("adj_full", FLICKR_N)):
        h, d = getattr(host, name), getattr(dev, name)
        assert d.is_cuda and d.is_sparse and d.dtype == torch.float32 and tuple(d.shape) == tuple(h.shape) == (n, n)
        hi, hv = h._indices().cpu().numpy(), h._values().cpu().numpy()
        keep = hv != 0
        assert np.array_equal(d._indices().cpu().numpy(), hi[:, keep])
        assert np.array_equal(d._values().cpu().numpy().view(np.uint32), hv[keep].view(np.uint32))
    clean_hat = Worker(argparse.Namespace(norm="FirstOrderGCN"), dataset="flickr", mode="vanilla-clean", data_root=str(tmp_path))
    assert not torch.equal(clean_hat.adj_full._indices().cpu(), dev.adj_full._indices().cpu())       # the served graph is perturbed


def test_main_multi_label_from_a_saved_model(tmp_path, monkeypatch, capsys):
    """``ppi`` (multi-label) is not trained here, but it loads, tests and attacks from a saved model: the validation / test lines
    are the reference's host arithmetic (BCE with logits, ``sigmoid > 0.5``, sklearn) on the library's logits."""
    from sklearn.metrics import f1_score
    from conftest import load_golden
    from linkteller_amd import synth
    from linkteller_amd.gcn import GCN
    g = load_golden("graphsaint_loader.npz")
    adj = sp.csr_matrix((g["in.adj.data"], g["in.adj.indices"], g["in.adj.indptr"]), shape=tuple(g["in.adj.shape"]))
    roles = {k: g[f"in.role.{k}"].tolist() for k in ("tr", "va", "te")}
    synth.write_graphsaint_dataset(str(tmp_path / "data"), "ppi", adj, g["in.feats"], g["in.labels.ppi"], roles)
    torch.manual_seed(0)
    torch.save(GCN(12, 16, 5, 0.5).state_dict(), tmp_path / "model.pt")
    tr = _run_main(tmp_path / "run", tmp_path / "data", monkeypatch,
                   f"--dataset ppi --test --model-path {tmp_path}/model.pt --hidden 16 --norm FirstOrderGCN --attack --attack-mode "
                   "efficient --sample-type unbalanced --n-test 20".split())
    out = capsys.readouterr().out
    w, res = tr.worker, tr.split_results
    assert w.multi_label == 5 and w.n_classes == 5 and "attack results saved to: eval_ppi/efficient_unbalanced_20_42.pt" in out
    with torch.no_grad():
        logits = tr.forward(mode="test").cpu()
    y = w.labels.cpu()
    for key, idx in (("valid", w.idx_val), ("test", w.idx_test)):
        want_loss = float(F.binary_cross_entropy_with_logits(logits[idx], y[idx].float()))
        pred = torch.sigmoid(logits[idx]) > 0.5
        want = [f1_score(y[idx], pred, average=k) for k in ("micro", "macro", "weighted")]
        assert abs(res[f"loss_{key}"] - want_loss) <= 1e-6 and all(abs(a - b) <= 1e-12 for a, b in zip(res[f"f1_{key}"], want))
    assert f"[clean] Test set results: loss = {res['loss_test']:.4f} f1_score [micro, macro, weighted] = " in out

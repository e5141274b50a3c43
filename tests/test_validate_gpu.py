"""Validation every epoch on the GPU (lt_eval_head, lt_early_stop_*, lt_gcn*_trainer_attach_validation / _run_validated /
_val_state / _restore_best / _val_logits; engine.GCN2Trainer / GCN3Trainer; ``--validate``) against the numpy restatements
(validate_restate.py) and the reference's recorded runs (golden/validate.npz, train.npz, train3.npz)."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import REPO, load_golden
import validate_restate as V

pytestmark = pytest.mark.gpu

LR, DECAY, EPOCHS = 0.01, 5e-4, 40
ROWS2 = ["FirstOrderGCN.h16", "FirstOrderGCN.h64", "AugRWalk.h16", "AugRWalk.h64"]
ROWS3 = ["FirstOrderGCN.h16_16", "FirstOrderGCN.h64_32", "AugRWalk.h16_16", "AugRWalk.h64_32"]


@pytest.fixture(scope="module")
def gold():
    return {"train": load_golden("train.npz"), "train3": load_golden("train3.npz"), "val": load_golden("validate.npz")}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _csr(g, norm, tag):
    n = g[f"{norm}.{tag}.indptr"].shape[0] - 1
    return sp.csr_matrix((g[f"{norm}.{tag}.data"], g[f"{norm}.{tag}.indices"], g[f"{norm}.{tag}.indptr"]), shape=(n, n))


class Case:
    """One fixture row: the two graphs, the data and a factory of fresh trainers from the row's initial weights."""

    def __init__(self, gold, key):
        self.key, self.gcn3 = key, "_" in key.split(".h")[1]
        norm = key.split(".")[0]
        t = gold["train"]
        self.src = gold["train3"] if self.gcn3 else t
        self.adj1, self.adj2 = _csr(t, norm, "adj1"), _csr(t, norm, "adj2")
        self.x1, self.x2, self.y1, self.y2 = t["x1"], t["x2"], t["y1"], t["y2"]
        self.names = [f"gc{i}.{w}" for i in range(1, 4 if self.gcn3 else 3) for w in ("weight", "bias")]

    def trainer(self, dropout=0.0, seed=42):
        from linkteller_amd import engine
        params = [_dev(self.src[f"{self.key}.init.{k}"].copy()) for k in self.names]
        cls = engine.GCN3Trainer if self.gcn3 else engine.GCN2Trainer
        return cls(self.adj1, _dev(self.x1), _dev(self.y1), *params, lr=LR, weight_decay=DECAY, dropout=dropout, seed=seed)

    def attached(self, keep_best=True, patience=0, dropout=0.0, seed=42, on_train_graph=False):
        tr = self.trainer(dropout, seed)
        if on_train_graph:
            tr.attach_validation(self.adj1, _dev(self.x1), _dev(self.y1), keep_best=keep_best, patience=patience)
        else:
            tr.attach_validation(self.adj2, _dev(self.x2), _dev(self.y2), keep_best=keep_best, patience=patience)
        return tr


def _bits(tr):
    return [p.cpu().numpy().copy() for p in tr.params]


# ---------------------------------------------------------------------------------------------------------------------
# the head alone
# ---------------------------------------------------------------------------------------------------------------------
def _head_case(n, c, seed):
    """Logits [n, c] as a view of a wider buffer (ldz = c + 3), loss O(1): gaussian rows; every 5th row has tied maxima (the
    first must win); every 7th row has magnitude 80 with the maximum on its own label.  Class c - 1 is absent from the labels."""
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((n, c)).astype(np.float32)
    y = rng.randint(0, max(c - 1, 1), n).astype(np.int64)
    if c > 1:
        rows = np.arange(0, n, 5)
        a, b = rng.randint(0, c, rows.size), rng.randint(0, c, rows.size)
        top = z[rows].max(axis=1) + np.float32(0.5)
        z[rows, a] = top
        z[rows, b] = top
    big = np.arange(3, n, 7)
    z[big] = np.float32(-80.0)
    z[big, y[big]] = np.float32(80.0)
    if c > 2:
        z[big[::2], c - 1] = np.float32(80.0)      # a tie at 80 with a later class
    return z, y


@pytest.mark.parametrize("c", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_eval_head_against_restatement(n, c):
    from linkteller_amd import engine
    z, y = _head_case(n, c, 100 * c + n % 97)
    wide = torch.full((n, c + 3), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :c] = _dev(z)
    view = wide[:, :c]
    assert view.stride(0) == c + 3
    loss, conf = engine.eval_head(view, _dev(y))
    loss_b, conf_b = engine.eval_head(view, _dev(y))
    l64, c64 = V.head(z, y, np.float64)
    l32, c32 = V.head(z, y, np.float32)
    got, got_conf = float(loss.cpu()), conf.cpu().numpy().astype(np.int64)
    print(f"n={n} C={c}: dev {got:.9g} l64 {l64:.9g} l32 {l32:.9g} |dev-l64| {abs(got - l64):.3g} |l32-l64| {abs(l32 - l64):.3g}")
    assert np.array_equal(got_conf, c64) and np.array_equal(c32, c64)
    assert got_conf.sum() == n and (c == 1 or got_conf[c - 1].sum() == 0)
    assert 0.0 <= l64 < 4.0
    assert abs(got - l64) <= 2 * abs(l32 - l64) + 1e-5
    assert torch.equal(loss.view(torch.int32), loss_b.view(torch.int32)) and torch.equal(conf, conf_b)


def test_eval_head_refusals():
    from linkteller_amd import _lib
    h = _lib.lib()
    z, y = torch.zeros((4, 2), device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    loss, conf = torch.zeros((), device="cuda"), torch.zeros((2, 2), dtype=torch.int32, device="cuda")
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda")
    args = lambda n, c, ldz, nbytes: (z.data_ptr(), ldz, y.data_ptr(), n, c, loss.data_ptr(), conf.data_ptr(), ws.data_ptr(),
                                      nbytes, None)
    assert h.lt_eval_head(*args(0, 2, 2, 64)) == -1
    assert h.lt_eval_head(*args(4, 9, 9, 64)) == -1
    assert h.lt_eval_head(*args(4, 2, 1, 64)) == -1
    assert h.lt_eval_head(*args(4, 2, 2, 8)) == _lib.LT_ERR_WORKSPACE
    assert h.lt_eval_head_workspace_bytes(4, 2) == 4 * (1 + 4) and h.lt_eval_head_workspace_bytes(65537, 8) == 257 * 65 * 4
    assert h.lt_eval_head_workspace_bytes(4, 9) == 0
    assert h.lt_early_stop_update(loss.data_ptr(), -1, 0, ws.data_ptr(), None) == -1
    assert h.lt_early_stop_update(None, 1, 0, ws.data_ptr(), None) == -1 and h.lt_early_stop_reset(None, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the state kernel alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,losses,patience,want,counter", V.HAND_SEQUENCES, ids=[h[0] for h in V.HAND_SEQUENCES])
def test_state_kernel_word_for_word(name, losses, patience, want, counter):
    from linkteller_amd import engine
    st = engine.EarlyStopState(patience)
    ref = V.state_reset()
    assert np.array_equal(st.read(), ref)
    dev_losses = _dev(np.asarray(losses, dtype=np.float32))
    for e in range(len(losses)):
        st.update(dev_losses[e:e + 1], e)
        ref = V.state_update(ref, losses[e], patience, e)
        assert np.array_equal(st.read(), ref), (name, e, st.read(), ref)
    assert (int(ref[V.BEST_EPOCH]), int(ref[V.STOP_EPOCH])) == want and int(ref[V.COUNTER]) == counter


# ---------------------------------------------------------------------------------------------------------------------
# per-epoch validation inside the trainers
# ---------------------------------------------------------------------------------------------------------------------
def _check_records(gold, key, r):
    v = gold["val"]
    l64, l32 = v[f"{key}.loss_val64"], v[f"{key}.loss_val32"]
    err, e32 = np.abs(r["val_loss"] - l64).max(), np.abs(l32 - l64).max()
    trace = np.trace(r["val_counts"], axis1=1, axis2=2)
    trace64 = np.trace(v[f"{key}.counts64"], axis1=1, axis2=2)
    print(f"{key}: |val_loss - l64| {err:.3g}, |l32 - l64| {e32:.3g}, trace diff max {np.abs(trace - trace64).max()}")
    assert r["val_loss"].shape == (EPOCHS,) and r["val_counts"].shape == (EPOCHS, 2, 2)
    assert err <= 2 * e32 + 1e-5
    assert np.all(np.abs(trace - trace64) <= v[f"{key}.tiny_val64"])
    assert np.all(r["val_counts"].sum(axis=(1, 2)) == 250)


@pytest.mark.parametrize("key", ROWS2)
def test_gcn2_validation_every_row(gold, key):
    from linkteller_amd import engine
    case = Case(gold, key)
    tr = case.attached(keep_best=True, patience=0)
    x2 = _dev(case.x2)
    first = tr.run_validated(1)
    assert torch.equal(tr.val_logits(), engine.gcn2_forward(case.adj2, x2, *tr.params))        # after epoch 0
    rest = tr.run_validated(EPOCHS - 1)
    assert torch.equal(tr.val_logits(), engine.gcn2_forward(case.adj2, x2, *tr.params))        # after epoch 39
    r = {k: np.concatenate([first[k], rest[k]]) for k in ("loss", "correct", "val_loss", "val_counts")}
    _check_records(gold, key, r)
    assert rest["stop_epoch"] == -1 and rest["best_epoch"] == V.decide(r["val_loss"], 0)[0]
    # the train record is the plain run's
    t = gold["train"]
    assert np.abs(r["loss"] - t[f"{key}.loss64"]).max() <= 2 * np.abs(t[f"{key}.loss32"] - t[f"{key}.loss64"]).max() + 1e-5


@pytest.mark.parametrize("key", ROWS3)
def test_gcn3_validation_every_row(gold, key):
    case = Case(gold, key)
    tr = case.attached(keep_best=True, patience=0)
    r = tr.run_validated(EPOCHS)
    _check_records(gold, key, r)
    assert r["stop_epoch"] == -1 and r["best_epoch"] == V.decide(r["val_loss"], 0)[0]
    z = tr.val_logits().cpu().numpy().astype(np.float64)
    z64, z32 = gold["train3"][f"{key}.logits2_64"], gold["train3"][f"{key}.logits2_32"]
    assert np.abs(z - z64).max() <= 2 * np.abs(z32 - z64).max() + 1e-5 * np.abs(z64).max(), \
        (np.abs(z - z64).max(), np.abs(z32 - z64).max())


@pytest.mark.parametrize("patience", [3, 10])
@pytest.mark.parametrize("key", ROWS2 + ROWS3)
def test_early_stopping_matches_the_reference(gold, key, patience):
    case = Case(gold, key)
    want = tuple(int(v) for v in gold["val"][f"{key}.p{patience}"])
    runs = {}
    for chunk in (None, 1, 7, 40):
        tr = case.attached(keep_best=True, patience=patience)
        r = tr.run_validated(EPOCHS, chunk=chunk)
        state = tr.val_state()
        tr.restore_best()
        runs[chunk] = (r, state, _bits(tr))
        assert (r["best_epoch"], r["stop_epoch"]) == want, (chunk, r["best_epoch"], r["stop_epoch"], want)
        assert (state["best_epoch"], state["stop_epoch"]) == want and state["improved"] == 0
        assert len(r["loss"]) == len(r["val_loss"]) == len(r["val_counts"]) == want[1] + 1
        assert np.float32(state["best_loss"]) == r["val_loss"][want[0]]
    # the selected model: a fresh, identical trainer run for exactly best_epoch + 1 epochs
    fresh = case.trainer()
    fresh.run(want[0] + 1)
    model = _bits(fresh)
    base = runs[1]
    for chunk, (r, state, bits) in runs.items():
        for k in ("loss", "correct", "val_loss", "val_counts"):
            assert np.array_equal(r[k], base[0][k]), (chunk, k)
        assert state == base[1], (chunk, state, base[1])        # 40 epochs enqueued in one go: the state froze at the stop
        for a, b in zip(bits, model):
            assert np.array_equal(a, b), chunk


@pytest.mark.parametrize("key", ["AugRWalk.h64", "FirstOrderGCN.h64_32"])
def test_validation_on_the_training_graph_is_the_next_epochs_forward(gold, key):
    """Dropout 0: epoch e's validation forward and epoch e + 1's training forward see the same parameters and the same
    graph.  The counts agree exactly; the two mean losses are fp32 sums of bit-identical row losses in different orders."""
    case = Case(gold, key)
    tr = case.attached(keep_best=False, patience=0, on_train_graph=True)
    r = tr.run_validated(EPOCHS)
    n = case.x1.shape[0]
    assert np.array_equal(np.trace(r["val_counts"], axis1=1, axis2=2)[:-1], r["correct"][1:])
    rel = np.abs(r["val_loss"][:-1].astype(np.float64) - r["loss"][1:]) / r["loss"][1:]
    print(f"{key}: relative difference of the two sums, max {rel.max():.3g} (bound {2 * n * 2.0 ** -24:.3g})")
    assert rel.max() <= 2 * n * 2.0 ** -24


@pytest.mark.parametrize("key", ["AugRWalk.h64", "FirstOrderGCN.h64_32"])
def test_validation_does_not_disturb_training(gold, key):
    case = Case(gold, key)
    plain = case.trainer(dropout=0.5, seed=7)
    want = plain.run(EPOCHS)
    validated = case.attached(keep_best=True, patience=0, dropout=0.5, seed=7)
    r = validated.run_validated(EPOCHS)
    assert np.array_equal(r["loss"], want[0]) and np.array_equal(r["correct"], want[1])
    for a, b in zip(_bits(validated), _bits(plain)):
        assert np.array_equal(a, b)
    assert validated.epoch == EPOCHS
    # plain run() on an attached trainer keeps its meaning
    attached = case.attached(keep_best=True, patience=3, dropout=0.5, seed=7)
    got = attached.run(EPOCHS)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for a, b in zip(_bits(attached), _bits(plain)):
        assert np.array_equal(a, b)
    assert attached.val_state()["seen"] == 0


def test_shapes_with_hub_rows_and_odd_widths():
    """A validation graph with rows longer than one segment, a hidden width that is no multiple of 4 (the scalar snapshot
    path) and 3 classes: the validation logits are the forward's bits and the snapshot is the best epoch's model."""
    from linkteller_amd import engine, graph, synth
    n1, n2, f, h, c = 500, 700, 120, 30, 3
    adj1 = graph.aug_random_walk(synth.powerlaw_graph(n1, 3000, seed=2))
    adj2 = graph.aug_random_walk(synth.powerlaw_graph(n2, 9000, seed=5))
    x1 = synth.twitch_like_features(n1, f, seed=3, density=0.05)
    x2 = synth.twitch_like_features(n2, f, seed=6, density=0.05)
    y1, y2 = (np.arange(n1) * 7 % c).astype(np.int64), (np.arange(n2) * 5 % c).astype(np.int64)
    w = synth.gcn_weights(f, h, c, seed=4)

    def make():
        params = [_dev(w[k].copy()) for k in ("W1", "b1", "W2", "b2")]
        return engine.GCN2Trainer(adj1, _dev(x1), _dev(y1), *params, lr=LR, weight_decay=DECAY, dropout=0.0, seed=1)
    tr = make()
    tr.attach_validation(adj2, _dev(x2), _dev(y2), keep_best=True, patience=0)
    r = tr.run_validated(12)
    assert torch.equal(tr.val_logits(), engine.gcn2_forward(adj2, _dev(x2), *tr.params))
    z = tr.val_logits().cpu().numpy()
    l64, c64 = V.head(z, y2, np.float64)
    l32, _ = V.head(z, y2, np.float32)
    assert np.array_equal(r["val_counts"][-1], c64) and abs(float(r["val_loss"][-1]) - l64) <= 2 * abs(l32 - l64) + 1e-5
    tr.restore_best()
    fresh = make()
    fresh.run(r["best_epoch"] + 1)
    for a, b in zip(_bits(tr), _bits(fresh)):
        assert np.array_equal(a, b)


def test_refusals(gold):
    from linkteller_amd import _lib
    case = Case(gold, "AugRWalk.h16")
    x2, y2 = _dev(case.x2), _dev(case.y2)
    before = [p.clone() for p in case.trainer().params]
    tr = case.trainer()
    with pytest.raises(ValueError):
        tr.run_validated(1)                                              # nothing attached
    with pytest.raises(ValueError):
        tr.val_state()
    with pytest.raises(ValueError):
        tr.attach_validation(case.adj2, x2[:-1], y2[:-1])                # rows of X2 that do not match the graph
    bad = case.y2.copy()
    bad[7] = 2
    with pytest.raises(ValueError):
        tr.attach_validation(case.adj2, x2, _dev(bad))                   # a label outside [0, C)
    with pytest.raises(ValueError):
        tr.attach_validation(case.adj2, x2, y2, patience=-1)             # negative patience
    if torch.cuda.device_count() >= 2:                                   # another device
        with pytest.raises(ValueError):
            tr.attach_validation(case.adj2, x2.to("cuda:1"), y2)
    # the same refusals at the C boundary, every one LT_ERR_INVALID
    from linkteller_amd.graph import as_hip_graph
    g2, y32 = as_hip_graph(case.adj2), y2.to(torch.int32)
    h = _lib.lib()

    def attach(n2=250, labels=y32, keep=1, patience=0, x=x2):
        return h.lt_gcn2_trainer_attach_validation(tr._h, g2.handle, x.data_ptr(), x.shape[1], n2, labels.data_ptr(), keep,
                                                   patience, None)
    assert attach(n2=249) == -1 and b"rows" in h.lt_last_error()
    assert attach(labels=_dev(bad).to(torch.int32)) == -1 and b"labels2[7]=2" in h.lt_last_error()
    assert attach(patience=-1) == -1 and attach(keep=2) == -1
    assert attach(x=torch.from_numpy(case.x2).pin_memory()) == -1 and b"device" in h.lt_last_error()      # not device memory
    rec = torch.zeros((1, 2), device="cuda")
    vl, vc = torch.zeros(1, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    assert h.lt_gcn2_trainer_run_validated(tr._h, 1, rec.data_ptr(), vl.data_ptr(), vc.data_ptr(), None) == -1
    assert h.lt_gcn2_trainer_restore_best(tr._h, None) == -1
    torch.cuda.synchronize()
    assert tr.epoch == 0 and all(torch.equal(a, b) for a, b in zip(tr.params, before))      # nothing was launched
    tr.attach_validation(case.adj2, x2, y2, keep_best=False, patience=2)
    with pytest.raises(ValueError):
        tr.attach_validation(case.adj2, x2, y2)                          # a second attach
    assert attach() == -1 and b"already attached" in h.lt_last_error()
    with pytest.raises(ValueError):
        tr.restore_best()                                                # attached without keep_best
    assert h.lt_gcn2_trainer_restore_best(tr._h, None) == -1
    with pytest.raises(ValueError):
        tr.run_validated(4, chunk=0)
    assert h.lt_gcn2_trainer_run_validated(tr._h, -1, rec.data_ptr(), vl.data_ptr(), vc.data_ptr(), None) == -1
    assert h.lt_gcn2_trainer_run_validated(tr._h, 1, rec.data_ptr(), None, vc.data_ptr(), None) == -1
    assert tr.epoch == 0
    # the 3-layer trainer refuses the same way
    tr3 = Case(gold, "AugRWalk.h16_16").trainer()
    with pytest.raises(ValueError):
        tr3.run_validated(1)
    assert h.lt_gcn3_trainer_attach_validation(tr3._h, g2.handle, x2.data_ptr(), x2.shape[1], 249, y32.data_ptr(), 1, 0, None) == -1
    assert h.lt_gcn3_trainer_attach_validation(tr3._h, g2.handle, x2.data_ptr(), x2.shape[1], 250, y32.data_ptr(), 1, -3, None) == -1
    assert h.lt_gcn3_trainer_run_validated(tr3._h, 1, rec.data_ptr(), vl.data_ptr(), vc.data_ptr(), None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def _main(cwd, args):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "linkteller_amd.main"] + args, cwd=cwd, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _tiny_twitch(tmp_path):
    from linkteller_amd import synth
    data = tmp_path / "data"
    synth.write_musae_dataset(str(data), "ES", synth.erdos_renyi_graph(200, 800, seed=21), 3170, 21)
    synth.write_musae_dataset(str(data), "RU", synth.erdos_renyi_graph(150, 600, seed=22), 3170, 22)
    return ["--dataset", "twitch/ES/RU", "--norm", "FirstOrderGCN", "--mode", "vanilla-clean"]


def _epoch_lines(log):
    return re.findall(r"\('Epoch: (\d+)', (.*?), 'time: [0-9.]+s'\)", log)


def test_cli_validate_early(tmp_path):
    common = _tiny_twitch(tmp_path)
    out = _main(str(tmp_path), ["--train", "--num-epochs", "200", "--validate", "early", "--patience", "3"] + common)
    assert "Optimization Finished!" in out
    models = glob.glob(str(tmp_path / "model_twitch" / "ES" / "RU" / "*" / "model.pt"))
    logs = glob.glob(str(tmp_path / "logs_twitch" / "ES" / "RU" / "*.log"))
    assert len(models) == 1 and len(logs) == 1
    log = open(logs[0]).read()
    lines = _epoch_lines(log)
    fields = [re.fullmatch(r"'loss_train: ([0-9.]+)', 'acc_train: ([0-9.]+)', 'loss_val: ([0-9.]+)', 'acc_val: ([0-9.]+)'", body)
              for _, body in lines]
    assert lines and all(fields), lines[:2]
    assert [int(e) for e, _ in lines] == list(range(1, len(lines) + 1))
    val = [float(m.group(3)) for m in fields]
    assert all(0.0 <= float(m.group(4)) <= 1.0 for m in fields)
    stops = re.findall(r"early stop at epoch (\d+)", log)
    best, stop = V.decide(val, 3)            # the log's own losses under the restatement
    print(f"{len(lines)} epochs logged, restatement on the logged losses: best {best}, stop {stop}; stop lines {stops}")
    assert len(lines) < 200 and stops == [str(stop)] and len(lines) == stop + 1
    assert re.search(r"best validation loss [0-9.]+ at epoch \d+: that model is saved", out)
    _main(str(tmp_path), ["--test", "--model-path", models[0]] + common)
    sd = torch.load(models[0], map_location="cpu")
    assert sorted(sd) == ["gc1.bias", "gc1.weight", "gc2.bias", "gc2.weight"]


def _gcntrainer_run(tmp_path, monkeypatch, name, argv):
    """The calls of main's _train in process (the documented way to train a GCN3): returns (log text, saved state_dict)."""
    import logging
    import random
    from linkteller_amd import main as lt_main
    from linkteller_amd.trainer import GCNTrainer
    from linkteller_amd.worker import Worker
    monkeypatch.chdir(tmp_path)
    args = lt_main.get_arguments(argv)
    lt_main.check_validate(args)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    handler = lt_main.init_logger("./logs_{}".format(args.dataset), name)
    try:
        trainer = GCNTrainer(args, subdir=name, worker=Worker(args, dataset=args.dataset, mode=args.mode, data_root=args.data_root))
        trainer.init_model()
        trainer.train()
    finally:
        logging.getLogger().removeHandler(handler)
        handler.close()
    log = open(tmp_path / "logs_twitch" / "ES" / "RU" / f"{name}.log").read()
    return log, torch.load(tmp_path / "model_twitch" / "ES" / "RU" / name / "model.pt", map_location="cpu")


@pytest.mark.parametrize("layers", [["--n-layer", "2"], ["--n-layer", "3", "--hidden1", "16", "--hidden2", "8"]])
def test_gcntrainer_validate_log_and_best(tmp_path, monkeypatch, layers):
    """``GCNTrainer.train()`` with ``--validate`` for both model families: ``log`` saves the model a plain run saves and logs
    the two validation fields; ``best`` saves the model of the best logged epoch, which is what a plain run of
    ``best_epoch + 1`` epochs leaves."""
    common = _tiny_twitch(tmp_path) + layers
    plain_log, plain = _gcntrainer_run(tmp_path, monkeypatch, "plain", ["--train", "--num-epochs", "12"] + common)
    log, logged = _gcntrainer_run(tmp_path, monkeypatch, "log", ["--train", "--num-epochs", "12", "--validate", "log"] + common)
    assert sorted(plain) == sorted(logged) and all(torch.equal(plain[k], logged[k]) for k in plain)
    lines, plain_lines = _epoch_lines(log), _epoch_lines(plain_log)
    assert len(lines) == 12 and [b for _, b in lines] != [b for _, b in plain_lines]
    assert [b.split(", 'loss_val")[0] for _, b in lines] == [b for _, b in plain_lines]      # the train fields are unchanged
    assert all(re.search(r"'loss_val: [0-9.]+', 'acc_val: [01]\.[0-9]{4}'$", b) for _, b in lines)
    assert "early stop" not in log and "best validation loss" not in log
    best_log, best = _gcntrainer_run(tmp_path, monkeypatch, "best", ["--train", "--num-epochs", "12", "--validate", "best"] + common)
    assert _epoch_lines(best_log) == lines and "early stop" not in best_log
    m = re.search(r"best validation loss ([0-9.]+) at epoch (\d+): that model is saved", best_log)
    assert m, best_log[-500:]
    e = int(m.group(2))
    assert f"'loss_val: {m.group(1)}'" in lines[e][1]
    _, upto = _gcntrainer_run(tmp_path, monkeypatch, "upto", ["--train", "--num-epochs", str(e + 1)] + common)
    assert all(torch.equal(best[k], upto[k]) for k in best)


def test_cli_validate_off_is_todays_run(tmp_path, monkeypatch):
    """``main`` itself, in process (the child-process route is test_cli_validate_early's): the default and ``--validate off``."""
    from linkteller_amd import main as lt_main
    runs = []
    for i, extra in enumerate(([], ["--validate", "off"])):
        cwd = tmp_path / f"run{i}"
        cwd.mkdir()
        common = _tiny_twitch(cwd)
        monkeypatch.chdir(cwd)
        lt_main.main(["--train", "--num-epochs", "20"] + extra + common)      # (the 20 epochs of test_cli_train_then_attack)
        log = open(glob.glob(str(cwd / "logs_twitch" / "ES" / "RU" / "*.log"))[0]).read()
        sd = torch.load(glob.glob(str(cwd / "model_twitch" / "ES" / "RU" / "*" / "model.pt"))[0], map_location="cpu")
        runs.append((_epoch_lines(log), sd))
        assert "loss_val" not in log and "early stop" not in log
    assert len(runs[0][0]) == 20 and runs[0][0] == runs[1][0]
    assert re.fullmatch(r"'loss_train: [0-9.]+', 'acc_train: [0-9.]+'", runs[0][0][0][1])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k])

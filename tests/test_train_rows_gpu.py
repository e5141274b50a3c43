"""Training on a listed subset of the rows (lt_gcn*_trainer_set_train_rows; engine.GCN2Trainer / GCN3Trainer(train_rows=),
``main --train-setting transductive``): the whole graph is forwarded, the loss head sees the listed rows only.

The list 0 .. n - 1 trains the bits of a trainer without a list on every route, which pins the listed heads' arithmetic to the
existing heads'; lists of every length around TR_BLOCK = 256 are held to train_rows_restate.epoch_reference_rows in fp64 by the
project's gate (train_cases.gate: err_hip <= 2 err_fp32 + 1e-6 max|ref64| + 1e-12, at read-back parameters, the gradients
against the fp64 derivative under the device's own ReLU pattern, as test_train_wide_gpu.py does); labels off the list do not
matter; a changed list leaves no stale gradient rows; refused lists leave the trainer as it was; validation does not see the
list; and ``main`` trains, saves, tests and attacks a flickr and a ppi fixture transductively."""
import ctypes as C
import glob
import re

import numpy as np
import pytest
import torch

import train_cases as K
import train_rows_restate as R

pytestmark = pytest.mark.gpu

INVALID = -1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(ts):
    return [t.cpu().numpy().copy() for t in ts]


_cases = {}


def _case(c, loss, graph_kind="er"):
    if (c, loss, graph_kind) not in _cases:
        _cases[c, loss, graph_kind] = R.make(c, loss, graph_kind)
    return _cases[c, loss, graph_kind]


def _params(case, layers):
    """Fresh device parameters: the case's four, or for GCN3 six of widths F -> H -> 16 -> C."""
    if layers == 2:
        return [_dev(p.copy()) for p in case["params"]]
    from linkteller_amd import synth
    w, w3 = synth.gcn_weights(case["F"], case["H"], 16, seed=4), synth.gcn_weights(16, case["C"], case["C"], seed=8)
    return [_dev(w[k].copy()) for k in ("W1", "b1", "W2", "b2")] + [_dev(w3["W1"].copy()), _dev(w3["b1"].copy())]


def _trainer(case, params, head, rows=None, dropout=None, y=None, lr=K.LR):
    from linkteller_amd import engine
    cls = engine.GCN2Trainer if len(params) == 4 else engine.GCN3Trainer
    kw = dict(head="wide", loss=case["loss"]) if head == "wide" else {}
    if rows is not None:
        kw["train_rows"] = rows
    return cls(case["adj"], _dev(case["x"]), _dev(case["y"] if y is None else y), *params, lr=lr, weight_decay=K.DECAY,
               dropout=case["p"] if dropout is None else dropout, seed=K.SEED, **kw)


def _state(tr, params, record=None):
    """Everything two trainers must agree on, as host arrays."""
    out = ([] if record is None else [record]) + _host(tr.grads()) + [tr.logits().cpu().numpy()] + _host(params)
    if tr.head == "wide":
        out.append(tr.counts().cpu().numpy())
    return out


def _same(a, b, tag):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.dtype == v.dtype and np.array_equal(u.view(np.uint8), v.view(np.uint8)), (tag, i)


#           id,             layers, C, loss, head
ROUTES = [("gcn2-narrow-c2", 2, 2, "ce", "narrow"), ("gcn2-narrow-c7", 2, 7, "ce", "narrow"),
          ("gcn2-wide-ce41", 2, 41, "ce", "wide"), ("gcn2-wide-bce9", 2, 9, "bce", "wide"),
          ("gcn3-narrow", 3, 7, "ce", "narrow"), ("gcn3-wide", 3, 41, "ce", "wide")]


@pytest.mark.parametrize("layers,c,loss,head", [r[1:] for r in ROUTES], ids=[r[0] for r in ROUTES])
def test_identity_list_is_no_list(layers, c, loss, head):
    """3 epochs at p = 0.5: a trainer with the list 0 .. n - 1 and one without a list agree bit for bit on the record, the
    gradients, the logits, the parameters and (wide) the counts."""
    case = _case(c, loss)
    runs = []
    for rows in (None, np.arange(case["n"])):
        params = _params(case, layers)
        tr = _trainer(case, params, head, rows=rows)
        assert tr.n_train == case["n"]
        rec = tr.run_async(3).cpu().numpy()
        assert np.isfinite(rec).all()
        runs.append(_state(tr, params, rec))
    _same(runs[0], runs[1], (layers, c, loss, head))
    assert not np.array_equal(runs[0][-1 - (head == "wide")], _host(_params(case, layers))[-1])      # the class bias moved


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 gate
# ---------------------------------------------------------------------------------------------------------------------
def _graph_for(c):
    return {3: "directed", 33: "directed", 8: "hub", 121: "hub"}.get(c, "er")


def _check_epoch(case, tr, params, rows, epoch, tag):
    torch.set_num_threads(1)
    start = _host(params)
    loss, correct = tr.run(1)
    assert tr.epoch == epoch + 1
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(R.NAMES, tr.grads())}
    got["Z2"], got["H1d"] = (t.cpu().numpy().astype(np.float64) for t in (tr.logits(), tr.hidden()))
    got["loss"] = float(loss[0])
    an = R.analyse(case, start, epoch, rows)
    r64, r32 = an["r64"], an["r32"]
    on = got["H1d"] > 0
    diff = on != (an["keep"] & (r64["Z1"] > 0))
    print(f"  {tag} epoch {epoch}: tau {an['tau']:.3e}, pattern differs at {int(diff.sum())} elements ({int(an['near'].sum())} "
          f"near-kink), fragile {an['fragile']}")
    assert not (diff & ~an["near"]).any(), (tag, epoch, int((diff & ~an["near"]).sum()))
    errs = [(k, float(np.abs(got[k] - r64[k]).max()), K.gate(np.abs(r32[k].astype(np.float64) - r64[k]).max(), r64[k]))
            for k in ("H1d", "Z2")]
    errs.append(("loss", abs(got["loss"] - r64["loss"]), K.gate(abs(r32["loss"] - r64["loss"]), np.float64(r64["loss"]))))
    g64 = R.epoch_reference_rows(*an["args"], np.float64, relu_on=on)
    g32 = R.epoch_reference_rows(*an["args"], np.float32, relu_on=on)
    for k in R.NAMES:
        errs.append((k, float(np.abs(got[k] - g64[k]).max()), K.gate(np.abs(g32[k].astype(np.float64) - g64[k]).max(), g64[k])))
    for k, e, g in errs:
        print(f"  {tag} epoch {epoch} {k}: err_hip {e:.3e}  gate {g:.3e}  ratio {e / g:.3f}")
    for k, e, g in errs:
        assert np.isfinite(got[k]).all() and e <= g, (tag, epoch, k, e, g)
    # counts: exact off the fragile rows (a fragile row or element moves at most three cells by one)
    if tr.head == "wide":
        counts = tr.counts().cpu().numpy().astype(np.int64)
        off = int(np.abs(counts - r64["counts"]).sum())
        print(f"  {tag} epoch {epoch} counts: {off} cells off")
        assert off <= 3 * an["fragile"], (tag, epoch, off, an["fragile"])
        assert int(correct[0]) == int(counts[:, 0].sum())
        if case["loss"] == "ce":
            assert counts[:, [0, 2]].sum() == len(rows)      # every listed row is a tp or a fn of its class, no other row counts
    else:
        assert abs(int(correct[0]) - r64["correct"]) <= an["fragile"], (tag, epoch, int(correct[0]), r64["correct"])
    assert 0 <= int(correct[0]) <= len(rows) * (case["C"] if case["loss"] == "bce" else 1)


def _gate_case(c, loss, head, m):
    case = _case(c, loss, _graph_for(c))
    if case["graph"] == "hub":
        from linkteller_amd import graph
        assert graph.as_hip_graph(case["adj"]).max_row_nnz > 128
    rows = R.row_list(case["n"], m, seed=c + m)
    assert 0 in rows and (m == 1 or case["n"] - 1 in rows)
    params = _params(case, 2)
    tr = _trainer(case, params, head, rows=rows)
    assert tr.n == case["n"] and tr.n_train == m
    tag = f"{head} C={c} {loss} m={m} {case['graph']}"
    _check_epoch(case, tr, params, rows, 0, tag)
    tr.run(1)
    _check_epoch(case, tr, params, rows, 2, tag)


@pytest.mark.parametrize("m", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("c", [1, 2, 3, 8])
def test_narrow_head_against_fp64(c, m):
    _gate_case(c, "ce", "narrow", m)


@pytest.mark.parametrize("m", [1, 17, 257])
@pytest.mark.parametrize("loss", ["ce", "bce"])
@pytest.mark.parametrize("c", [9, 33, 65, 121, 256])
def test_wide_head_against_fp64(c, loss, m):
    _gate_case(c, loss, "wide", m)


# ---------------------------------------------------------------------------------------------------------------------
# what the list must and must not reach
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,loss,head", [(3, "ce", "narrow"), (33, "ce", "wide"), (9, "bce", "wide")])
def test_off_list_rows_do_not_matter(c, loss, head):
    """Every off-list row gets another label (ce) or every label bit flipped (bce): record, gradients, logits, parameters and
    counts after 2 epochs are bit-identical."""
    case = _case(c, loss)
    rows = R.row_list(case["n"], 257, seed=5)
    off = np.setdiff1d(np.arange(case["n"]), rows)
    other = case["y"].copy()
    other[off] = (other[off] + 1) % c if loss == "ce" else 1 - other[off]
    assert (other[off] != case["y"][off]).all() and np.array_equal(other[rows], case["y"][rows])
    runs = []
    for y in (case["y"], other):
        params = _params(case, 2)
        tr = _trainer(case, params, head, rows=rows, y=y)
        rec = tr.run_async(2).cpu().numpy()
        runs.append(_state(tr, params, rec))
    _same(runs[0], runs[1], (c, loss, head))
    # ... and on-list labels do: a trainer over all rows of `other` differs
    params = _params(case, 2)
    tr = _trainer(case, params, head, y=other)
    assert not np.array_equal(tr.run_async(2).cpu().numpy(), runs[0][0])


@pytest.mark.parametrize("layers,c,loss,head", [(2, 7, "ce", "narrow"), (2, 9, "bce", "wide"), (3, 41, "ce", "wide")])
def test_changing_the_list(layers, c, loss, head):
    """Dropout 0.  Trainer 1: list A, one epoch, parameters p, list B (a subset of A), one epoch.  Trainer 2: created at p with
    B, one epoch.  The gradients agree bit for bit: no row of A \\ B kept a gradient.  And a list set and cleared again leaves
    the bits of a trainer that never had one."""
    case = _case(c, loss)
    a = R.row_list(case["n"], 300, seed=7)
    b = a[::3].copy()
    p1 = _params(case, layers)
    t1 = _trainer(case, p1, head, rows=a, dropout=0.0)
    t1.run(1)
    mid = [p.clone() for p in p1]
    t1.set_train_rows(b)
    assert t1.n_train == len(b)
    rec1 = t1.run_async(1).cpu().numpy()
    t2 = _trainer(case, mid, head, rows=b, dropout=0.0)
    rec2 = t2.run_async(1).cpu().numpy()
    _same([rec1] + _host(t1.grads()) + [t1.logits().cpu().numpy()], [rec2] + _host(t2.grads()) + [t2.logits().cpu().numpy()],
          "A then B")
    assert any(g.any() for g in _host(t1.grads()))
    runs = []
    for touch in (False, True):
        params = _params(case, layers)
        tr = _trainer(case, params, head)
        if touch:
            tr.set_train_rows(a)
            tr.set_train_rows(None)
        assert tr.n_train == case["n"]
        runs.append(_state(tr, params, tr.run_async(2).cpu().numpy()))
    _same(runs[0], runs[1], "set then cleared")


@pytest.mark.parametrize("layers,head", [(2, "narrow"), (3, "wide")])
def test_refused_lists_leave_the_trainer_unchanged(layers, head):
    """Out-of-range ids, repeated ids, more ids than rows, a float dtype, two dimensions, an empty list -- through the engine
    and through the C entry point itself: each is refused, and the next epoch equals the epoch of an untouched twin (both keep
    the list they had)."""
    from linkteller_amd import _lib
    case = _case(7 if head == "narrow" else 41, "ce")
    n = case["n"]
    rows = R.row_list(n, 257, seed=3)
    pa, pb = _params(case, layers), _params(case, layers)
    tr, twin = _trainer(case, pa, head, rows=rows), _trainer(case, pb, head, rows=rows)
    lib = _lib.lib()
    fn = getattr(lib, f"lt_gcn{layers}_trainer_set_train_rows")
    stream = torch.cuda.current_stream().cuda_stream

    def raw(ids, m=None):
        host = np.ascontiguousarray(ids, dtype=np.int32)
        return fn(tr._h, host.ctypes.data_as(C.c_void_p), len(host) if m is None else m, stream)

    def step(tag):
        assert tr.n_train == 257
        ra, rb = tr.run_async(1).cpu().numpy(), twin.run_async(1).cpu().numpy()
        _same(_state(tr, pa, ra), _state(twin, pb, rb), tag)

    outside = rows.copy()
    outside[[10, 200]] = [n, -1]
    with pytest.raises(IndexError, match="2 ids outside the graph"):
        tr.set_train_rows(outside)
    step("outside")
    repeated = rows.copy()
    repeated[[5, 6, 256]] = rows[0]
    with pytest.raises(ValueError, match="3 ids repeat"):
        tr.set_train_rows(repeated)
    step("repeated")
    with pytest.raises(ValueError, match="repeat"):
        tr.set_train_rows(np.concatenate([np.arange(n), [0]]))            # m > n: in range, so one id repeats
    for bad in (rows.astype(np.float32), torch.tensor(rows, dtype=torch.float64), rows.reshape(1, -1), np.zeros(0, np.int64)):
        with pytest.raises(ValueError):
            tr.set_train_rows(bad)
    step("dtype, shape, empty")
    # the library checks the host list itself and names the first offender
    assert raw(outside) == INVALID and f"rows[10]={n} outside [0, {n})" in lib.lt_last_error().decode()
    assert raw(repeated) == INVALID and f"rows[5]={rows[0]} repeats" in lib.lt_last_error().decode()
    assert raw(np.concatenate([np.arange(n), [0]])) == INVALID and f"m={n + 1}" in lib.lt_last_error().decode()
    assert raw(rows, m=-1) == INVALID and "m=-1" in lib.lt_last_error().decode()
    assert fn(tr._h, None, 5, stream) == INVALID
    step("C ABI")
    # accepted forms: a tensor of another integer dtype, a list
    tr.set_train_rows(torch.tensor(rows, dtype=torch.int16))
    step("int16 tensor")
    tr.set_train_rows([int(r) for r in rows])
    step("python list")


@pytest.mark.parametrize("c,loss,head", [(7, "ce", "narrow"), (9, "bce", "wide")])
def test_run_validated_with_a_training_list(c, loss, head):
    """Training rows and a disjoint validation list on the same graph: every epoch's val_loss / val_counts are the evaluation
    head's over the validation rows of val_logits(), the train record is the record of the same trainer without validation,
    and restore_best puts back the parameters of the best epoch."""
    from linkteller_amd import engine
    case = _case(c, loss)
    perm = np.random.RandomState(11).permutation(case["n"])
    tr_rows, va_rows = perm[:257], perm[257:400]
    x, y = _dev(case["x"]), _dev(case["y"])
    params = _params(case, 2)
    tr = _trainer(case, params, head, rows=tr_rows, lr=0.2)
    tr.attach_validation(case["adj"], x, y, keep_best=True, rows=va_rows)
    plain_p = _params(case, 2)
    plain = _trainer(case, plain_p, head, rows=tr_rows, lr=0.2)
    models, losses = [], []
    for e in range(6):
        r = tr.run_validated(1)
        models.append(_host(params))
        if head == "wide":
            want_loss, want_counts = engine.eval_head_wide(tr.val_logits(), y, rows=va_rows, loss=loss)
        else:
            want_loss, want_counts = engine.eval_head(tr.val_logits(), y, rows=va_rows)
        assert r["val_loss"].view(np.int32)[0] == int(want_loss.view(torch.int32).cpu()), e
        assert np.array_equal(r["val_counts"][0], want_counts.cpu().numpy()), e
        rec = plain.run_async(1).cpu().numpy()
        assert np.float32(rec[0, 0]) == r["loss"][0] and int(rec[0, 1]) == r["correct"][0], e
        losses.append(float(r["val_loss"][0]))
    _same(_host(params), _host(plain_p), "validation does not touch the training")
    best = tr.val_state()["best_epoch"]
    assert best == int(np.argmin(losses)) or losses[best] == min(losses)
    tr.restore_best()
    _same(_host(params), models[best], "restore_best")


# ---------------------------------------------------------------------------------------------------------------------
# main --train-setting transductive
# ---------------------------------------------------------------------------------------------------------------------
N_FULL, NF, N_TR = 300, 24, 150


def _fixture(root, name):
    """300 nodes, F = 24, mean degree 6, split 50 / 25 / 25, learnable: flickr with 7 classes, ppi with 121 labels per node."""
    from linkteller_amd import synth
    rng = np.random.RandomState(31)
    adj = synth.erdos_renyi_graph(N_FULL, 900, seed=32).astype(np.float64)
    if name == "ppi":
        proto = rng.randint(0, 6, N_FULL)
        y = (rng.uniform(size=(6, 121)) < 0.3)[proto].astype(np.int64)
        centres = rng.standard_normal((6, NF))
    else:
        proto = y = rng.randint(0, 7, N_FULL)
        centres = rng.standard_normal((7, NF))
    feats = centres[proto] * 1.5 + rng.standard_normal((N_FULL, NF))
    perm = rng.permutation(N_FULL)
    roles = {"tr": perm[:N_TR].tolist(), "va": perm[N_TR:225].tolist(), "te": perm[225:].tolist()}
    synth.write_graphsaint_dataset(str(root), name, adj, feats, y, roles)


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


@pytest.mark.parametrize("name,extra", [("flickr", ""), ("ppi", "--train-head wide")])
def test_main_transductive(name, extra, tmp_path, monkeypatch, capsys):
    data = tmp_path / "data"
    _fixture(data, name)
    common = f"--dataset {name} --hidden 16 --norm FirstOrderGCN"
    tr = _run_main(tmp_path / "run", data, monkeypatch,
                   f"{common} --train --train-setting transductive --early --patience 5 --num-epochs 30 {extra}".split())
    gt, w = tr.gpu_trainer, tr.worker
    assert gt.n == N_FULL == w.n_nodes and gt.n_train == N_TR == len(w.idx_train)
    assert gt.head == ("wide" if extra else "narrow") and gt.n2 == N_FULL
    logs = glob.glob(str(tmp_path / "run" / f"logs_{name}" / "*.log"))
    models = glob.glob(str(tmp_path / "run" / f"model_{name}" / "*" / "model.pt"))
    assert len(logs) == 1 and len(models) == 1
    log = open(logs[0]).read()
    acc = [float(v) for v in re.findall(r"'acc_train: ([0-9.]+)'", log)]
    state = gt.val_state()
    ran = state["stop_epoch"] + 1 if state["stop_epoch"] >= 0 else 30
    assert len(acc) == ran >= 1 and all(0.0 <= v <= 1.0 for v in acc), acc
    assert len(re.findall(r"'loss_val: ([0-9.]+)'", log)) == ran
    if not extra:      # single label: the last epochs classify most of the 150 listed rows (an all-rows divisor would halve it)
        assert max(acc) > 0.5, acc
    sd = torch.load(models[0], map_location="cpu")
    assert sorted(sd) == ["gc1.bias", "gc1.weight", "gc2.bias", "gc2.weight"] and sd["gc1.weight"].shape == (NF, 16)
    assert all(bool(torch.isfinite(t).all()) for t in sd.values())
    capsys.readouterr()
    _run_main(tmp_path / "attack", data, monkeypatch,
              f"{common} --test --model-path {models[0]} --attack --attack-mode efficient --sample-type unbalanced --n-test 40".split())
    out = capsys.readouterr().out
    assert f"attack results saved to: eval_{name}/efficient_unbalanced_40_42.pt" in out and "Test set results" in out

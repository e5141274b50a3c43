"""CPU checks of the minibatch MLP baselines: the numpy restatement (mlp_restate.py) against torch fp64 autograd, the Philox
shuffle, the ``order="torch"`` law against a DataLoader, the host mirrors against the reference's initial parameters
(golden/mlp_train.npz), main_simple's refusals, and the library's exports."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mlp_cases as K
import mlp_restate as M
import train_restate as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_train.npz")


def _torch_step(x, y, params, rows, depth, loss, keep, scale):
    """Two plainly written affine layers under torch fp64 autograd."""
    ps = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in params]
    xb = torch.tensor(x[rows], dtype=torch.float64)
    if depth == 2:
        h = torch.relu(xb @ ps[0] + ps[1])
        if keep is not None:
            h = h * torch.tensor(keep, dtype=torch.float64) * float(scale)
        z = h @ ps[2] + ps[3]
    else:
        z = xb @ ps[0] + ps[1]
    if loss == "ce":
        lt = F.cross_entropy(z, torch.tensor(y[rows], dtype=torch.int64))
    else:
        lt = F.binary_cross_entropy_with_logits(z, torch.tensor(y[rows], dtype=torch.float64))
    lt.backward()
    return z.detach().numpy(), float(lt.detach()), [p.grad.numpy() for p in ps]


@pytest.mark.parametrize("name,step", [("D", 0), ("D", 4), ("K", 0), ("E", 2), ("F", 2), ("G", 2), ("H", 0), ("B", 2)])
def test_restatement_equals_torch_autograd(name, step):
    """Gather, both depths, CE and BCE, the step's Philox mask, short last batches (D-4: 2 rows, B-2: 1 row)."""
    case = K.make(name)
    rows = K.batch_of(case, step)
    keep, scale = None, 1.0
    if case["depth"] == 2 and case["p"] > 0:
        keep, scale = M.step_keep(rows.size, case["H"], step, K.SEED, case["p"]), float(T.dropout_scale(case["p"]))
        assert 0 < keep.mean() < 1
    ref = M.step_reference(case["x"], case["y"], case["params"], rows, case["depth"], case["loss"], keep, scale)
    z, lt, grads = _torch_step(case["x"], case["y"], case["params"], rows, case["depth"], case["loss"], keep, scale)
    assert np.abs(ref["Z"] - z).max() <= 1e-12 * max(1.0, np.abs(z).max())
    assert abs(ref["loss"] - lt) <= 1e-12
    assert len(grads) == len(ref["grads"])
    for a, b in zip(ref["grads"], grads):
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    if case["loss"] == "ce":
        assert ref["count"] == int((z.argmax(1) == case["y"][rows]).sum())
    else:
        assert ref["count"] == int(((z > 0) & (case["y"][rows] != 0)).sum())


def test_epoch_restatement_follows_torch_adam():
    """One epoch of case D without dropout: fp64 gradients at the fp32 parameters, Adam in fp32 -- against the same loop under
    torch (autograd in fp64, optim.Adam on the fp32 parameters): the first loss to 1e-12, the later ones to 1e-6 of their size
    (a last-bit difference in a parameter moves the loss by about 1e-7 of it), the parameters to 2 ulp of their size."""
    case = K.make("D")
    state = M.State(case["params"])
    losses, counts = M.run_epoch(state, case["x"], case["y"], case["orders"][0], 2, case["B"], K.LR, K.DECAY)
    assert len(losses) == case["spe"] == 5 and state.step == 5 and M.batches(case["orders"][0], case["B"])[-1].size == 2
    ps = [torch.tensor(p.copy(), requires_grad=True) for p in case["params"]]
    opt = torch.optim.Adam(ps, lr=K.LR, weight_decay=K.DECAY)
    for k, rows in enumerate(M.batches(case["orders"][0], case["B"])):
        _, lt, grads = _torch_step(case["x"], case["y"], [p.detach().numpy() for p in ps], rows, 2, "ce", None, 1.0)
        # step 0 starts from the same parameters; later steps from parameters that may differ in their last bit
        assert abs(lt - losses[k]) <= (1e-12 if k == 0 else 1e-6 * abs(lt))
        for p, g in zip(ps, grads):
            p.grad = torch.tensor(g.astype(np.float32))
        opt.step()
    for a, b in zip(state.params, ps):
        assert np.abs(a - b.detach().numpy()).max() <= 2.4e-7 * np.abs(a).max()


@pytest.mark.parametrize("n", [1, 2, 257])
def test_shuffle_restatement_is_a_permutation(n):
    o0, o1 = M.shuffle_order(n, 0, K.SEED), M.shuffle_order(n, 1, K.SEED)
    assert np.array_equal(np.sort(o0), np.arange(n)) and np.array_equal(np.sort(o1), np.arange(n))
    assert np.array_equal(o0, M.shuffle_order(n, 0, K.SEED))
    if n > 2:
        assert not np.array_equal(o0, o1) and not np.array_equal(o0, np.arange(n))
        assert not np.array_equal(o0, M.shuffle_order(n, 0, K.SEED + 1))


def test_torch_order_is_the_dataloaders():
    """``order="torch"`` (engine.torch_epoch_orders) under a seed = the batches DataLoader(shuffle=True) yields under it."""
    from torch.utils.data import DataLoader, TensorDataset
    from linkteller_amd.engine import torch_epoch_orders
    n, bsz = 300, 64
    torch.manual_seed(1234)
    orders = torch_epoch_orders(n, 3).numpy()
    torch.manual_seed(1234)
    loader = DataLoader(TensorDataset(torch.arange(n)), batch_size=bsz, shuffle=True)
    for e in range(3):
        want = [b[0].numpy() for b in loader]
        got = M.batches(orders[e], bsz)
        assert len(got) == len(want) == 5 and got[-1].size == 44
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert not np.array_equal(orders[0], orders[1])


@pytest.mark.parametrize("key,depth,h,c", [("d2.h16", 2, 16, 2), ("d2.h64", 2, 64, 2), ("d2.h16.ml5", 2, 16, 5), ("d1", 1, 0, 2)])
def test_host_mirrors_start_where_the_reference_starts(key, depth, h, c):
    """A seed gives the reference's initial parameters: same key names, [out, in] shapes and values (depth 2 carries the
    reference's unused W layer); project_params / load_project_params round-trip; autograd is refused."""
    from linkteller_amd.gcn import OneLayerMLP, SingleHiddenLayerMLP
    g = np.load(GOLDEN)
    torch.manual_seed(42)
    model = OneLayerMLP(nfeat=160, nclass=c) if depth == 1 else SingleHiddenLayerMLP(nfeat=160, nhid=h, nclass=c, dropout=0.0)
    sd = model.state_dict()
    want = sorted(k[len(key) + 6:] for k in g.files if k.startswith(key + ".init."))
    assert sorted(sd) == want == (["W.bias", "W.weight"] if depth == 1 else
                                  ["W.bias", "W.weight", "W1.bias", "W1.weight", "W2.bias", "W2.weight"])
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), g[f"{key}.init.{k}"]), k
    ps = model.project_params()
    assert [tuple(p.shape) for p in ps] == ([(160, c), (c,)] if depth == 1 else [(160, h), (h,), (h, c), (c,)])
    model.load_project_params([p + 1 for p in ps])
    assert all(torch.equal(a, b + 1) for a, b in zip(model.project_params(), ps))
    with pytest.raises(NotImplementedError):
        model.train()(torch.zeros(3, 160))


@pytest.mark.parametrize("argv,exc", [
    (["--mode", "sgc", "--dataset", "twitch/ES/RU"], NotImplementedError),
    (["--dataset", "twitch/ES/RU"], NotImplementedError),                                   # the reference's default mode
    (["--mode", "mlp", "--depth", "3", "--dataset", "twitch/ES/RU", "--batch"], NotImplementedError),
    (["--mode", "mlp", "--trainer-type", "dp_mlp", "--dataset", "twitch/ES/RU", "--batch"], NotImplementedError),
    (["--mode", "mlp", "--dataset", "flickr"], NotImplementedError),                        # full batch on a split dataset
    (["--mode", "mlp", "--batch"], NotImplementedError),                                    # the reference's default dataset, cora
    (["--mode", "mlp", "--dataset", "wikipedia/chameleon", "--batch"], NotImplementedError),   # a transfer family that is not read
    (["--mode", "mlp", "--dataset", "twitch-train/ES", "--batch"], NotImplementedError),
    (["--mode", "mlp", "--dataset", "deezer", "--test", "--model-path", "model.pt"], NotImplementedError),
    (["--mode", "mlp", "--dataset", "twitch/ES/RU", "--test"], ValueError),                 # no model path
    (["--mode", "mlp", "--dataset", "twitch/ES/RU", "--batch", "--batch-size", "0"], ValueError),
    (["--mode", "mlp", "--depth", "2", "--hidden", "300", "--dataset", "twitch/ES/RU", "--batch"], NotImplementedError),
])
def test_main_simple_refuses_before_any_file_is_read(argv, exc, tmp_path, monkeypatch):
    from linkteller_amd import main_simple
    monkeypatch.chdir(tmp_path)
    with pytest.raises(exc):
        main_simple.main(argv + ["--data-root", str(tmp_path / "nowhere")])
    assert os.listdir(tmp_path) == []      # no log or model directory either


def test_main_simple_takes_the_reference_flags():
    from linkteller_amd import main_simple
    a = main_simple.get_arguments([])
    assert (a.lr, a.weight_decay, a.depth, a.batch_size, a.mode, a.patience, a.dropout) == (0.2, 5e-6, 1, 256, "sgc", 50, 0.5)
    a = main_simple.get_arguments("--mode mlp --depth 2 --batch --batch-size 64 --early --num-epochs 3".split())
    assert a.batch and a.early and a.batch_size == 64 and a.num_epochs == 3 and a.assign_seed == 42


def test_library_exports_the_mlp_entry_points():
    from linkteller_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("lt_mlp_trainer_create", "lt_mlp_trainer_run", "lt_mlp_trainer_step", "lt_mlp_trainer_grads",
                 "lt_mlp_trainer_logits", "lt_mlp_trainer_counts", "lt_mlp_trainer_order", "lt_mlp_trainer_destroy",
                 "lt_mlp_forward", "lt_mlp_forward_workspace_bytes"):
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES


def test_graphsaint_reader_without_the_adjacency(tmp_path):
    """``read_graphsaint(with_adj=False)`` -- what ``worker.FeatureData`` calls -- opens no edge file: it gives the same features,
    labels and split with ``adj_full.npz`` deleted."""
    from linkteller_amd import synth
    from linkteller_amd.worker import FeatureData, read_graphsaint
    rng = np.random.RandomState(0)
    adj = synth.erdos_renyi_graph(40, 80, seed=1).astype(np.float64)
    perm = rng.permutation(40)
    synth.write_graphsaint_dataset(str(tmp_path), "flickr", adj, rng.standard_normal((40, 6)), rng.randint(0, 3, 40),
                                   {"tr": perm[:20].tolist(), "va": perm[20:30].tolist(), "te": perm[30:].tolist()})
    full = read_graphsaint(str(tmp_path / "flickr"))
    os.remove(tmp_path / "flickr" / "adj_full.npz")
    bare = read_graphsaint(str(tmp_path / "flickr"), with_adj=False)
    assert full[6] is not None and bare[6] is None
    for a, b in zip(full[:6], bare[:6]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    w = FeatureData("flickr", data_root=str(tmp_path))
    assert (w.n_nodes, w.n_features, w.multi_label, w.n_classes, w.transfer) == (40, 6, 1, 3, False)


def test_rare_class_f1_is_sklearns():
    """metrics.rare_class_f1 (shared by GCNTrainer and MLPTrainer) against sklearn with the minority class as pos_label, for
    either class being the rare one; a bare 0, as the reference, when nothing is predicted rare."""
    from sklearn.metrics import average_precision_score, f1_score, precision_score, recall_score
    from linkteller_amd.metrics import rare_class_f1
    rng = np.random.RandomState(5)
    for rare in (0, 1):
        y = (rng.random_sample(200) < (0.3 if rare == 1 else 0.7)).astype(np.int64)
        z = torch.tensor(rng.standard_normal((200, 2)) + 0.8 * np.eye(2)[y])
        got = rare_class_f1(z, torch.tensor(y))
        pred = z.argmax(1).numpy()
        want = (f1_score(y, pred, pos_label=rare), precision_score(y, pred, pos_label=rare), recall_score(y, pred, pos_label=rare),
                average_precision_score(y if rare == 1 else 1 - y, torch.softmax(z, 1).max(1)[0].numpy()))
        assert int((y == rare).sum()) < 100 and all(abs(a - b) <= 1e-12 for a, b in zip(got, want)), (got, want)
    z, y = torch.tensor([[5.0, 0.0]] * 4), torch.tensor([0, 0, 0, 1])
    assert rare_class_f1(z, y) == 0                                  # nothing predicted rare: the reference's bare 0 ...
    got = rare_class_f1(z, y, bare_zero=False)                       # ... or zeros and the AP
    assert got[:3] == (0.0, 0.0, 0.0) and abs(got[3] - average_precision_score(y.numpy(), [1 / (1 + np.exp(-5.0))] * 4)) <= 1e-12
    z = torch.tensor([[0.0, 5.0], [5.0, 0.0], [5.0, 0.0], [5.0, 0.0]])      # one row predicted rare, and it is not
    got = rare_class_f1(z, y)
    assert got[:3] == (0.0, 0.0, 0.0) and got[:3] == (f1_score(y, [1, 0, 0, 0]), precision_score(y, [1, 0, 0, 0]), recall_score(y, [1, 0, 0, 0]))

"""Training of the 3-layer GCN, the parts that need no GPU: the written-out epoch (train3_restate.epoch_reference3) against
torch's fp64 autograd, the per-layer dropout mask, the conditions of the cases of test_train3_backward_gpu.py, the refusals
of engine.GCN3Trainer and GCNTrainer.init_model without a GPU, GCN3's init law against the reference's."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
import train_restate as T
import train3_cases as K3
import train3_restate as T3


def _autograd3(adj, x, y, params, keep1, keep2, scale):
    """fp64 autograd on the dense adjacency with the same masks."""
    import torch.nn.functional as F
    a = torch.from_numpy(np.asarray(adj.todense(), dtype=np.float64))
    ps = [torch.from_numpy(np.asarray(p, dtype=np.float64)).requires_grad_() for p in params]
    w1, b1, w2, b2, w3, b3 = ps
    d1 = torch.from_numpy(keep1.astype(np.float64) * float(scale))
    d2 = torch.from_numpy(keep2.astype(np.float64) * float(scale))
    h1 = torch.relu(a @ (torch.from_numpy(x).double() @ w1) + b1) * d1
    h2 = torch.relu(a @ (h1 @ w2) + b2) * d2
    z = a @ (h2 @ w3) + b3
    loss = F.cross_entropy(z, torch.from_numpy(y))
    loss.backward()
    return dict(Z3=z.detach().numpy(), loss=float(loss.detach()), **{k: p.grad.numpy() for k, p in zip(T3.NAMES3, ps)})


def test_epoch_reference3_against_autograd():
    """Case B3 (both masks on, pad widths, three classes): all six gradients within 1e-12 of each tensor's largest magnitude,
    the loss within 1e-12."""
    torch.set_num_threads(1)
    case = K3.make("B3")
    keep1, keep2 = K3.masks(case, 0)
    scale = T.dropout_scale(case["p"])
    got = T3.epoch_reference3(case["adj"], case["x"], case["y"], case["params"], keep1, keep2, scale, np.float64)
    ref = _autograd3(case["adj"], case["x"], case["y"], case["params"], keep1, keep2, scale)
    for k in T3.NAMES3 + ("Z3",):
        err, top = np.abs(got[k] - ref[k]).max(), np.abs(ref[k]).max()
        assert got[k].dtype == np.float64 and top > 0 and err <= 1e-12 * top, (k, err, top)
    assert abs(got["loss"] - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    # on1 / on2 reach the gradients only: the forward does not depend on them
    other = T3.epoch_reference3(case["adj"], case["x"], case["y"], case["params"], keep1, keep2, scale, np.float64,
                                on1=np.ones_like(keep1), on2=got["Z2"] > 0)
    assert all(np.array_equal(got[k], other[k]) for k in ("Z1", "Z2", "Z3", "H1d", "H2d", "dW2", "db2", "dW3", "db3"))
    assert not np.array_equal(got["dW1"], other["dW1"])


@pytest.mark.parametrize("p", [0.3, 0.5])
def test_dropout_mask_layers(p):
    n, h, epoch, seed = 211, 30, 3, K3.SEED
    k0, k1 = T3.dropout_keep3(n, h, epoch, seed, p, 0), T3.dropout_keep3(n, h, epoch, seed, p, 1)
    assert np.array_equal(k0, T.dropout_keep(n, h, epoch, seed, p))
    assert not np.array_equal(k0, k1)                     # the layer word: two masks at H1 = H2
    sigma = np.sqrt(p * (1 - p) / (n * h))
    for k in (k0, k1):
        assert abs(k.mean() - (1 - p)) <= 3 * sigma, (k.mean(), p, sigma)
    assert abs((k0 == k1).mean() - (p * p + (1 - p) ** 2)) <= 4 * sigma      # independent, not complementary or shifted
    for layer in (0, 1):
        assert T3.dropout_keep3(n, h, epoch, seed, 0.0, layer).all()
        assert not T3.dropout_keep3(n, h, epoch, seed, 1.0, layer).any()
    # the counter layout, element by element
    t = np.uint64(int(np.floor(p * 2 ** 32)))
    for r, j in [(0, 0), (1, 1), (n - 1, h - 1), (11, 2)]:
        i = r * h + j
        w = T.philox4x32_10(np.array([[(i >> 2) & 0xFFFFFFFF, (i >> 2) >> 32, epoch, 1]], dtype=np.uint64),
                            np.array([[seed & 0xFFFFFFFF, seed >> 32]], dtype=np.uint64))[0]
        assert k1[r, j] == (np.uint64(w[i & 3]) >= t)


def _advance(case, epochs):
    """The parameters after ``epochs`` epochs of the fp32 epoch_reference3 gradients under train_restate.adam_step."""
    sizes = [a.size for a in case["params"]]
    shapes = [a.shape for a in case["params"]]
    p = np.concatenate([a.ravel() for a in case["params"]]).astype(np.float32)
    m, v = np.zeros_like(p), np.zeros_like(p)
    scale = T.dropout_scale(case["p"])
    for e in range(epochs):
        cur = [a.reshape(s) for a, s in zip(np.split(p, np.cumsum(sizes)[:-1]), shapes)]
        keep1, keep2 = K3.masks(case, e)
        r = T3.epoch_reference3(case["adj"], case["x"], case["y"], cur, keep1, keep2, scale, np.float32)
        g = np.concatenate([r[k].ravel() for k in T3.NAMES3]).astype(np.float32)
        p, m, v = T.adam_step(p, g, m, v, e + 1, K3.LR, weight_decay=K3.DECAY)
    return [a.reshape(s) for a, s in zip(np.split(p, np.cumsum(sizes)[:-1]), shapes)]


@pytest.mark.parametrize("name,epoch", K3.CASE_EPOCHS, ids=[f"{k}-epoch{e}" for k, e in K3.CASE_EPOCHS])
def test_backward_case_conditions(name, epoch):
    """What test_train3_backward_gpu.py relies on, at every checked epoch: per hidden layer the near-kink elements are at
    most 0.1 % of the kept ones and no row has a fragile argmax; and what each case is there to reach is really in it."""
    torch.set_num_threads(1)
    case = K3.make(name)
    n, f, h1, h2, c, p, _ = K3.SHAPES[name]
    shapes = [(f, h1), (h1,), (h1, h2), (h2,), (h2, c), (c,)]
    assert [a.shape for a in case["params"]] == shapes and all(a.dtype == np.float32 for a in case["params"])
    assert case["x"].shape == (n, f) and int(case["y"].max()) == c - 1
    an = K3.analyse(case, _advance(case, epoch), epoch)
    K3.check_conditions(case, an)
    assert an["r32"]["dW1"].dtype == np.float32
    rows = np.diff(case["adj"].indptr)
    if name == "A3":
        assert rows.max() > 128 and np.diff(case["adj"].tocsc().indptr).max() > 128
    if name == "D3":
        assert rows.min() == 0 and (case["adj"] != case["adj"].T).nnz > 0 and h2 > h1 and h2 == 256 and p == 0
    if name in ("B3", "E3"):
        assert h1 % 4 and h2 % 4 and h1 % 32 and h2 % 16
    if name == "G3":
        assert h2 % 32 and c == 2
    if name == "E3":
        r = an["r64"]
        assert all(not r[k].any() for k in T3.NAMES3[:5]) and np.abs(r["db3"]).max() > 0
        assert np.array_equal(r["Z3"], np.broadcast_to(case["params"][5].astype(np.float64), r["Z3"].shape))
    if name == "C3":
        r = an["r64"]
        assert r["loss"] == 0 and all(not r[k].any() for k in T3.NAMES3)


def test_trainer3_refuses_bad_dropout_and_no_gpu():
    from linkteller_amd import _lib, engine
    import scipy.sparse as sp
    z = torch.zeros
    args = (sp.identity(4, format="csr"), z(4, 3), [0, 1, 0, 1], z(3, 2), z(2), z(2, 2), z(2), z(2, 2), z(2))
    with pytest.raises(ValueError):
        engine.GCN3Trainer(*args, lr=0.01, weight_decay=0.0, dropout=1.5, seed=0)
    if torch.cuda.is_available():
        return
    with pytest.raises(_lib.LinkTellerHipError):
        engine.GCN3Trainer(*args, lr=0.01, weight_decay=0.0, dropout=0.5, seed=0)


def test_init_model_three_layers_reaches_the_trainer():
    """GCNTrainer.init_model() with n_layer = 3 and no model path builds GCN3 and goes on to the GPU trainer's constructor:
    without a GPU that is LinkTellerHipError, not the NotImplementedError of a trainer that stops at two layers."""
    import scipy.sparse as sp
    from linkteller_amd import _lib
    from linkteller_amd.gcn import GCN3
    from linkteller_amd.trainer import GCNTrainer
    n, f = 6, 5
    worker = types.SimpleNamespace(mode="vanilla-clean", dataset="twitch/ES/RU", n_features=f, n_classes=2, transfer=True,
                                   adj_1=sp.identity(n, format="csr"), features_1=torch.zeros(n, f),
                                   labels_1=torch.zeros(n, dtype=torch.int64))
    args = types.SimpleNamespace(n_layer=3, hidden=16, hidden1=8, hidden2=4, dropout=0.5, lr=0.01, weight_decay=5e-4, seed=1)
    tr = GCNTrainer(args, subdir="", worker=worker)
    if torch.cuda.is_available():
        worker.features_1, worker.labels_1 = worker.features_1.cuda(), worker.labels_1.cuda()
        tr.init_model()
        assert type(tr.gpu_trainer).__name__ == "GCN3Trainer"
    else:
        with pytest.raises(_lib.LinkTellerHipError):
            tr.init_model()
    assert isinstance(tr.model, GCN3)
    assert [tuple(p.shape) for p in tr.model.parameters()] == [(f, 8), (8,), (8, 4), (4,), (4, 2), (2,)]


@pytest.mark.parametrize("h1,h2", [(16, 16), (64, 32)])
def test_init_law_matches_reference(h1, h2):
    from linkteller_amd.gcn import GCN3
    g, g2 = load_golden("train3.npz"), load_golden("train.npz")
    torch.manual_seed(42)
    model = GCN3(nfeat=g2["x1"].shape[1], nhid1=h1, nhid2=h2, nclass=2, dropout=0.5)
    sd = model.state_dict()
    assert sorted(sd) == ["gc1.bias", "gc1.weight", "gc2.bias", "gc2.weight", "gc3.bias", "gc3.weight"]
    for name, p in sd.items():
        assert np.array_equal(p.numpy(), g[f"FirstOrderGCN.h{h1}_{h2}.init.{name}"]), name

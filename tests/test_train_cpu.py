"""GPU training, the parts that need no GPU: the dropout mask's Philox4x32-10 restatement, the fp32 Adam op order against
torch.optim.Adam, the --train switch of the command line, the model's init law against the reference's."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import train_restate as T


def test_philox_known_answers():
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
              "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in cases:
        got = T.philox4x32_10(np.array([ctr], dtype=np.uint64), np.array([key], dtype=np.uint64))[0]
        assert " ".join(f"{w:08x}" for w in got) == want


@pytest.mark.parametrize("h", [16, 7])
def test_dropout_mask_counter_layout(h):
    n, epoch, seed, p = 23, 5, (3 << 32) | 42, 0.5
    keep = T.dropout_keep(n, h, epoch, seed, p)
    t = np.uint64(int(np.floor(p * 2 ** 32)))
    for r, j in [(0, 0), (0, 3), (1, 1), (7, h - 1), (n - 1, h - 1), (11, 2)]:
        i = r * h + j
        q = i >> 2
        w = T.philox4x32_10(np.array([[q & 0xFFFFFFFF, q >> 32, epoch, 0]], dtype=np.uint64),
                            np.array([[seed & 0xFFFFFFFF, seed >> 32]], dtype=np.uint64))[0]
        assert keep[r, j] == (np.uint64(w[i & 3]) >= t)
    assert 0.35 < keep.mean() < 0.65
    assert not np.array_equal(keep, T.dropout_keep(n, h, epoch + 1, seed, p))    # the epoch is part of the counter
    assert T.dropout_keep(n, h, epoch, seed, 0.0).all()
    assert not T.dropout_keep(n, h, epoch, seed, 1.0).any()


def _autograd(adj, x, y, params, keep, scale, dtype):
    """The form of test_train_gpu._autograd, with the forward values returned as well."""
    import torch.nn.functional as F
    coo = adj.tocoo()
    a = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]), coo.data.astype(np.float64), adj.shape).to(dtype).coalesce()
    ps = [torch.from_numpy(np.asarray(p, dtype=np.float64)).to(dtype).requires_grad_() for p in params]
    w1, b1, w2, b2 = ps
    xt = torch.from_numpy(x).to(dtype)
    z1 = torch.sparse.mm(a, xt @ w1) + b1
    h = torch.relu(z1) * torch.from_numpy(keep.astype(np.float64) * float(scale)).to(dtype)
    z = torch.sparse.mm(a, h @ w2) + b2
    loss = F.cross_entropy(z, torch.from_numpy(y))
    loss.backward()
    return dict(Z1=z1.detach().numpy(), Z2=z.detach().numpy(), loss=float(loss.detach()),
                **{k: p.grad.numpy() for k, p in zip(("dW1", "db1", "dW2", "db2"), ps)})


@pytest.mark.parametrize("name", ["B", "D"])
def test_epoch_reference_against_autograd(name):
    """The written-out fp64 epoch (train_restate.epoch_reference) against torch's fp64 autograd: 1e-12 of each tensor's
    largest magnitude.  B has dropout, three classes and a symmetric graph; D a directed weighted graph with empty rows and
    columns, where A^T is not A."""
    import train_cases as K
    torch.set_num_threads(1)
    case = K.make(name)
    keep = T.dropout_keep(case["n"], case["H"], 0, K.SEED, case["p"])
    scale = T.dropout_scale(case["p"])
    got = T.epoch_reference(case["adj"], case["x"], case["y"], case["params"], keep, scale, np.float64)
    ref = _autograd(case["adj"], case["x"], case["y"], case["params"], keep, scale, torch.float64)
    for k in ("Z1", "Z2", "dW1", "db1", "dW2", "db2"):
        err, top = np.abs(got[k] - ref[k]).max(), np.abs(ref[k]).max()
        assert got[k].dtype == np.float64 and top > 0 and err <= 1e-12 * top, (k, err, top)
    assert abs(got["loss"] - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    assert np.array_equal(got["argmax"], ref["Z2"].argmax(axis=1))
    if name == "D":
        a = case["adj"]
        assert (np.diff(a.indptr) == 0).any() and (np.diff(a.tocsc().indptr) == 0).any() and (a != a.T).nnz > 0


def test_epoch_reference_relu_argument_and_extremes():
    """relu_on reaches dW1 and db1 only, and only the columns it changes; a single class gives a zero loss and zero
    gradients; p = 1 gives zero dW1, db1, dW2 and logits equal to b2."""
    import train_cases as K
    case = K.make("F")
    keep = T.dropout_keep(case["n"], case["H"], 0, K.SEED, case["p"])
    args = (case["adj"], case["x"], case["y"], case["params"], keep, T.dropout_scale(case["p"]), np.float64)
    base = T.epoch_reference(*args)
    on = base["Z1"] > 0
    flip = on.copy()
    r, h = np.argwhere(keep)[0]
    flip[r, h] = ~flip[r, h]
    other = T.epoch_reference(*args, relu_on=flip)
    for k in ("Z1", "Z2", "dW2", "db2"):
        assert np.array_equal(base[k], other[k])
    cols = np.arange(case["H"]) != h
    assert np.array_equal(base["dW1"][:, cols], other["dW1"][:, cols]) and np.array_equal(base["db1"][cols], other["db1"][cols])
    assert base["db1"][h] != other["db1"][h] and not np.array_equal(base["dW1"][:, h], other["dW1"][:, h])
    assert np.array_equal(T.epoch_reference(*args, relu_on=on)["dW1"], base["dW1"])
    c = K.make("C")
    keep = T.dropout_keep(c["n"], c["H"], 0, K.SEED, c["p"])
    one = T.epoch_reference(c["adj"], c["x"], c["y"], c["params"], keep, T.dropout_scale(c["p"]), np.float64)
    assert one["loss"] == 0 and all(not one[k].any() for k in K.NAMES) and np.abs(one["Z2"]).max() > 0
    e = K.make("E")
    none = T.epoch_reference(e["adj"], e["x"], e["y"], e["params"], np.zeros((e["n"], e["H"]), bool), T.dropout_scale(1.0),
                             np.float64)
    assert all(not none[k].any() for k in ("dW1", "db1", "dW2")) and np.abs(none["db2"]).max() > 0
    assert np.array_equal(none["Z2"], np.broadcast_to(e["params"][3].astype(np.float64), none["Z2"].shape))


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "F", "T"])
def test_backward_case_conditions(name):
    """What test_train_backward_gpu.py relies on, at the initial parameters: hidden columns with near-kink elements (kept
    pre-activations within tau = 8 max|Z1_fp32 - Z1_fp64| of 0) are at most 1/8 of H, rows with a top-2 logit margin below
    1e-4 at most 1 % of n; and what each case is there to reach is really in it."""
    import train_cases as K
    from linkteller_amd import graph
    case = K.make(name)
    n, f, h, c, p, _ = K.SHAPES[name]
    assert case["x"].shape == (n, f) and case["params"][0].shape == (f, h) and case["params"][2].shape == (h, c)
    assert int(case["y"].max()) == c - 1 and p == case["p"]
    an = K.analyse(case, case["params"], 0)
    K.check_conditions(case, an)
    assert an["r32"]["Z1"].dtype == np.float32 and an["r32"]["dW1"].dtype == np.float32
    assert an["tau"] > 0 or p == 1.0
    rows = np.diff(case["adj"].indptr)
    if name == "A":
        assert rows.max() > 128 and np.diff(case["adj"].tocsc().indptr).max() > 128     # hub rows and hub columns
    if name == "D":
        assert rows.min() == 0 and np.diff(case["adj"].tocsc().indptr).min() == 0
    if name in ("B", "E"):
        assert h % 4 and f % 4 == 1
    if name in ("A", "B", "T"):
        assert np.array_equal(graph.csr_arrays(case["adj"])[3], case["adj"].data)       # the reference reads the device's values
        assert not np.array_equal(an["keep"], T.dropout_keep(n, h, 1, K.SEED, p))


def _ulps(a, b):
    ia = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_adam_restatement_against_torch(wd):
    """The numpy restatement of the kernel's op order against torch's single-tensor Adam on the CPU (torch 2.10).  What
    holds: with torch's own sqrt substituted, the restatement is BITWISE equal to torch (m, v and p, every step) -- the
    weight-decay add, lerp_ and addcmul_ are fused multiply-adds in torch's vectorised CPU kernels, and so in the
    restatement and the kernel.  With the correctly rounded sqrt the kernel uses, m and v stay bitwise and p differs
    where torch's vectorised sqrt is not correctly rounded.  A 1-ulp sqrt difference passes through the division and the
    final add (two more roundings), so the gate on p is 2 ulp of the largest of |p|, |p_new| and the step (observed: 2)."""
    rng = np.random.RandomState(0)
    n = 4099
    p0 = rng.standard_normal(n).astype(np.float32) * 0.1
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=0.01, weight_decay=wd, foreach=False)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    n_diff = 0
    for step in range(1, 8):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 1, n)).astype(np.float32)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[tp]
        tp1, tm1, tv1 = tp.detach().numpy().copy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
        torch_sqrt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).sqrt().numpy()   # noqa: E731
        ps, ms, vs = T.adam_step(p, g, m, v, step, 0.01, weight_decay=wd, sqrt=torch_sqrt)
        assert np.array_equal(ps, tp1) and np.array_equal(ms, tm1) and np.array_equal(vs, tv1), step
        pc, mc, vc = T.adam_step(p, g, m, v, step, 0.01, weight_decay=wd)
        assert np.array_equal(mc, tm1) and np.array_equal(vc, tv1), step
        bound = np.spacing(np.maximum(np.maximum(np.abs(p), np.abs(tp1)), np.abs(tp1 - p)).astype(np.float32))
        assert np.all(np.abs(pc - tp1) <= 2 * bound), step
        n_diff += int((pc != tp1).sum())
        p, m, v = tp1, tm1.copy(), tv1.copy()
    print(f"adam restatement vs torch CPU (weight_decay={wd}): bitwise with torch's sqrt; with a correctly rounded sqrt "
          f"{n_diff} of {7 * n} parameter updates differ, within 2 ulp of max(|p|, |p_new|, |step|)")


def test_train_switch_parses():
    from linkteller_amd import main as lt_main
    a = lt_main.get_arguments(["--train"])
    assert a.train is True and a.test is False
    assert lt_main.get_arguments([]).train is False
    a = lt_main.get_arguments(["--train-ratio", "0.3", "--trainable"])
    assert a.train_ratio == 0.3 and a.trainable is True and a.train is False
    a = lt_main.get_arguments(["--train", "--train-ratio", "0.7"])
    assert a.train and a.train_ratio == 0.7 and not a.trainable


def test_train_refusals():
    from linkteller_amd import main as lt_main
    with pytest.raises(NotImplementedError):
        lt_main.main(["--train", "--n-layer", "3", "--dataset", "twitch/ES/RU"])
    with pytest.raises(NotImplementedError):
        lt_main.main(["--dataset", "twitch/ES/RU"])           # neither --test nor --train: still refused


def test_trainer_refuses_bad_dropout_and_no_gpu():
    from linkteller_amd import _lib, engine
    import scipy.sparse as sp
    z = torch.zeros
    with pytest.raises(ValueError):
        engine.GCN2Trainer(sp.identity(4, format="csr"), z(4, 3), [0, 1, 0, 1], z(3, 2), z(2), z(2, 2), z(2),
                           lr=0.01, weight_decay=0.0, dropout=1.5, seed=0)
    if torch.cuda.is_available():
        return
    with pytest.raises(_lib.LinkTellerHipError):
        engine.GCN2Trainer(sp.identity(4, format="csr"), z(4, 3), [0, 1, 0, 1], z(3, 2), z(2), z(2, 2), z(2),
                           lr=0.01, weight_decay=0.0, dropout=0.5, seed=0)


@pytest.mark.parametrize("h", [16, 64])
def test_init_law_matches_reference(h):
    from linkteller_amd.gcn import GCN
    g = load_golden("train.npz")
    torch.manual_seed(42)
    model = GCN(nfeat=g["x1"].shape[1], nhid=h, nclass=2, dropout=0.5)
    for name, p in model.state_dict().items():
        assert np.array_equal(p.numpy(), g[f"FirstOrderGCN.h{h}.init.{name}"]), name

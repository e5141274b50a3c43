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

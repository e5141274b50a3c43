"""The 3-layer training epoch (lt_gcn3_trainer_*, lt_train.hip) against train3_restate.epoch_reference3 in fp64, case by case
(train3_cases.py): hub rows in both wide layers, pad columns in both hidden widths, partial MFMA tiles in M, N and K of
dW2 = H1d^T dS2 and of the dZ1 product, a directed graph, H2 > H1 and K = 256, p = 0 / 1, one class, the smallest shapes; the
epoch word and the layer word of the Philox counter, Adam over six tensors, the mirrors, determinism, the C ABI's leading
dimensions, the refusals, and the 2-layer trainer's bits next to a 3-layer one.

Each check runs the epochs before the checked one, reads the parameters back, runs one more epoch and compares that epoch
with the reference evaluated AT THE READ-BACK PARAMETERS with that epoch's two masks.  Gate, per tensor
(train_cases.gate): err_hip <= 2 err_fp32 + 1e-6 max|ref64| + 1e-12 with err_fp32 from the same reference in float32.  The
gradients are compared with the fp64 derivative of the function the device evaluated: the reference takes the ReLU patterns
hidden(k) > 0 the device used, which may differ from the fp64 ones only at near-kink elements (asserted)."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import train_cases as K
import train_restate as T
import train3_cases as K3
import train3_restate as T3

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(ts):
    return [t.cpu().numpy().copy() for t in ts]


def _trainer(case, params, dropout=None, weight_decay=K3.DECAY):
    from linkteller_amd import engine
    return engine.GCN3Trainer(case["adj"], _dev(case["x"]), _dev(case["y"]), *params, lr=K3.LR, weight_decay=weight_decay,
                              dropout=case["p"] if dropout is None else dropout, seed=K3.SEED)


_cases, _epochs = {}, {}


def _case(name, h2=None):
    if (name, h2) not in _cases:
        _cases[name, h2] = K3.make(name, h2)
    return _cases[name, h2]


def _epoch(name, epoch, h2=None):
    """Run `epoch` epochs, read the parameters back, run one more: (case, parameters the checked epoch started from, what the
    device produced in it as float64 arrays).  Computed once per (case, epoch) and shared."""
    if (name, epoch, h2) in _epochs:
        return _epochs[name, epoch, h2]
    case = _case(name, h2)
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params)
    if epoch:
        tr.run(epoch)
    start = _host(params)
    loss, correct = tr.run(1)
    assert tr.epoch == epoch + 1
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(K3.NAMES, tr.grads())}
    got["Z3"] = tr.logits().cpu().numpy().astype(np.float64)
    got["H1d"] = tr.hidden(1).cpu().numpy().astype(np.float64)
    got["H2d"] = tr.hidden(2).cpu().numpy().astype(np.float64)
    got["loss"], got["correct"] = float(loss[0]), int(correct[0])
    _epochs[name, epoch, h2] = (case, start, got)
    return _epochs[name, epoch, h2]


def _forward_errors(an, got):
    r64, r32 = an["r64"], an["r32"]
    out = [(k, float(np.abs(got[k] - r64[k]).max()), K.gate(np.abs(r32[k].astype(np.float64) - r64[k]).max(), r64[k]))
           for k in ("H1d", "H2d", "Z3")]
    out.append(("loss", abs(got["loss"] - r64["loss"]), K.gate(abs(r32["loss"] - r64["loss"]), np.float64(r64["loss"]))))
    return out


def _compare(case, start, epoch, got):
    torch.set_num_threads(1)
    an = K3.analyse(case, start, epoch)
    K3.check_conditions(case, an)
    r64 = an["r64"]
    # 1. the ReLU patterns the device used
    on = []
    for k, (hk, zk) in enumerate((("H1d", "Z1"), ("H2d", "Z2"))):
        on_k = got[hk] > 0
        diff = on_k != (an["keep"][k] & (r64[zk] > 0))
        print(f"  {case['name']} epoch {epoch} layer {k + 1}: pattern differs at {int(diff.sum())} elements "
              f"({int(an['near'][k].sum())} near-kink)")
        assert not (diff & ~an["near"][k]).any(), (case["name"], epoch, k, int((diff & ~an["near"][k]).sum()))
        on.append(on_k)
    # 2. forward
    errs = _forward_errors(an, got)
    # 3. gradients: the derivative of the function the device evaluated
    g64 = T3.epoch_reference3(*an["args"], np.float64, on1=on[0], on2=on[1])
    g32 = T3.epoch_reference3(*an["args"], np.float32, on1=on[0], on2=on[1])
    for k in K3.NAMES:
        errs.append((k, float(np.abs(got[k] - g64[k]).max()), K.gate(np.abs(g32[k].astype(np.float64) - g64[k]).max(), g64[k])))
    for k, e, g in errs:
        print(f"  {case['name']} epoch {epoch} {k}: err_hip {e:.3e}  gate {g:.3e}  ratio {e / g:.3f}")
    for k, e, g in errs:
        assert e <= g, (case["name"], epoch, k, e, g)
    # 4. correct count
    want = int((r64["argmax"] == case["y"]).sum())
    print(f"  {case['name']} epoch {epoch} correct: {got['correct']} (fp64 {want}, fragile rows {an['fragile']})")
    assert an["fragile"] == 0 and got["correct"] == want, (got["correct"], want, an["fragile"])
    return an


@pytest.mark.parametrize("name,epoch", K3.CASE_EPOCHS, ids=[f"{k}-epoch{e}" for k, e in K3.CASE_EPOCHS])
def test_epoch_against_fp64(name, epoch):
    case, start, got = _epoch(name, epoch)
    _compare(case, start, epoch, got)
    if name == "C3":      # one class: the loss and every gradient are exactly zero
        assert got["loss"] == 0.0 and got["correct"] == case["n"]
        assert all(not got[k].any() for k in K3.NAMES)
        assert np.abs(got["Z3"]).max() > 0
    if name == "E3":      # p = 1: nothing is kept
        assert all(not got[k].any() for k in K3.NAMES[:5]) and np.abs(got["db3"]).max() > 0
        assert not got["H1d"].any() and not got["H2d"].any()
        assert np.array_equal(got["Z3"], np.broadcast_to(start[5].astype(np.float64), got["Z3"].shape))


def test_epoch_word_and_layer_word_reach_the_counter():
    """Case B3, epoch 2, judged with epoch 0's masks: the logits miss their gate by more than 100x.  B3 with H2 = H1 = 30,
    epoch 2, judged with the two layers' masks swapped: the same.  The right masks pass both times."""
    torch.set_num_threads(1)
    case, start, got = _epoch("B3", 2)
    right, wrong = K3.analyse(case, start, 2), K3.analyse(case, start, 2, mask_epoch=0)
    z_right, z_wrong = _forward_errors(right, got)[2], _forward_errors(wrong, got)[2]
    print(f"  epoch 2 logits with epoch 2's masks: {z_right[1]:.3e} (gate {z_right[2]:.3e}); with epoch 0's: {z_wrong[1]:.3e} "
          f"(gate {z_wrong[2]:.3e})")
    assert z_right[0] == "Z3" and z_right[1] <= z_right[2]
    assert z_wrong[1] > 100 * z_wrong[2]
    case, start, got = _epoch("B3", 2, h2=30)
    assert case["H1"] == case["H2"] == 30
    right, wrong = K3.analyse(case, start, 2), K3.analyse(case, start, 2, swap=True)
    z_right, z_wrong = _forward_errors(right, got)[2], _forward_errors(wrong, got)[2]
    print(f"  H1 = H2 = 30, epoch 2 logits with the layers' own masks: {z_right[1]:.3e} (gate {z_right[2]:.3e}); swapped: "
          f"{z_wrong[1]:.3e} (gate {z_wrong[2]:.3e})")
    assert z_right[1] <= z_right[2]
    assert z_wrong[1] > 100 * z_wrong[2]


def test_adam_inside_the_epoch_bitwise():
    """Case B3 with weight decay: after each of four run(1), the six device parameters equal a host copy of (p, m, v) over the
    concatenation W1 | b1 | W2 | b2 | W3 | b3 advanced by train_restate.adam_step with that epoch's grads(), step = epoch + 1."""
    case = _case("B3")
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params, weight_decay=K3.DECAY)
    sizes = [p.size for p in case["params"]]
    p = np.concatenate([a.ravel() for a in case["params"]]).astype(np.float32)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for e in range(4):
        tr.run(1)
        g = np.concatenate([t.ravel() for t in _host(tr.grads())])
        assert g.dtype == np.float32 and np.abs(g).max() > 0
        p, m, v = T.adam_step(p, g, m, v, e + 1, K3.LR, weight_decay=K3.DECAY)
        for name, want, got in zip(("W1", "b1", "W2", "b2", "W3", "b3"), np.split(p, np.cumsum(sizes)[:-1]), _host(params)):
            assert np.array_equal(got.ravel(), want), (e, name, int((got.ravel() != want).sum()))


def test_mirrors_follow_an_outside_change():
    """The padded copies of b1, b2, W3 are rebuilt at every run: after run(2) with
    p = 0, W2, W3 and b1 are overwritten in place; the next epoch's logits are within the gate of the reference at the new
    parameters and differ from the stale ones."""
    torch.set_num_threads(1)
    case = dict(_case("B3"), p=0.0)
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params, dropout=0.0)
    tr.run(2)
    rng = np.random.RandomState(9)
    for k in (2, 4, 1):
        params[k].copy_(_dev(rng.uniform(-0.5, 0.5, case["params"][k].shape).astype(np.float32)))
    start = _host(params)
    stale = tr.logits().cpu().numpy()
    tr.run(1)
    z = tr.logits().cpu().numpy()
    an = K3.analyse(case, start, 2)
    err = float(np.abs(z.astype(np.float64) - an["r64"]["Z3"]).max())
    gate = K.gate(np.abs(an["r32"]["Z3"].astype(np.float64) - an["r64"]["Z3"]).max(), an["r64"]["Z3"])
    print(f"  logits after the outside change: err {err:.3e}  gate {gate:.3e}; stale differ by {np.abs(z - stale).max():.3e}")
    assert err <= gate
    assert not np.array_equal(z, stale)


def test_deterministic_and_resumable():
    """p = 0.5: run(12) equals run(5); run(7), and both equal a second trainer -- record, grads(), logits() and parameters,
    bit for bit."""
    case = dict(_case("B3"), p=0.5)
    runs = []
    for chunks in ([12], [5, 7], [12]):
        params = [_dev(p.copy()) for p in case["params"]]
        tr = _trainer(case, params)
        rec = np.concatenate([tr.run_async(k).cpu().numpy() for k in chunks])
        assert tr.epoch == 12 and np.isfinite(rec).all()
        runs.append([rec] + _host(tr.grads()) + [tr.logits().cpu().numpy()] + _host(params))
    for other in runs[1:]:
        for i, (a, b) in enumerate(zip(runs[0], other)):
            assert np.array_equal(a, b), i
    assert not np.array_equal(runs[0][-6], case["params"][0])


def test_padded_operands_through_the_c_abi():
    """Case B3 through lt_gcn3_trainer_create with ldx = 304 > F = 301 (the pad columns hold NaN), lt_gcn3_trainer_logits with
    ldz = 5 > C and lt_gcn3_trainer_hidden with ld = H + 3 into sentinel-filled tensors: the bits are the dense run's, the
    pad columns keep the sentinel."""
    from linkteller_amd import _lib, graph
    case = _case("B3")
    n, f, h1, h2, c = case["n"], case["F"], case["H1"], case["H2"], case["C"]
    dense_p = [_dev(p.copy()) for p in case["params"]]
    dense = _trainer(case, dense_p)
    lib, dev = _lib.lib(), dense_p[0].device
    xp = torch.full((n, 304), float("nan"), dtype=torch.float32, device=dev)
    xp[:, :f] = _dev(case["x"])
    g = graph.as_hip_graph(case["adj"])
    labels = _dev(case["y"]).to(torch.int32).contiguous()
    raw_p = [_dev(p.copy()) for p in case["params"]]
    handle = C.c_void_p()
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.lt_gcn3_trainer_create(g.handle, xp.data_ptr(), 304, f, labels.data_ptr(), h1, h2, c,
                                          *[t.data_ptr() for t in raw_p], K3.LR, K3.DECAY, case["p"], K3.SEED, stream,
                                          C.byref(handle)), "lt_gcn3_trainer_create")
    try:
        for e in range(3):
            rec_d = dense.run_async(1)
            rec_r = torch.empty((1, 2), dtype=torch.float32, device=dev)
            _lib.check(lib.lt_gcn3_trainer_run(handle, 1, rec_r.data_ptr(), stream), "lt_gcn3_trainer_run")
            grads = [torch.empty_like(p) for p in raw_p]
            _lib.check(lib.lt_gcn3_trainer_grads(handle, *[t.data_ptr() for t in grads], stream), "lt_gcn3_trainer_grads")
            z = torch.full((n, 5), -77.25, dtype=torch.float32, device=dev)
            _lib.check(lib.lt_gcn3_trainer_logits(handle, z.data_ptr(), 5, stream), "lt_gcn3_trainer_logits")
            hid = []
            for layer, h in ((1, h1), (2, h2)):
                t = torch.full((n, h + 3), -77.25, dtype=torch.float32, device=dev)
                _lib.check(lib.lt_gcn3_trainer_hidden(handle, layer, t.data_ptr(), h + 3, stream), "lt_gcn3_trainer_hidden")
                hid.append(t)
            torch.cuda.synchronize()
            assert torch.equal(rec_r, rec_d) and bool(torch.isfinite(rec_r).all()), e
            for k, a, b in zip(K3.NAMES, grads, dense.grads()):
                assert torch.equal(a, b), (e, k)
            assert torch.equal(z[:, :c].contiguous(), dense.logits()), e
            assert bool((z[:, c:] == -77.25).all()), e
            for layer, h, t in ((1, h1, hid[0]), (2, h2, hid[1])):
                assert torch.equal(t[:, :h].contiguous(), dense.hidden(layer)), (e, layer)
                assert bool((t[:, h:] == -77.25).all()), (e, layer)
            for a, b in zip(raw_p, dense_p):
                assert torch.equal(a, b), e
        assert bool(torch.isnan(xp[:, f:]).all())
        assert lib.lt_gcn3_trainer_hidden(handle, 3, hid[0].data_ptr(), h1 + 3, stream) == -1
        assert lib.lt_gcn3_trainer_hidden(handle, 1, hid[0].data_ptr(), h1 - 1, stream) == -1
    finally:
        _lib.check(lib.lt_gcn3_trainer_destroy(handle), "lt_gcn3_trainer_destroy")


def test_refusals():
    from linkteller_amd import _lib, synth
    n, f = 50, 20
    adj = synth.erdos_renyi_graph(n, 100, seed=1)
    x = synth.gaussian_features(n, f, seed=1)
    y = np.zeros(n, np.int64)
    case = dict(adj=adj, x=x, y=y, p=0.5)
    for h1, h2, c in ((257, 16, 2), (16, 257, 2), (16, 16, 9)):
        with pytest.raises(_lib.LinkTellerHipError):
            _trainer(case, [_dev(p) for p in K3.init_params(f, h1, h2, c)])
    ok = lambda: [_dev(p) for p in K3.init_params(f, 16, 8, 2)]      # noqa: E731
    bad = x.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError):
        _trainer(dict(case, x=bad), ok())
    with pytest.raises(ValueError):
        _trainer(dict(case, y=np.full(n, 2)), ok())
    _trainer(case, ok()).run(1)


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


PARENT_SHA = "f7de0246d36b21000465dcdce6695f6903841b274216a15091e227a82e0763c1"


def test_two_layer_trainer_is_untouched():
    """Case B of train_cases through GCN2Trainer (three epochs: record, grads, parameters) gives the same bits before and
    after three GCN3Trainer epochs ran in the same process -- the layer word added to the Philox counter defaults to 0 and
    the shared kernels kept their arithmetic.  sha256 over record | grads | parameters as produced by a build of the commit
    before the 3-layer trainer on an MI355X:
    f7de0246d36b21000465dcdce6695f6903841b274216a15091e227a82e0763c1 (asserted)."""
    from linkteller_amd import engine

    def two_layer():
        case = K.make("B")
        params = [_dev(p.copy()) for p in case["params"]]
        tr = engine.GCN2Trainer(case["adj"], _dev(case["x"]), _dev(case["y"]), *params, lr=K.LR, weight_decay=K.DECAY,
                                dropout=case["p"], seed=K.SEED)
        rec = tr.run_async(3).cpu().numpy()
        return [rec] + _host(tr.grads()) + _host(params)

    before = two_layer()
    case3 = _case("B3")
    _trainer(case3, [_dev(p.copy()) for p in case3["params"]]).run(3)
    after = two_layer()
    print(f"  2-layer case B, three epochs: sha256 {_sha(before)}")
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert _sha(before) == PARENT_SHA

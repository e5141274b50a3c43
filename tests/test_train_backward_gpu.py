"""The training backward (lt_train.hip) against train_restate.epoch_reference in fp64, case by case (train_cases.py): every
route of the backward kernels -- split-K and partial tiles of dW1 = X^T dS1, per-element Philox selection, the epoch word
of the counter, the widths of k_tr_bwd_rows, the loss head at C != 2 and n < 256, hub rows and the tiled layer 1 inside the
trainer, the A^T products on a directed graph, Adam inside the epoch and its mirrors, p = 1 and C = 1.

Each check runs the epochs before the checked one, reads the parameters back, runs one more epoch and compares that epoch
with the reference evaluated AT THE READ-BACK PARAMETERS with that epoch's mask, so no check depends on trajectory drift and
a wrong mask is an O(1) error in the logits.  Gate, per tensor (test_train_gpu.test_first_epoch_gradients_against_fp64):
err_hip <= 2 err_fp32 + 1e-6 max|ref64| + 1e-12 with err_fp32 from the same reference in float32.  Hidden columns with
near-kink elements (train_restate.near_kink) are held to the interval between the fp64 gradients with all of their
near-kink derivatives off and all on, widened by the same gate; they are at most 1/8 of H (asserted)."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_cases as K
import train_restate as T

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(ts):
    return [t.cpu().numpy().copy() for t in ts]


def _trainer(case, params, dropout=None, weight_decay=K.DECAY):
    from linkteller_amd import engine
    return engine.GCN2Trainer(case["adj"], _dev(case["x"]), _dev(case["y"]), *params, lr=K.LR, weight_decay=weight_decay,
                              dropout=case["p"] if dropout is None else dropout, seed=K.SEED)


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = K.make(name)
    return _cases[name]


def _epoch(name, epoch):
    """Run `epoch` epochs, read the parameters back, run one more: (case, parameters the checked epoch started from, its
    record, its gradients and logits as float64 arrays)."""
    case = _case(name)
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params)
    if epoch:
        tr.run(epoch)
    start = _host(params)
    loss, correct = tr.run(1)
    assert tr.epoch == epoch + 1
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(K.NAMES, tr.grads())}
    got["Z2"] = tr.logits().cpu().numpy().astype(np.float64)
    got["loss"], got["correct"] = float(loss[0]), int(correct[0])
    return case, start, got


def _errors(case, an, got):
    """[(name, err_hip, gate)] of one epoch against `an`; for dW1 / db1 over the hidden columns without near-kink elements."""
    r64, r32 = an["r64"], an["r32"]
    strict = ~an["kink_cols"]
    out = []
    for k in K.NAMES + ("Z2",):
        a, b64, b32 = got[k], r64[k], r32[k].astype(np.float64)
        if k in ("dW1", "db1"):
            a, b64s, b32 = a[..., strict], b64[..., strict], b32[..., strict]
        else:
            b64s = b64
        out.append((k, float(np.abs(a - b64s).max()), K.gate(np.abs(b32 - b64s).max(), b64)))
    out.append(("loss", abs(got["loss"] - r64["loss"]), K.gate(abs(r32["loss"] - r64["loss"]), np.float64(r64["loss"]))))
    return out


def _compare(case, start, epoch, got):
    torch.set_num_threads(1)
    an = K.analyse(case, start, epoch)
    K.check_conditions(case, an)
    errs = _errors(case, an, got)
    for k, e, g in errs:
        print(f"  {case['name']} epoch {epoch} {k}: err_hip {e:.3e}  gate {g:.3e}  ratio {e / g:.3f}")
    for k, e, g in errs:
        assert e <= g, (case["name"], epoch, k, e, g)
    cols = an["kink_cols"]
    if cols.any():
        for k, (_, _, g) in zip(("dW1", "db1"), errs[:2]):
            lo = np.minimum(an["off"][k], an["on"][k])[..., cols] - g
            hi = np.maximum(an["off"][k], an["on"][k])[..., cols] + g
            a = got[k][..., cols]
            out = np.maximum(lo - a, a - hi).max()
            print(f"  {case['name']} epoch {epoch} {k}: {int(cols.sum())} near-kink columns, outside their interval by {out:.3e}")
            assert out <= 0, (case["name"], epoch, k, out, g)
    want = int((an["r64"]["argmax"] == case["y"]).sum())
    print(f"  {case['name']} epoch {epoch} correct: {got['correct']} (fp64 {want}, fragile rows {an['fragile']})")
    assert abs(got["correct"] - want) <= an["fragile"], (got["correct"], want, an["fragile"])
    return an


# Case T and the second checked epoch of A and B are not marked slow: the whole module takes 2.7 s on an MI355X against
# test_train_gpu.py's 19.5 s (NOTES.md).
@pytest.mark.parametrize("name,epoch", K.CASE_EPOCHS, ids=[f"{k}-epoch{e}" for k, e in K.CASE_EPOCHS])
def test_epoch_against_fp64(name, epoch):
    case, start, got = _epoch(name, epoch)
    _compare(case, start, epoch, got)
    if name == "C":      # one class: the loss and every gradient are exactly zero
        assert got["loss"] == 0.0 and got["correct"] == case["n"]
        assert all(not got[k].any() for k in K.NAMES)
        assert np.abs(got["Z2"]).max() > 0
    if name == "E":      # p = 1: nothing is kept
        assert all(not got[k].any() for k in ("dW1", "db1", "dW2")) and np.abs(got["db2"]).max() > 0
        assert np.array_equal(got["Z2"], np.broadcast_to(start[3].astype(np.float64), got["Z2"].shape))


def test_epoch_word_reaches_the_counter():
    """Case B, epoch 2, judged with epoch 0's mask: the logits must miss their gate by more than 100x -- the comparison of
    test_epoch_against_fp64 tells one epoch's mask from another's."""
    case, start, got = _epoch("B", 2)
    torch.set_num_threads(1)
    right, wrong = K.analyse(case, start, 2), K.analyse(case, start, 2, mask_epoch=0)
    z_right, z_wrong = _errors(case, right, got)[4], _errors(case, wrong, got)[4]
    print(f"  epoch 2 logits with epoch 2's mask: {z_right[1]:.3e} (gate {z_right[2]:.3e}); with epoch 0's: {z_wrong[1]:.3e} "
          f"(gate {z_wrong[2]:.3e})")
    assert z_right[0] == "Z2" and z_right[1] <= z_right[2]
    assert z_wrong[1] > 100 * z_wrong[2]


def test_padded_features_and_logits_through_the_c_abi():
    """Case B through lt_gcn2_trainer_create with ldx = 304 > F = 301 (the three pad columns hold NaN) and
    lt_gcn2_trainer_logits with ldz = 5 > C = 3 into a sentinel-filled tensor: record, gradients, logits and parameters
    equal the dense run's bits after each of three epochs, and the pad columns of the logits keep the sentinel."""
    from linkteller_amd import _lib, graph
    case = _case("B")
    n, f, h, c = case["n"], case["F"], case["H"], case["C"]
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
    _lib.check(lib.lt_gcn2_trainer_create(g.handle, xp.data_ptr(), 304, f, labels.data_ptr(), h, c,
                                          *[t.data_ptr() for t in raw_p], K.LR, K.DECAY, case["p"], K.SEED, stream,
                                          C.byref(handle)), "lt_gcn2_trainer_create")
    try:
        for e in range(3):
            rec_d = dense.run_async(1)
            rec_r = torch.empty((1, 2), dtype=torch.float32, device=dev)
            _lib.check(lib.lt_gcn2_trainer_run(handle, 1, rec_r.data_ptr(), stream), "lt_gcn2_trainer_run")
            grads = [torch.empty_like(p) for p in raw_p]
            _lib.check(lib.lt_gcn2_trainer_grads(handle, *[t.data_ptr() for t in grads], stream), "lt_gcn2_trainer_grads")
            z = torch.full((n, 5), -77.25, dtype=torch.float32, device=dev)
            _lib.check(lib.lt_gcn2_trainer_logits(handle, z.data_ptr(), 5, stream), "lt_gcn2_trainer_logits")
            torch.cuda.synchronize()
            assert torch.equal(rec_r, rec_d) and bool(torch.isfinite(rec_r).all()), e
            for k, a, b in zip(K.NAMES, grads, dense.grads()):
                assert torch.equal(a, b), (e, k)
            assert torch.equal(z[:, :c].contiguous(), dense.logits()), e
            assert bool((z[:, c:] == -77.25).all()), e
            for a, b in zip(raw_p, dense_p):
                assert torch.equal(a, b), e
        assert bool(torch.isnan(xp[:, f:]).all())
    finally:
        _lib.check(lib.lt_gcn2_trainer_destroy(handle), "lt_gcn2_trainer_destroy")


@pytest.mark.parametrize("name", ["A", "B"])
def test_tiled_layer1_inside_the_trainer(name):
    """The tiled layer-1 route forced (tiled_min_bytes = 0) on case A (hub rows: their segments and k_layer1_long run inside
    the trainer) and on case B (a pad column): three epochs give the row route's record, gradients, logits and parameters
    bit for bit."""
    from linkteller_amd import _lib, graph
    case = _case(name)
    if name == "A":
        assert graph.as_hip_graph(case["adj"]).max_row_nnz > 128      # longer than one layer-1 segment
    runs = []
    for tiled in (False, True):
        params = [_dev(p.copy()) for p in case["params"]]
        if tiled:
            _lib.set_tuning("tiled_min_bytes", 0)
        try:
            tr = _trainer(case, params)
            rec = tr.run_async(3).cpu().numpy()
            runs.append((rec, _host(tr.grads()), tr.logits().cpu().numpy(), _host(params)))
        finally:
            _lib.set_tuning("tiled_min_bytes", None)
    (rec0, g0, z0, p0), (rec1, g1, z1, p1) = runs
    assert np.isfinite(rec0).all() and np.array_equal(rec0, rec1) and np.array_equal(z0, z1)
    for a, b in zip(g0 + p0, g1 + p1):
        assert np.array_equal(a, b)
    assert not np.array_equal(p0[0], case["params"][0])


def test_adam_inside_the_epoch_bitwise():
    """Case B with weight decay: after each of four run(1), the four device parameters equal a host copy of (p, m, v) over the
    concatenation W1 | b1 | W2 | b2 advanced by train_restate.adam_step with that epoch's grads() and step = epoch + 1."""
    case = _case("B")
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params, weight_decay=K.DECAY)
    sizes = [p.size for p in case["params"]]
    p = np.concatenate([a.ravel() for a in case["params"]]).astype(np.float32)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for e in range(4):
        tr.run(1)
        g = np.concatenate([t.ravel() for t in _host(tr.grads())])
        assert g.dtype == np.float32 and np.abs(g).max() > 0
        p, m, v = T.adam_step(p, g, m, v, e + 1, K.LR, weight_decay=K.DECAY)
        for name, want, got in zip(("W1", "b1", "W2", "b2"), np.split(p, np.cumsum(sizes)[:-1]), _host(params)):
            assert np.array_equal(got.ravel(), want), (e, name, int((got.ravel() != want).sum()))


@pytest.mark.parametrize("name", ["B", "D"])
def test_mirrors_follow_an_outside_change(name):
    """The padded copies of b1 and W2 that the row kernels read are rebuilt at every run: after run(2) with p = 0, W2 and b1
    are overwritten in place, and the next epoch's logits are gcn2_forward's bits for the new parameters (B: H = 30, the
    forward pads too; D: H = 100, the forward reads the caller's tensors)."""
    from linkteller_amd import engine
    case = _case(name)
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params, dropout=0.0)
    tr.run(2)
    rng = np.random.RandomState(9)
    params[2].copy_(_dev(rng.uniform(-0.5, 0.5, case["params"][2].shape).astype(np.float32)))
    params[1].copy_(_dev(rng.uniform(-0.5, 0.5, case["params"][1].shape).astype(np.float32)))
    x = _dev(case["x"])
    ref = engine.gcn2_forward(case["adj"], x, *[p.clone() for p in params])
    stale = tr.logits()
    tr.run(1)
    assert torch.equal(tr.logits(), ref)
    assert not torch.equal(stale, ref)

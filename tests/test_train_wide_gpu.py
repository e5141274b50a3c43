"""The 2-layer trainer with the wide head (lt_gcn2_trainer_create_wide, lt_eval_head_wide; lt_train_wide.hip.h) against
train_wide_restate.epoch_reference_wide in fp64, case by case (train_wide_cases.py): the first width the narrow head refuses,
reddit's and ppi's class counts, the lane-group and GEMM-tile edge at 64 / 65, the limit C = 256 with C > H, one class, p = 1;
both losses; determinism, the narrow head next to the wide one, the evaluation head over row lists, validated runs, the C ABI's
refusals and exports.

Method of test_train3_backward_gpu.py: run the epochs before the checked one, read the parameters back, run one more epoch and
compare it with the reference evaluated AT THE READ-BACK PARAMETERS with that epoch's mask.  Gate per tensor (train_cases.gate):
err_hip <= 2 err_fp32 + 1e-6 max|ref64| + 1e-12, err_fp32 from the same restatement in float32.  The gradients are compared
with the fp64 derivative of the function the device evaluated: the reference takes the ReLU pattern hidden() > 0, which may
differ from the fp64 one only at near-kink elements (asserted)."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_cases as K
import train_wide_cases as KW
import train_wide_restate as TW
import validate_restate as VR

pytestmark = pytest.mark.gpu

INVALID = -1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(ts):
    return [t.cpu().numpy().copy() for t in ts]


def _trainer(case, params, dropout=None, lr=KW.LR, head="wide", loss=None):
    from linkteller_amd import engine
    return engine.GCN2Trainer(case["adj"], _dev(case["x"]), _dev(case["y"]), *params, lr=lr, weight_decay=KW.DECAY,
                              dropout=case["p"] if dropout is None else dropout, seed=KW.SEED, head=head,
                              loss=case["loss"] if loss is None else loss)


_cases, _epochs = {}, {}


def _case(name):
    if name not in _cases:
        _cases[name] = KW.make(name)
    return _cases[name]


def _read(tr):
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(KW.NAMES, tr.grads())}
    got["Z2"] = tr.logits().cpu().numpy().astype(np.float64)
    got["H1d"] = tr.hidden().cpu().numpy().astype(np.float64)
    got["counts"] = tr.counts().cpu().numpy().astype(np.int64)
    return got


def _epoch(name, epoch):
    """(case, parameters the checked epoch started from, what the device produced in it); once per (case, epoch)."""
    if (name, epoch) in _epochs:
        return _epochs[name, epoch]
    case = _case(name)
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params)
    if epoch:
        tr.run(epoch)
    start = _host(params)
    loss, tp = tr.run(1)
    assert tr.epoch == epoch + 1
    got = _read(tr)
    got["loss"], got["tp"] = float(loss[0]), int(tp[0])
    _epochs[name, epoch] = (case, start, got)
    return _epochs[name, epoch]


def _compare(case, start, epoch, got):
    torch.set_num_threads(1)
    an = KW.analyse(case, start, epoch)
    KW.check_conditions(case, an)
    r64, r32 = an["r64"], an["r32"]
    on = got["H1d"] > 0
    diff = on != (an["keep"] & (r64["Z1"] > 0))
    print(f"  {case['name']} epoch {epoch}: pattern differs at {int(diff.sum())} elements ({int(an['near'].sum())} near-kink)")
    assert not (diff & ~an["near"]).any(), (case["name"], epoch, int((diff & ~an["near"]).sum()))
    errs = [(k, float(np.abs(got[k] - r64[k]).max()), K.gate(np.abs(r32[k].astype(np.float64) - r64[k]).max(), r64[k]))
            for k in ("H1d", "Z2")]
    errs.append(("loss", abs(got["loss"] - r64["loss"]), K.gate(abs(r32["loss"] - r64["loss"]), np.float64(r64["loss"]))))
    g64 = TW.epoch_reference_wide(*an["args"], np.float64, relu_on=on)
    g32 = TW.epoch_reference_wide(*an["args"], np.float32, relu_on=on)
    for k in KW.NAMES:
        errs.append((k, float(np.abs(got[k] - g64[k]).max()), K.gate(np.abs(g32[k].astype(np.float64) - g64[k]).max(), g64[k])))
    for k, e, g in errs:
        print(f"  {case['name']} epoch {epoch} {k}: err_hip {e:.3e}  gate {g:.3e}  ratio {e / g:.3f}")
    for k, e, g in errs:
        assert e <= g, (case["name"], epoch, k, e, g)
    assert np.isfinite(got["loss"]) and all(np.isfinite(got[k]).all() for k in KW.NAMES + ("Z2", "H1d"))
    assert np.array_equal(got["counts"], r64["counts"]), (case["name"], epoch)
    assert got["tp"] == int(r64["counts"][:, 0].sum())
    return an


@pytest.mark.parametrize("name,epoch", KW.CASE_EPOCHS, ids=[f"{k}-epoch{e}" for k, e in KW.CASE_EPOCHS])
def test_epoch_against_fp64(name, epoch):
    case, start, got = _epoch(name, epoch)
    _compare(case, start, epoch, got)
    if name == "P1":      # p = 1: nothing is kept, only db2 is not zero, the logits are b2
        assert not got["H1d"].any() and all(not got[k].any() for k in ("dW1", "db1", "dW2"))
        assert np.abs(got["db2"]).max() > 0
        assert np.array_equal(got["Z2"], np.broadcast_to(start[3].astype(np.float64), got["Z2"].shape))


def test_bce_at_large_logits():
    """W65 at p = 0 with W2 and b2 scaled by 300: logits beyond |z| = 90.  The loss is finite, every tensor passes its gate
    (sigma - y is then 0 or +-1 / (n C) to fp32's last bit where fp64 says so), nothing is NaN."""
    torch.set_num_threads(1)
    case = dict(_case("W65"), p=0.0)
    case["params"] = [case["params"][0], case["params"][1], case["params"][2] * np.float32(300), case["params"][3] * np.float32(300)]
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params)
    loss, tp = tr.run(1)
    got = _read(tr)
    got["loss"], got["tp"] = float(loss[0]), int(tp[0])
    assert np.abs(got["Z2"]).max() > 90
    an = KW.analyse(case, case["params"], 0)
    on = got["H1d"] > 0
    assert not ((on != (an["r64"]["Z1"] > 0)) & ~an["near"]).any()
    g64 = TW.epoch_reference_wide(*an["args"], np.float64, relu_on=on)
    g32 = TW.epoch_reference_wide(*an["args"], np.float32, relu_on=on)
    unit = 1.0 / (case["n"] * case["C"])
    saturated = int((np.abs(g64["dZ2"]) == unit).sum() + (g64["dZ2"] == 0).sum())
    print(f"  max|Z2| {np.abs(got['Z2']).max():.1f}, loss {got['loss']:.6f} (fp64 {g64['loss']:.6f}), saturated elements {saturated}")
    assert saturated > 0
    for k in ("Z2", "loss") + KW.NAMES:
        e = float(np.abs(got[k] - g64[k]).max())
        g = K.gate(np.abs(np.float64(g32[k]) - g64[k]).max(), np.float64(g64[k]))
        print(f"  large logits {k}: err_hip {e:.3e}  gate {g:.3e}")
        assert np.isfinite(got[k]).all() and e <= g, (k, e, g)
    assert an["fragile"] == 0 and np.array_equal(got["counts"], g64["counts"])


@pytest.mark.parametrize("name", ["W9", "W65"])
def test_deterministic_and_resumable(name):
    """p = 0.5: run(12) equals run(5); run(7), and both equal a second trainer -- record, grads, logits, counts and parameters,
    bit for bit."""
    case = _case(name)
    assert case["p"] == 0.5
    runs = []
    for chunks in ([12], [5, 7], [12]):
        params = [_dev(p.copy()) for p in case["params"]]
        tr = _trainer(case, params)
        rec = np.concatenate([tr.run_async(k).cpu().numpy() for k in chunks])
        assert tr.epoch == 12 and np.isfinite(rec).all()
        runs.append([rec] + _host(tr.grads()) + [tr.logits().cpu().numpy(), tr.counts().cpu().numpy()] + _host(params))
    for other in runs[1:]:
        for i, (a, b) in enumerate(zip(runs[0], other)):
            assert np.array_equal(a, b), (name, i)
    assert not np.array_equal(runs[0][-4], case["params"][0])


@pytest.mark.parametrize("c", [2, 7])
def test_the_two_heads_meet(c):
    """train_cases B's graph, features and widths with C classes: the narrow trainer and wide-ce pass the same fp64 gate on
    loss, logits and gradients (each with its own ReLU pattern), and count the same correct rows."""
    from linkteller_amd import synth
    torch.set_num_threads(1)
    base = K.make("B")
    w = synth.gcn_weights(base["F"], base["H"], c, seed=0)
    case = dict(base, C=c, loss="ce", y=np.random.RandomState(1).randint(0, c, base["n"]).astype(np.int64),
                params=[w[k] for k in ("W1", "b1", "W2", "b2")], name=f"B-C{c}")
    an = KW.analyse(case, case["params"], 0)
    KW.check_conditions(case, an)
    correct = {}
    for head in ("narrow", "wide"):
        params = [_dev(p.copy()) for p in case["params"]]
        tr = _trainer(case, params, head=head)
        loss, corr = tr.run(1)
        got = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(KW.NAMES, tr.grads())}
        got["Z2"], got["loss"] = tr.logits().cpu().numpy().astype(np.float64), np.float64(loss[0])
        on = tr.hidden().cpu().numpy() > 0
        assert not ((on != (an["keep"] & (an["r64"]["Z1"] > 0))) & ~an["near"]).any()
        g64 = TW.epoch_reference_wide(*an["args"], np.float64, relu_on=on)
        g32 = TW.epoch_reference_wide(*an["args"], np.float32, relu_on=on)
        for k in ("Z2", "loss") + KW.NAMES:
            e = float(np.abs(got[k] - g64[k]).max())
            g = K.gate(np.abs(np.float64(g32[k]) - g64[k]).max(), np.float64(g64[k]))
            print(f"  C = {c} {head} {k}: err_hip {e:.3e}  gate {g:.3e}")
            assert e <= g, (head, k, e, g)
        correct[head] = int(corr[0])
    assert correct["narrow"] == correct["wide"] == int(an["r64"]["counts"][:, 0].sum())


@pytest.mark.parametrize("key,loss", [("ce9", "ce"), ("bce12", "bce")])
def test_trajectory_against_reference(key, loss):
    """tests/golden/train_wide.npz: 40 epochs of the reference's GCN, losses and optim.Adam at p = 0 in fp64 and fp32
    (golden/generate_train_wide.py).  Gate of test_train_gpu.py: twice the reference fp32 run's own deviation from its fp64
    run plus the floor; the tp sums may differ by the rows (elements) the generator found fragile."""
    import scipy.sparse as sp
    from conftest import load_golden
    from linkteller_amd import engine
    gold = load_golden("train_wide.npz")
    n = gold["x"].shape[0]
    adj = sp.csr_matrix((gold["adj.data"], gold["adj.indices"], gold["adj.indptr"]), shape=(n, n))
    params = [_dev(gold[f"{key}.init.{k}"].copy()) for k in ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias")]
    tr = engine.GCN2Trainer(adj, _dev(gold["x"]), _dev(gold[f"{key}.y"]), *params, lr=float(gold["lr"]),
                            weight_decay=float(gold["decay"]), dropout=0.0, seed=1, head="wide", loss=loss)
    got, tp = tr.run(int(gold["epochs"]))
    l64, l32 = gold[f"{key}.loss64"], gold[f"{key}.loss32"]
    e, g = np.abs(got - l64).max(), 2 * np.abs(l32 - l64).max() + 1e-5
    print(f"  {key}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, |hip - fp64| max {e:.3e}, gate {g:.3e}")
    assert e <= g, (e, g)
    assert np.all(np.abs(tp - gold[f"{key}.tp64"]) <= gold[f"{key}.tiny64"]), (tp, gold[f"{key}.tp64"])
    # the trained parameters: the eval-mode logits they give, formed in fp64 on the host
    w1, b1, w2, b2 = (p.cpu().numpy().astype(np.float64) for p in params)
    a = adj.astype(np.float64)
    z = a @ (np.maximum(a @ (gold["x"].astype(np.float64) @ w1) + b1, 0) @ w2) + b2
    z64, z32 = gold[f"{key}.logits64"], gold[f"{key}.logits32"]
    assert np.abs(z - z64).max() <= 2 * np.abs(z32 - z64).max() + 1e-5 * np.abs(z64).max(), \
        (np.abs(z - z64).max(), np.abs(z32 - z64).max())


# ---- lt_eval_head_wide -------------------------------------------------------------------------------------------------------
N_EVAL = 300
_LISTS = {}


def _lists():
    if not _LISTS:
        rng = np.random.RandomState(3)
        for m in (1, 255, 256, 257, 513):
            _LISTS[m] = rng.randint(0, N_EVAL, m)      # repeats (513 > n forces them), any order
        _LISTS["perm"] = rng.permutation(N_EVAL)
    return _LISTS


def _eval_inputs(c, loss, seed=0):
    rng = np.random.RandomState(seed)
    z = (rng.standard_normal((N_EVAL, c)) * 3).astype(np.float32)
    z[np.abs(z) < 1e-3] = 0.5      # no fragile sign; the argmax margins of a 3-sigma draw are checked below
    y = KW.labels_for(N_EVAL, c, loss, seed)
    return z, y


def _gate_loss(z, y, loss, got):
    l64, _, counts = TW.head_reference(z, y, loss, np.float64)
    l32, _, _ = TW.head_reference(z, y, loss, np.float32)
    return abs(got - l64), K.gate(abs(l32 - l64), np.float64(l64)), counts


@pytest.mark.parametrize("loss", ["ce", "bce"])
@pytest.mark.parametrize("c", [9, 65, 121, 256])
def test_eval_head_wide_over_rows_and_lists(c, loss):
    from linkteller_amd import engine
    z, y = _eval_inputs(c, loss)
    if loss == "ce":
        assert TW.ce_margin_rows(z.astype(np.float64)) == 0
    zp = torch.full((N_EVAL, c + 3), float("nan"), dtype=torch.float32, device="cuda")      # ldz > C
    zp[:, :c] = _dev(z)
    zv = zp[:, :c]
    if loss == "bce":
        yp = torch.full((N_EVAL, c + 5), 1, dtype=torch.uint8, device="cuda")                # ldy > C
        yp[:, :c] = _dev(y)
        yv = yp[:, :c]
    else:
        yv = _dev(y)
    l_all, k_all = engine.eval_head_wide(zv, yv, loss=loss)
    e, g, counts = _gate_loss(z, y, loss, float(l_all))
    print(f"  C = {c} {loss} all rows: err {e:.3e}  gate {g:.3e}")
    assert e <= g and np.array_equal(k_all.cpu().numpy(), counts)
    l_id, k_id = engine.eval_head_wide(zv, yv, rows=np.arange(N_EVAL), loss=loss)            # the all-rows call's bits
    assert torch.equal(l_id, l_all) and torch.equal(k_id, k_all)
    for key, rows in _lists().items():
        l, k = engine.eval_head_wide(zv, yv, rows=rows, loss=loss)
        e, g, counts = _gate_loss(z[rows], y[rows], loss, float(l))
        assert e <= g and np.array_equal(k.cpu().numpy(), counts), (c, loss, key, e, g)


def _raw_eval(z, ldz, y, ldy, n, c, kind, rows, m, loss, counts, n_bad, ws, nbytes):
    from linkteller_amd import _lib
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    return _lib.lib().lt_eval_head_wide(ptr(z), ldz, ptr(y), ldy, n, c, kind, ptr(rows), m, ptr(loss), ptr(counts), ptr(n_bad),
                                        ptr(ws), nbytes, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("loss", ["ce", "bce"])
def test_eval_head_wide_skips_and_counts_ids_out_of_range(loss):
    from linkteller_amd import _lib
    c, kind = 65, {"ce": 0, "bce": 1}[loss]
    z, y = _eval_inputs(c, loss, seed=1)
    rows = _lists()[257].copy()
    bad = rows.copy()
    bad[[0, 100, 256]] = [-1, N_EVAL, 2 ** 31 - 1]
    good = np.delete(rows, [0, 100, 256])
    zd, yd = _dev(z), _dev(y if loss == "bce" else y.astype(np.int32))
    out_l = torch.zeros((), dtype=torch.float32, device="cuda")
    out_k = torch.zeros((c, 3), dtype=torch.int32, device="cuda")
    n_bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    nbytes = _lib.lib().lt_eval_head_wide_workspace_bytes(257, c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert _raw_eval(zd, c, yd, c, N_EVAL, c, kind, _dev(bad.astype(np.int32)), 257, out_l, out_k, n_bad, ws, nbytes) == 0
    assert int(n_bad.cpu()) == 3
    # the divisor stays m: the loss is the good rows' sum over 257 (times C for bce)
    l64, _, counts = TW.head_reference(z[good], y[good], loss, np.float64, divisor_rows=257)
    l32, _, _ = TW.head_reference(z[good], y[good], loss, np.float32, divisor_rows=257)
    assert abs(float(out_l) - l64) <= K.gate(abs(l32 - l64), np.float64(l64))
    assert np.array_equal(out_k.cpu().numpy(), counts)
    assert _raw_eval(zd, c, yd, c, N_EVAL, c, kind, _dev(rows.astype(np.int32)), 257, out_l, out_k, None, ws, nbytes) == 0


@pytest.mark.parametrize("c", [2, 5, 8])
def test_eval_head_wide_agrees_with_the_confusion_matrix(c):
    from linkteller_amd import engine
    z, y = _eval_inputs(c, "ce", seed=2)
    assert TW.ce_margin_rows(z.astype(np.float64)) == 0
    rows = _lists()[513]
    for r in (None, rows):
        _, conf = engine.eval_head(_dev(z), _dev(y), rows=r)
        _, counts = engine.eval_head_wide(_dev(z), _dev(y), rows=r, loss="ce")
        conf, counts = conf.cpu().numpy().astype(np.int64), counts.cpu().numpy().astype(np.int64)
        diag = np.diag(conf)
        assert counts[:, 0].sum() == np.trace(conf)
        assert np.array_equal(counts[:, 0], diag)
        assert np.array_equal(counts[:, 1], conf.sum(axis=0) - diag) and np.array_equal(counts[:, 2], conf.sum(axis=1) - diag)


# ---- validated runs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W9", "W65"])
def test_validated_run_over_a_row_list(name):
    """Every epoch's val_loss and val_counts equal eval_head_wide on val_logits bit for bit; best and stop epochs equal the host
    restatement of EarlyStopping on the (non-monotone) loss sequence; restore_best gives the snapshot's bits."""
    from linkteller_amd import engine
    case = _case(name)
    rows = np.random.RandomState(5).randint(0, case["n"], 257)
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params, lr=0.3)
    patience = 2
    tr.attach_validation(case["adj"], _dev(case["x"]), _dev(case["y"]), keep_best=True, patience=patience, rows=rows)
    losses, snaps = [], []
    for e in range(14):
        rec, vl, vc = tr.run_validated_async(1)
        zl = tr.val_logits()
        l, k = engine.eval_head_wide(zl, _dev(case["y"]), rows=rows, loss=case["loss"])
        assert vc.shape == (1, case["C"], 3)
        assert torch.equal(vl[0], l) and torch.equal(vc[0], k), (name, e)
        losses.append(float(vl[0]))
        snaps.append(_host(params))
    best, stop = VR.decide(losses, patience)
    state = tr.val_state()
    print(f"  {name}: val losses {['%.4f' % v for v in losses]}, best {best}, stop {stop}")
    assert any(b > a for a, b in zip(losses, losses[1:])), "the validation loss never rose: raise lr"
    assert (state["best_epoch"], state["stop_epoch"]) == (best, stop)
    assert stop >= 0
    tr.restore_best()
    for a, b in zip(_host(params), snaps[best]):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        tr.attach_validation(case["adj"], _dev(case["x"]), _dev(case["y"]))


def test_run_validated_returns_counts_per_class():
    case = _case("W9")
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params)
    tr.attach_validation(case["adj"], _dev(case["x"]), _dev(case["y"]))      # all rows
    r = tr.run_validated(3)
    assert r["val_counts"].shape == (3, 9, 3) and r["val_loss"].shape == (3,)
    assert (r["val_counts"].sum(axis=(1, 2)) >= case["n"]).all()      # every row adds a tp, or an fp and an fn


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_new_exports_are_present():
    from linkteller_amd import _lib
    lib = _lib.lib()
    for name in ("lt_gcn2_trainer_create_wide", "lt_gcn2_trainer_counts", "lt_gcn2_trainer_hidden",
                 "lt_gcn2_trainer_attach_validation_wide", "lt_eval_head_wide", "lt_eval_head_wide_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.lt_eval_head_wide_workspace_bytes(0, 9) == 0 and lib.lt_eval_head_wide_workspace_bytes(10, 257) == 0
    assert lib.lt_eval_head_wide_workspace_bytes(10, 256) > 0


def _last_error():
    from linkteller_amd import _lib
    return _lib.lib().lt_last_error().decode()


def test_c_abi_refusals():
    from linkteller_amd import _lib, graph, synth
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    n, f = 50, 20
    g = graph.as_hip_graph(K._f32(graph.first_order_gcn(synth.erdos_renyi_graph(n, 100, seed=1))))
    x = _dev(synth.gaussian_features(n, f, seed=1))
    y32 = torch.zeros(n, dtype=torch.int32, device="cuda")
    y8 = torch.zeros((n, 300), dtype=torch.uint8, device="cuda")
    buf = torch.zeros(300 * 300, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()

    def create(labels, ldy, kind, h, c):
        h_ = C.c_void_p()
        rc = lib.lt_gcn2_trainer_create_wide(g.handle, x.data_ptr(), f, f, labels.data_ptr(), ldy, kind, h, c, p, p, p, p, 0.01,
                                             0.0, 0.5, 1, stream, C.byref(h_))
        return rc, h_

    for args, word in (((y32, 0, 0, 257, 9), "H=257"), ((y32, 0, 0, 16, 257), "C=257"), ((y8, 8, 1, 16, 9), "ldy=8"),
                       ((y32, 0, 2, 16, 9), "loss_kind=2")):
        rc, h_ = create(*args)
        assert rc == INVALID and not h_.value and word in _last_error(), (args[1:], _last_error())
    # the narrow create keeps its refusal and its text
    h_ = C.c_void_p()
    rc = lib.lt_gcn2_trainer_create(g.handle, x.data_ptr(), f, f, y32.data_ptr(), 16, 9, p, p, p, p, 0.01, 0.0, 0.5, 1, stream,
                                    C.byref(h_))
    assert rc == INVALID and "lt_gcn2_trainer_create: H=16 C=9 (supported: H <= 256, C <= 8)" in _last_error()
    # attach entry points on the other kind of trainer
    rc, wide = create(y32, 0, 0, 16, 9)
    assert rc == 0
    rc = lib.lt_gcn2_trainer_create(g.handle, x.data_ptr(), f, f, y32.data_ptr(), 16, 2, p, p, p, p, 0.01, 0.0, 0.5, 1, stream,
                                    C.byref(h_))
    assert rc == 0
    narrow = h_
    rows = torch.zeros(4, dtype=torch.int32, device="cuda")
    try:
        assert lib.lt_gcn2_trainer_attach_validation(wide, g.handle, x.data_ptr(), f, n, y32.data_ptr(), 0, 0, stream) == INVALID
        assert lib.lt_gcn2_trainer_attach_validation_rows(wide, g.handle, x.data_ptr(), f, n, y32.data_ptr(), 0, 0, rows.data_ptr(),
                                                          4, stream) == INVALID
        assert lib.lt_gcn2_trainer_attach_validation_wide(narrow, g.handle, x.data_ptr(), f, n, y32.data_ptr(), 0, 0, 0, None, 0,
                                                          stream) == INVALID
        assert "narrow" in _last_error()
        out = torch.zeros((9, 3), dtype=torch.int32, device="cuda")
        assert lib.lt_gcn2_trainer_counts(narrow, out.data_ptr(), stream) == INVALID
        assert lib.lt_gcn2_trainer_counts(wide, out.data_ptr(), stream) == INVALID      # no epoch has run
        z = torch.zeros((n, 9), dtype=torch.float32, device="cuda")
        assert lib.lt_gcn2_trainer_logits(wide, z.data_ptr(), 8, stream) == INVALID     # ldz < C
        assert lib.lt_gcn2_trainer_hidden(wide, z.data_ptr(), 15, stream) == INVALID    # ld < H
    finally:
        lib.lt_gcn2_trainer_destroy(wide)
        lib.lt_gcn2_trainer_destroy(narrow)
    # lt_eval_head_wide
    loss = torch.zeros((), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((9, 3), dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    z = torch.zeros((n, 9), dtype=torch.float32, device="cuda")
    for args in ((z, 9, y32, 0, 0, 9, 0), (z, 9, y32, 0, n, 257, 0), (z, 8, y32, 0, n, 9, 0), (z, 9, y8, 8, n, 9, 1),
                 (z, 9, y32, 0, n, 9, 5)):
        assert _raw_eval(*args, None, 0, loss, cnt, None, ws, ws.numel()) == INVALID, args[1:]
    assert _raw_eval(z, 9, y32, 0, n, 9, 0, rows, 0, loss, cnt, None, ws, ws.numel()) == INVALID      # a list with m <= 0
    assert _raw_eval(z, 9, y32, 0, n, 9, 0, None, 0, loss, cnt, None, ws, 8) == _lib.LT_ERR_WORKSPACE
    assert _raw_eval(z, 9, y32, 0, n, 9, 0, None, 0, loss, cnt, None, ws, ws.numel()) == 0


def test_python_surface_refusals():
    from linkteller_amd import _lib, engine, synth
    case = _case("W9")
    ok = lambda: [_dev(p.copy()) for p in case["params"]]      # noqa: E731
    with pytest.raises(ValueError):
        _trainer(dict(case, y=np.full(case["n"], 9)), ok())                      # a label outside [0, C)
    with pytest.raises(ValueError):
        _trainer(case, ok(), loss="bce")                                         # bce wants [n, C]
    with pytest.raises(ValueError):
        _trainer(dict(case, y=np.full((case["n"], 9), 2)), ok(), loss="bce")     # not 0 / 1
    w = synth.gcn_weights(case["F"], 16, 257, seed=0)
    with pytest.raises(_lib.LinkTellerHipError, match="C=257"):
        _trainer(dict(case, y=np.zeros(case["n"], np.int64)), [_dev(w[k]) for k in ("W1", "b1", "W2", "b2")])
    with pytest.raises(_lib.LinkTellerHipError, match="C <= 8"):
        _trainer(case, ok(), head="narrow")                                      # the narrow head keeps refusing 9 classes
    with pytest.raises(ValueError):
        engine.eval_head_wide(_dev(case["x"]), _dev(case["y"]), loss="mse")

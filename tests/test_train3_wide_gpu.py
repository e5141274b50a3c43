"""The 3-layer trainer with the wide head (lt_gcn3_trainer_create_wide; engine.GCN3Trainer(head="wide")) against
train3_wide_restate.epoch_reference3_wide in fp64, case by case (train3_wide_cases.py): the first width the narrow head
refuses, reddit's and ppi's class counts on a directed and a hub-row graph, the lane-group and GEMM-tile edge at 65 with C > H2,
the limit C = 256 over H2 = 5, one class, p = 1; both losses; the second mask's layer word, large logits, determinism, the
narrow head next to the wide one, validated runs, the reference's trajectory, the C ABI's refusals and exports.

Method of test_train_wide_gpu.py: run the epochs before the checked one, read the parameters back, run one more epoch and
compare it with the reference evaluated AT THE READ-BACK PARAMETERS with that epoch's two masks.  Gate per tensor
(train_cases.gate): err_hip <= 2 err_fp32 + 1e-6 max|ref64| + 1e-12, err_fp32 from the same restatement in float32.  The
gradients are compared with the fp64 derivative of the function the device evaluated: the reference takes the ReLU patterns
hidden(1) > 0 and hidden(2) > 0, which may differ from the fp64 ones only at near-kink elements (asserted)."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_cases as K
import train3_cases as K3
import train3_wide_cases as KT
import train3_wide_restate as TW3
import validate_restate as VR

pytestmark = pytest.mark.gpu

INVALID = -1
FORWARD = ("H1d", "H2d", "Z3")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(ts):
    return [t.cpu().numpy().copy() for t in ts]


def _trainer(case, params, dropout=None, lr=KT.LR, head="wide", loss=None):
    from linkteller_amd import engine
    return engine.GCN3Trainer(case["adj"], _dev(case["x"]), _dev(case["y"]), *params, lr=lr, weight_decay=KT.DECAY,
                              dropout=case["p"] if dropout is None else dropout, seed=KT.SEED, head=head,
                              loss=case["loss"] if loss is None else loss)


_cases, _epochs = {}, {}


def _case(name, h2=None):
    if (name, h2) not in _cases:
        _cases[name, h2] = KT.make(name, h2=h2)
    return _cases[name, h2]


def _read(tr, loss, tp):
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(KT.NAMES, tr.grads())}
    got["Z3"] = tr.logits().cpu().numpy().astype(np.float64)
    got["H1d"], got["H2d"] = (tr.hidden(k).cpu().numpy().astype(np.float64) for k in (1, 2))
    if tr.head == "wide":
        got["counts"] = tr.counts().cpu().numpy().astype(np.int64)
    got["loss"], got["tp"] = float(loss[0]), int(tp[0])
    return got


def _epoch(name, epoch, h2=None):
    """(case, parameters the checked epoch started from, what the device produced in it); once per (case, epoch)."""
    if (name, epoch, h2) in _epochs:
        return _epochs[name, epoch, h2]
    case = _case(name, h2)
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params)
    if epoch:
        tr.run(epoch)
    start = _host(params)
    loss, tp = tr.run(1)
    assert tr.epoch == epoch + 1
    _epochs[name, epoch, h2] = (case, start, _read(tr, loss, tp))
    return _epochs[name, epoch, h2]


def _gated(tag, keys, got, r64, r32):
    """[(key, err_hip, gate)] of ``keys``, printed; asserts each inside its gate."""
    errs = []
    for k in keys:
        a, b = np.asarray(r64[k], dtype=np.float64), np.asarray(r32[k]).astype(np.float64)
        errs.append((k, float(np.abs(got[k] - a).max()), K.gate(float(np.abs(b - a).max()), a)))
    for k, e, g in errs:
        print(f"  {tag} {k}: err_hip {e:.3e}  gate {g:.3e}  ratio {e / g:.3f}")
    for k, e, g in errs:
        assert np.isfinite(got[k]).all() and e <= g, (tag, k, e, g)
    return errs


def _compare(case, start, epoch, got):
    torch.set_num_threads(1)
    an = KT.analyse(case, start, epoch)
    KT.check_conditions(case, an)
    r64 = an["r64"]
    tag = f"{case['name']} epoch {epoch}"
    on = got["H1d"] > 0, got["H2d"] > 0
    for k, z in ((0, "Z1"), (1, "Z2")):      # the device's ReLU pattern is fp64's outside the near-kink elements
        diff = on[k] != (an["keep"][k] & (r64[z] > 0))
        print(f"  {tag}: layer {k + 1} pattern differs at {int(diff.sum())} elements ({int(an['near'][k].sum())} near-kink)")
        assert not (diff & ~an["near"][k]).any(), (tag, k, int((diff & ~an["near"][k]).sum()))
    _gated(tag, FORWARD + ("loss",), got, r64, an["r32"])
    g64 = TW3.epoch_reference3_wide(*an["args"], np.float64, on1=on[0], on2=on[1])
    g32 = TW3.epoch_reference3_wide(*an["args"], np.float32, on1=on[0], on2=on[1])
    _gated(tag, KT.NAMES, got, g64, g32)
    if "counts" in got:
        assert np.array_equal(got["counts"], r64["counts"]), tag
    assert got["tp"] == int(r64["counts"][:, 0].sum())
    return an


@pytest.mark.parametrize("name,epoch", KT.CASE_EPOCHS, ids=[f"{k}-epoch{e}" for k, e in KT.CASE_EPOCHS])
def test_epoch_against_fp64(name, epoch):
    case, start, got = _epoch(name, epoch)
    _compare(case, start, epoch, got)
    if name == "P1":      # p = 1: nothing is kept, only db3 is not zero, the logits are b3
        assert not got["H1d"].any() and not got["H2d"].any() and all(not got[k].any() for k in KT.NAMES[:5])
        assert np.abs(got["db3"]).max() > 0
        assert np.array_equal(got["Z3"], np.broadcast_to(start[5].astype(np.float64), got["Z3"].shape))


def test_second_mask_is_the_layer_word_1_stream():
    """T9 with H2 = H1 = 30, epoch 2: the logits pass their gate with the layers' own masks and miss it by more than 100x with
    the two restated masks exchanged."""
    torch.set_num_threads(1)
    case, start, got = _epoch("T9", 2, h2=30)
    assert case["H1"] == case["H2"] == 30
    out = {}
    for swap in (False, True):
        an = KT.analyse(case, start, 2, swap=swap)
        r64, r32 = an["r64"], an["r32"]
        out[swap] = float(np.abs(got["Z3"] - r64["Z3"]).max()), K.gate(np.abs(r32["Z3"].astype(np.float64) - r64["Z3"]).max(), r64["Z3"])
    print(f"  own masks {out[False][0]:.3e} (gate {out[False][1]:.3e}); swapped {out[True][0]:.3e} (gate {out[True][1]:.3e})")
    assert out[False][0] <= out[False][1]
    assert out[True][0] > 100 * out[True][1]


def test_bce_at_large_logits():
    """T65 at p = 0 with W3 and b3 scaled by 300: logits beyond |z| = 90.  The loss is finite, every tensor passes its gate,
    nothing is NaN."""
    torch.set_num_threads(1)
    case = dict(_case("T65"), p=0.0)
    case["params"] = case["params"][:4] + [case["params"][4] * np.float32(300), case["params"][5] * np.float32(300)]
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params)
    got = _read(tr, *tr.run(1))
    assert np.abs(got["Z3"]).max() > 90 and np.isfinite(got["loss"])
    an = _compare(case, case["params"], 0, got)
    unit = 1.0 / (case["n"] * case["C"])
    dz = an["r64"]["dZ3"]
    assert int((np.abs(dz) == unit).sum() + (dz == 0).sum()) > 0      # saturated elements


@pytest.mark.parametrize("name", ["T9", "T65"])
def test_deterministic_and_resumable(name):
    """p = 0.5: run(12) equals run(5); run(7), and both equal a second trainer -- record, grads, logits, hidden layers, counts
    and parameters, bit for bit."""
    case = _case(name)
    assert case["p"] == 0.5
    runs = []
    for chunks in ([12], [5, 7], [12]):
        params = [_dev(p.copy()) for p in case["params"]]
        tr = _trainer(case, params)
        rec = np.concatenate([tr.run_async(k).cpu().numpy() for k in chunks])
        assert tr.epoch == 12 and np.isfinite(rec).all()
        runs.append([rec] + _host(tr.grads()) + _host([tr.logits(), tr.hidden(1), tr.hidden(2), tr.counts()]) + _host(params))
    for other in runs[1:]:
        for i, (a, b) in enumerate(zip(runs[0], other)):
            assert np.array_equal(a, b), (name, i)
    assert not np.array_equal(runs[0][-6], case["params"][0]) and not np.array_equal(runs[0][-1], case["params"][5])


@pytest.mark.parametrize("name", ["B3", "A3"])
def test_the_two_heads_meet(name):
    """train3_cases B3 (C = 3) and A3 (C = 8): the narrow and the wide GCN3Trainer each pass the fp64 gate on the hidden layers,
    logits, loss and gradients (each with its own ReLU patterns, both under the same two masks), and count the same correct rows."""
    case = dict(K3.make(name), loss="ce")
    assert case["C"] == {"B3": 3, "A3": 8}[name]
    correct = {}
    for head in ("narrow", "wide"):
        params = [_dev(p.copy()) for p in case["params"]]
        tr = _trainer(case, params, head=head)
        got = _read(tr, *tr.run(1))
        _compare(dict(case, name=f"{name} {head}"), case["params"], 0, got)
        correct[head] = got["tp"]
    assert correct["narrow"] == correct["wide"]


@pytest.mark.parametrize("key,loss", [("ce9", "ce"), ("bce12", "bce")])
def test_trajectory_against_reference(key, loss):
    """tests/golden/train3_wide.npz: 40 epochs of the reference's GCN3, losses and optim.Adam at p = 0 in fp64 and fp32
    (golden/generate_train3_wide.py).  Gate of test_train_gpu.py: twice the reference fp32 run's own deviation from its fp64
    run plus the floor; the tp sums may differ by the rows (elements) the generator found fragile."""
    import scipy.sparse as sp
    from conftest import load_golden
    from linkteller_amd import engine
    gold = load_golden("train3_wide.npz")
    n = gold["x"].shape[0]
    adj = sp.csr_matrix((gold["adj.data"], gold["adj.indices"], gold["adj.indptr"]), shape=(n, n))
    names = [f"gc{k}.{w}" for k in (1, 2, 3) for w in ("weight", "bias")]
    params = [_dev(gold[f"{key}.init.{k}"].copy()) for k in names]
    tr = engine.GCN3Trainer(adj, _dev(gold["x"]), _dev(gold[f"{key}.y"]), *params, lr=float(gold["lr"]),
                            weight_decay=float(gold["decay"]), dropout=0.0, seed=1, head="wide", loss=loss)
    got, tp = tr.run(int(gold["epochs"]))
    l64, l32 = gold[f"{key}.loss64"], gold[f"{key}.loss32"]
    e, g = np.abs(got - l64).max(), 2 * np.abs(l32 - l64).max() + 1e-5
    print(f"  {key}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, |hip - fp64| max {e:.3e}, gate {g:.3e}")
    assert e <= g, (e, g)
    assert np.all(np.abs(tp - gold[f"{key}.tp64"]) <= gold[f"{key}.tiny64"]), (tp, gold[f"{key}.tp64"])
    # the trained parameters: the eval-mode logits they give, formed in fp64 on the host
    w1, b1, w2, b2, w3, b3 = (p.cpu().numpy().astype(np.float64) for p in params)
    a = adj.astype(np.float64)
    h1 = np.maximum(a @ (gold["x"].astype(np.float64) @ w1) + b1, 0)
    z = a @ (np.maximum(a @ (h1 @ w2) + b2, 0) @ w3) + b3
    z64, z32 = gold[f"{key}.logits64"], gold[f"{key}.logits32"]
    assert np.abs(z - z64).max() <= 2 * np.abs(z32 - z64).max() + 1e-5 * np.abs(z64).max(), \
        (np.abs(z - z64).max(), np.abs(z32 - z64).max())


# ---- validated runs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rows", [True, False], ids=["rows", "all"])
@pytest.mark.parametrize("name", ["T9", "T65"])
def test_validated_run(name, with_rows):
    """Every epoch's val_loss and val_counts equal eval_head_wide on val_logits bit for bit; best and stop epochs equal the host
    restatement of EarlyStopping on the (non-monotone) loss sequence; restore_best gives the snapshot's bits."""
    from linkteller_amd import engine
    case = _case(name)
    rows = np.random.RandomState(5).randint(0, case["n"], 257) if with_rows else None
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params, lr=0.3)
    patience = 2
    tr.attach_validation(case["adj"], _dev(case["x"]), _dev(case["y"]), keep_best=True, patience=patience, rows=rows)
    losses, snaps = [], []
    for e in range(14):
        rec, vl, vc = tr.run_validated_async(1)
        zl = tr.val_logits()
        l, k = engine.eval_head_wide(zl, _dev(case["y"]), rows=rows, loss=case["loss"])
        assert vc.shape == (1, case["C"], 3) and zl.shape == (case["n"], case["C"])
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


def test_validation_forward_is_the_eval_mode_model():
    """T41 (directed graph): after two validated epochs, val_logits equals the fp64 eval-mode forward at the updated parameters
    within the gate and the counts are fp64's; run_validated returns [epochs, C, 3] counts.  (Two epochs: the smallest eval-mode
    argmax margin of train3_wide_cases.simulate is then 6.6e-4; after 1, 4 or 5 epochs a row lies below the 1e-4 of the
    condition.)"""
    torch.set_num_threads(1)
    case = _case("T41")
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params)
    tr.attach_validation(case["adj"], _dev(case["x"]), _dev(case["y"]))
    r = tr.run_validated(2)
    assert r["val_counts"].shape == (2, 41, 3) and r["val_loss"].shape == (2,)
    off = dict(case, p=0.0)
    an = KT.analyse(off, _host(params), 0)
    got = {"Z3": tr.val_logits().cpu().numpy().astype(np.float64), "loss": float(r["val_loss"][-1])}
    _gated("T41 validation", ("Z3", "loss"), got, an["r64"], an["r32"])
    assert an["fragile"] == 0 and np.array_equal(r["val_counts"][-1], an["r64"]["counts"])


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_new_exports_are_present():
    from linkteller_amd import _lib
    lib = _lib.lib()
    for name in ("lt_gcn3_trainer_create_wide", "lt_gcn3_trainer_counts", "lt_gcn3_trainer_attach_validation_wide"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.lt_abi_version() == 5


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

    def create(labels, ldy, kind, h1, h2, c, w3=p):
        h_ = C.c_void_p(0xdead)
        rc = lib.lt_gcn3_trainer_create_wide(g.handle, x.data_ptr(), f, f, labels, ldy, kind, h1, h2, c, p, p, p, p, w3, p, 0.01,
                                             0.0, 0.5, 1, stream, C.byref(h_))
        return rc, h_

    for args, word in (((y32.data_ptr(), 0, 0, 257, 16, 9), "H1=257"), ((y32.data_ptr(), 0, 0, 16, 257, 9), "H2=257"),
                       ((y32.data_ptr(), 0, 0, 16, 16, 257), "C=257"), ((y8.data_ptr(), 8, 1, 16, 16, 9), "ldy=8"),
                       ((y32.data_ptr(), 0, 2, 16, 16, 9), "loss_kind=2"), ((None, 0, 0, 16, 16, 9), "NULL"),
                       ((y32.data_ptr(), 0, 0, 16, 16, 9, None), "NULL")):
        rc, h_ = create(*args)
        assert rc == INVALID and not h_.value and word in _last_error() and "lt_gcn3_trainer_create_wide" in _last_error(), \
            (args[1:], _last_error())
    assert not buf.any()      # nothing was written
    # the narrow create keeps its refusal and its text
    h_ = C.c_void_p()
    rc = lib.lt_gcn3_trainer_create(g.handle, x.data_ptr(), f, f, y32.data_ptr(), 16, 16, 9, p, p, p, p, p, p, 0.01, 0.0, 0.5, 1,
                                    stream, C.byref(h_))
    assert rc == INVALID and "lt_gcn3_trainer_create: H1=16 H2=16 C=9 (supported: H1, H2 <= 256, C <= 8)" in _last_error()
    # attach entry points on the other kind of trainer
    rc, wide = create(y32.data_ptr(), 0, 0, 16, 16, 9)
    assert rc == 0
    rc = lib.lt_gcn3_trainer_create(g.handle, x.data_ptr(), f, f, y32.data_ptr(), 16, 16, 2, p, p, p, p, p, p, 0.01, 0.0, 0.5, 1,
                                    stream, C.byref(h_))
    assert rc == 0
    narrow = h_
    rows = torch.zeros(4, dtype=torch.int32, device="cuda")
    try:
        assert lib.lt_gcn3_trainer_attach_validation(wide, g.handle, x.data_ptr(), f, n, y32.data_ptr(), 0, 0, stream) == INVALID
        assert "lt_gcn3_trainer_attach_validation_wide" in _last_error()
        assert lib.lt_gcn3_trainer_attach_validation_rows(wide, g.handle, x.data_ptr(), f, n, y32.data_ptr(), 0, 0, rows.data_ptr(),
                                                          4, stream) == INVALID
        assert "lt_gcn3_trainer_attach_validation_wide" in _last_error()
        assert lib.lt_gcn3_trainer_attach_validation_wide(narrow, g.handle, x.data_ptr(), f, n, y32.data_ptr(), 0, 0, 0, None, 0,
                                                          stream) == INVALID
        assert "narrow" in _last_error() and "lt_gcn3_trainer_attach_validation or _attach_validation_rows" in _last_error()
        out = torch.zeros((9, 3), dtype=torch.int32, device="cuda")
        assert lib.lt_gcn3_trainer_counts(narrow, out.data_ptr(), stream) == INVALID
        assert lib.lt_gcn3_trainer_counts(wide, out.data_ptr(), stream) == INVALID      # no epoch has run
        assert lib.lt_gcn3_trainer_counts(wide, None, stream) == INVALID
        z = torch.zeros((n, 9), dtype=torch.float32, device="cuda")
        assert lib.lt_gcn3_trainer_logits(wide, z.data_ptr(), 8, stream) == INVALID     # ldz < C
        assert not out.any() and not z.any()
    finally:
        lib.lt_gcn3_trainer_destroy(wide)
        lib.lt_gcn3_trainer_destroy(narrow)


def test_python_surface_refusals():
    from linkteller_amd import _lib
    case = _case("T9")
    ok = lambda: [_dev(p.copy()) for p in case["params"]]      # noqa: E731
    with pytest.raises(ValueError):
        _trainer(dict(case, y=np.full(case["n"], 9)), ok())                      # a label outside [0, C)
    with pytest.raises(ValueError):
        _trainer(case, ok(), loss="bce")                                         # bce wants [n, C]
    with pytest.raises(_lib.LinkTellerHipError, match="C <= 8"):
        _trainer(case, ok(), head="narrow")                                      # the narrow head keeps refusing 9 classes
    tr = _trainer(dict(K3.make("F3"), loss="ce"), [_dev(p.copy()) for p in K3.make("F3")["params"]], head="narrow")
    with pytest.raises(ValueError, match="head='wide'"):
        tr.counts()

"""The minibatch MLP trainer (lt_mlp.hip, engine.MLPTrainer, engine.mlp_forward) on the GPU.

One-step check (mlp_cases.py): each checked step runs the steps before it, reads the parameters back, runs the step and compares
its gradients, logits, loss and count with mlp_restate.step_reference evaluated AT THE READ-BACK PARAMETERS under that step's
mask, so no check depends on trajectory drift.  Gate, per tensor: err_hip <= 2 err_fp32 + 1e-6 max|ref64| + 1e-12 with err_fp32
from the same restatement in float32.  Hidden columns with near-kink elements (train_restate.near_kink) are held to the interval
between the fp64 gradients with all of their near-kink derivatives off and all on, widened by the same gate; they are at most
1/8 of H (asserted per case).  Then: the reference's own training run (golden/mlp_train.npz), the Philox order, determinism,
row ids out of range, the full-batch form and lt_mlp_forward."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mlp_cases as K
import mlp_restate as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_train.npz")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(ts):
    return [t.cpu().numpy().copy() for t in ts]


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = K.make(name)
    return _cases[name]


def _trainer(case, params, **kw):
    from linkteller_amd import engine
    args = dict(depth=case["depth"], batch_size=case["B"], lr=K.LR, weight_decay=K.DECAY, dropout=case["p"], seed=K.SEED,
                loss=case["loss"])
    args.update(kw)
    return engine.MLPTrainer(_dev(case["x"]), _dev(case["y"]), *params, **args)


def _step(name, step):
    """Run `step` steps, read the parameters back, run one more: (case, the parameters it started from, what it produced)."""
    case = _case(name)
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params)
    for s in range(step):
        tr.step_async(K.batch_of(case, s))
    start = _host(params)
    rec = tr.step_async(K.batch_of(case, step)).cpu().numpy()
    assert tr.step == step + 1
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(K.names(case["depth"]), tr.grads())}
    got["Z"] = tr.logits().cpu().numpy().astype(np.float64)
    got["loss"], got["count"] = float(rec[0]), int(rec[1])
    return case, start, got


def _errors(case, an, got):
    r64, r32 = an["r64"], an["r32"]
    strict = ~an["kink_cols"]
    out = []
    for i, k in enumerate(K.names(case["depth"])):
        a, b64, b32 = got[k], r64["grads"][i], r32["grads"][i].astype(np.float64)
        b64s = b64
        if k in ("dW1", "db1"):
            a, b64s, b32 = a[..., strict], b64[..., strict], b32[..., strict]
        out.append((k, float(np.abs(a - b64s).max()) if a.size else 0.0, K.gate(np.abs(b32 - b64s).max() if a.size else 0.0, b64)))
    out.append(("Z", float(np.abs(got["Z"] - r64["Z"]).max()), K.gate(np.abs(r32["Z"].astype(np.float64) - r64["Z"]).max(), r64["Z"])))
    out.append(("loss", abs(got["loss"] - r64["loss"]), K.gate(abs(r32["loss"] - r64["loss"]), np.float64(r64["loss"]))))
    return out


def _compare(case, start, step, got):
    an = K.analyse(case, start, step)
    K.check_conditions(case, an)
    assert got["Z"].shape == an["r64"]["Z"].shape
    errs = _errors(case, an, got)
    for k, e, g in errs:
        print(f"  {case['name']} step {step} {k}: err_hip {e:.3e}  gate {g:.3e}  ratio {e / g:.3f}")
    for k, e, g in errs:
        assert e <= g, (case["name"], step, k, e, g)
    cols = an["kink_cols"]
    if cols.any():
        for i, k in enumerate(("dW1", "db1")):
            g = errs[i][2]
            lo = np.minimum(an["off"][i], an["on"][i])[..., cols] - g
            hi = np.maximum(an["off"][i], an["on"][i])[..., cols] + g
            a = got[k][..., cols]
            out = np.maximum(lo - a, a - hi).max()
            print(f"  {case['name']} step {step} {k}: {int(cols.sum())} near-kink columns, outside their interval by {out:.3e}")
            assert out <= 0, (case["name"], step, k, out, g)
    want = an["r64"]["count"]
    print(f"  {case['name']} step {step} count: {got['count']} (fp64 {want}, fragile {an['fragile']})")
    assert abs(got["count"] - want) <= an["fragile"], (got["count"], want, an["fragile"])
    return an


@pytest.mark.parametrize("name,step", K.CASE_STEPS, ids=[f"{k}-step{s}" for k, s in K.CASE_STEPS])
def test_step_against_fp64(name, step):
    case, start, got = _step(name, step)
    an = _compare(case, start, step, got)
    if name == "B":
        assert an["rows"].size == 1
    if name == "I":      # p = 1: nothing is kept
        assert all(not got[k].any() for k in ("dW1", "db1", "dW2")) and np.abs(got["db2"]).max() > 0
        assert np.array_equal(got["Z"], np.broadcast_to(start[3].astype(np.float64), got["Z"].shape))


def test_step_word_reaches_the_counter():
    """Case D, step 4, judged with step 0's mask: the logits miss their gate by more than 100x."""
    case, start, got = _step("D", 4)
    right, wrong = K.analyse(case, start, 4), K.analyse(case, start, 4, mask_step=0)
    z_right, z_wrong = _errors(case, right, got)[4], _errors(case, wrong, got)[4]
    assert z_right[0] == "Z" and z_right[1] <= z_right[2]
    assert z_wrong[1] > 100 * z_wrong[2]


def test_run_equals_its_steps_and_splits():
    """Case D (p = 0.5) under a given order: run(4) == run(1); run(3) == the twenty steps taken one by one, bit for bit:
    record, last gradients, last logits, parameters.  Two trainers agree bit for bit."""
    case = _case("D")
    orders = np.stack([np.random.RandomState(50 + e).permutation(case["n"]) for e in range(4)])
    outs = []
    for how in ("whole", "whole", "split", "steps"):
        params = [_dev(p.copy()) for p in case["params"]]
        tr = _trainer(case, params)
        if how == "whole":
            rec = tr.run_async(4, orders).cpu().numpy()
        elif how == "split":
            rec = np.concatenate([tr.run_async(1, orders[:1]).cpu().numpy(), tr.run_async(3, orders[1:]).cpu().numpy()])
        else:
            rec = np.stack([tr.step_async(b).cpu().numpy() for o in orders for b in M.batches(o, case["B"])])
        assert tr.step == 4 * case["spe"] and tr.epoch == (0 if how == "steps" else 4)
        outs.append((rec, _host(tr.grads()), tr.logits().cpu().numpy(), _host(params)))
    rec0, g0, z0, p0 = outs[0]
    assert np.isfinite(rec0).all() and rec0.shape == (4 * case["spe"], 2)
    assert not np.array_equal(p0[0], case["params"][0])
    for rec, g, z, p in outs[1:]:
        assert np.array_equal(rec, rec0) and np.array_equal(z, z0)
        for a, b in zip(g + p, g0 + p0):
            assert np.array_equal(a, b)


def test_philox_order_and_split_runs():
    """The Philox order read back equals the numpy restatement in epochs 0 and 2 after a run(1); run(2) split; run(4) equals
    run(1); run(3) bit for bit with p = 0.5 under that order; the record's counts are those of the restated batches."""
    case = _case("D")
    p_a = [_dev(p.copy()) for p in case["params"]]
    a = _trainer(case, p_a)
    rec_a = [a.run_async(1).cpu().numpy()]
    o0 = a.last_order().cpu().numpy()
    rec_a.append(a.run_async(2).cpu().numpy())
    o2 = a.last_order().cpu().numpy()
    assert np.array_equal(o0, M.shuffle_order(case["n"], 0, K.SEED))
    assert np.array_equal(o2, M.shuffle_order(case["n"], 2, K.SEED))
    assert np.array_equal(np.sort(o0), np.arange(case["n"])) and not np.array_equal(o0, o2)
    rec_a.append(a.run_async(1).cpu().numpy())
    p_b = [_dev(p.copy()) for p in case["params"]]
    b = _trainer(case, p_b)
    rec_b = b.run_async(4).cpu().numpy()
    assert np.array_equal(np.concatenate(rec_a), rec_b)
    for x, y in zip(_host(p_a), _host(p_b)):
        assert np.array_equal(x, y)
    # the same run with the restated orders given explicitly
    p_c = [_dev(p.copy()) for p in case["params"]]
    c = _trainer(case, p_c)
    rec_c = c.run_async(4, np.stack([M.shuffle_order(case["n"], e, K.SEED) for e in range(4)])).cpu().numpy()
    assert np.array_equal(rec_c, rec_b)


def test_row_id_out_of_range_is_reported_not_read():
    """An int32 device order with one id far outside [0, n): the run completes (row 0 stands in), node_check raises, and a
    clean run afterwards works."""
    from linkteller_amd import _lib, engine
    case = _case("C")
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params)
    order = torch.arange(case["n"], dtype=torch.int32, device="cuda").reshape(1, -1).clone()
    order[0, 5] = 2**30
    rec = tr.run_async(1, order)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rec).all())
    with pytest.raises((IndexError, _lib.LinkTellerHipError)):
        engine.node_check()
    engine.node_check()
    order[0, 5] = 5
    assert np.isfinite(tr.run(1, order)[0]).all()
    engine.node_check()


def test_full_batch_is_one_step_of_the_restatement():
    """batch_size >= n with the identity order (700 rows: two gradient slabs): one step per epoch, gated against the
    restatement's step over all rows."""
    case = dict(_case("A"), B=1000, spe=1)
    case["orders"] = np.arange(case["n"])[None, :]
    params = [_dev(p.copy()) for p in case["params"]]
    tr = _trainer(case, params)
    assert tr.steps_per_epoch == 1
    loss, count = tr.run(1, case["orders"])
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(K.names(2), tr.grads())}
    got["Z"] = tr.logits().cpu().numpy().astype(np.float64)
    got["loss"], got["count"] = float(loss[0]), int(count[0])
    _compare(case, case["params"], 0, got)


@pytest.mark.parametrize("name", ["A", "D", "F", "G", "K"])
def test_forward(name):
    """engine.mlp_forward against the restatement (dropout off) for all rows and for a row list with repeats; with p = 0 a
    step's logits are its bits on the batch's rows."""
    from linkteller_amd import engine
    case = _case(name)
    x = _dev(case["x"])
    params = [_dev(p.copy()) for p in case["params"]]
    rows = np.concatenate([K.batch_of(case, 0)[::3], [0, 0, case["n"] - 1]])
    for r in (None, rows):
        z = engine.mlp_forward(x, *params, depth=case["depth"], rows=r).cpu().numpy().astype(np.float64)
        idx = np.arange(case["n"]) if r is None else r
        args = (case["x"], case["y"], case["params"], idx, case["depth"], case["loss"])
        z64, z32 = M.step_reference(*args, dtype=np.float64)["Z"], M.step_reference(*args, dtype=np.float32)["Z"]
        err, g = np.abs(z - z64).max(), K.gate(np.abs(z32.astype(np.float64) - z64).max(), z64)
        print(f"  {name} forward ({'all' if r is None else 'list'}): err_hip {err:.3e} gate {g:.3e}")
        assert z.shape == z64.shape and err <= g
    batch = K.batch_of(case, 0)
    want = engine.mlp_forward(x, *params, depth=case["depth"], rows=batch)
    tr = _trainer(case, params, dropout=0.0)
    tr.step_async(batch)
    assert torch.equal(tr.logits(), want)


def test_padded_operands_through_the_c_abi():
    """ldx > F (pad columns NaN), ldy > C (pad bytes 255) and ldz > C through lt_mlp_trainer_*: three epochs equal the dense
    run's bits, and the logits' pad columns keep their sentinel."""
    from linkteller_amd import _lib
    n, f, h, c, bsz = 150, 41, 30, 5, 64
    rng = np.random.RandomState(3)
    x = rng.standard_normal((n, f)).astype(np.float32)
    y = (rng.random_sample((n, c)) < 0.4).astype(np.uint8)
    init = [rng.uniform(-0.2, 0.2, s).astype(np.float32) for s in ((f, h), (h,), (h, c), (c,))]
    case = dict(x=x, y=y, depth=2, B=bsz, p=0.5, loss="bce")
    dense_p = [_dev(p.copy()) for p in init]
    dense = _trainer(case, dense_p)
    lib, dev = _lib.lib(), dense_p[0].device
    xp = torch.full((n, 44), float("nan"), dtype=torch.float32, device=dev)
    xp[:, :f] = _dev(x)
    yp = torch.full((n, 8), 255, dtype=torch.uint8, device=dev)
    yp[:, :c] = _dev(y)
    raw_p = [_dev(p.copy()) for p in init]
    handle = C.c_void_p()
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.lt_mlp_trainer_create(xp.data_ptr(), 44, n, f, yp.data_ptr(), 8, 1, 2, h, c, *[t.data_ptr() for t in raw_p],
                                         bsz, K.LR, K.DECAY, 0.5, K.SEED, stream, C.byref(handle)), "lt_mlp_trainer_create")
    try:
        for e in range(3):
            rec_d = dense.run_async(1)
            rec_r = torch.empty((3, 2), dtype=torch.float32, device=dev)
            _lib.check(lib.lt_mlp_trainer_run(handle, 1, None, rec_r.data_ptr(), stream), "lt_mlp_trainer_run")
            grads = [torch.empty_like(p) for p in raw_p]
            _lib.check(lib.lt_mlp_trainer_grads(handle, *[t.data_ptr() for t in grads], stream), "lt_mlp_trainer_grads")
            z = torch.full((n - 2 * bsz, 7), -77.25, dtype=torch.float32, device=dev)
            _lib.check(lib.lt_mlp_trainer_logits(handle, z.data_ptr(), 7, stream), "lt_mlp_trainer_logits")
            torch.cuda.synchronize()
            assert torch.equal(rec_r, rec_d) and bool(torch.isfinite(rec_r).all()), e
            for a, b in zip(grads, dense.grads()):
                assert torch.equal(a, b), e
            assert torch.equal(z[:, :c].contiguous(), dense.logits()), e
            assert bool((z[:, c:] == -77.25).all()), e
            for a, b in zip(raw_p, dense_p):
                assert torch.equal(a, b), e
    finally:
        _lib.check(lib.lt_mlp_trainer_destroy(handle), "lt_mlp_trainer_destroy")


def test_limits_are_refused_with_nothing_allocated():
    """Every documented refusal of lt_mlp_trainer_create: LT_ERR_INVALID, a message naming the value, a NULL handle, and the
    device's free memory as before the call (the accepted shape takes tens of MB).  lt_mlp_forward: LT_ERR_WORKSPACE
    for a short, a missing and a misaligned workspace, with Z untouched."""
    from linkteller_amd import _lib
    lib = _lib.lib()
    n, f = 4096, 3000
    x = torch.zeros((n, f), dtype=torch.float32, device="cuda")
    y = torch.zeros((n,), dtype=torch.int32, device="cuda")
    w = torch.zeros((f * 256,), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def create(depth=2, h=256, c=2, bsz=2048, loss=0, ldy=0, f_=f, n_=n, ldx=f, p=0.0, lr=0.01, wd=0.0, w1=None):
        handle = C.c_void_p()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        rc = lib.lt_mlp_trainer_create(x.data_ptr(), ldx, n_, f_, y.data_ptr(), ldy, loss, depth, h, c,
                                       w.data_ptr() if w1 is None else w1, w.data_ptr(), w.data_ptr(), w.data_ptr(), bsz, lr, wd,
                                       p, 1, st, C.byref(handle))
        msg = lib.lt_last_error().decode()
        torch.cuda.synchronize()
        taken = free0 - torch.cuda.mem_get_info()[0]
        if rc == 0:
            lib.lt_mlp_trainer_destroy(handle)
        return rc, msg, handle.value, taken

    rc, _, h, accepted = create()
    assert rc == 0 and h and accepted > (8 << 20)      # the accepted shape does allocate: slabs, moments, batch buffers
    for kw, word in ((dict(h=257), "H=257"), (dict(h=0), "H=0"), (dict(c=257), "C=257"), (dict(c=0), "C=0"),
                     (dict(bsz=0), "batch_size=0"), (dict(depth=3), "depth=3"), (dict(depth=0), "depth=0"),
                     (dict(loss=2), "loss_kind=2"), (dict(loss=1, ldy=1), "ldy=1"), (dict(n_=0), "n=0"), (dict(f_=0), "F=0"),
                     (dict(ldx=f - 1), f"ldx={f - 1}"), (dict(p=1.5), "dropout=1.5"), (dict(p=-0.1), "dropout=-0.1"),
                     (dict(lr=-1.0), "lr=-1"), (dict(wd=-1.0), "weight_decay=-1"), (dict(w1=0), "NULL")):
        rc, msg, h, taken = create(**kw)
        # (free memory is the device's: a quarter of the accepted figure leaves room for another process's small change)
        assert rc == -1 and word in msg and not h and taken < accepted // 4, (kw, rc, msg, taken)

    wz = torch.zeros((f * 16,), dtype=torch.float32, device="cuda")
    need = lib.lt_mlp_forward_workspace_bytes(n, f, 2, 16, 2)
    assert need == 6 * n * 16 * 4 and lib.lt_mlp_forward_workspace_bytes(n, f, 2, 257, 2) == 0
    ws = torch.zeros((need + 64,), dtype=torch.uint8, device="cuda")
    z = torch.full((n, 2), -77.25, dtype=torch.float32, device="cuda")

    def forward(ws_ptr, ws_bytes):
        rc = lib.lt_mlp_forward(x.data_ptr(), f, n, f, 2, 16, 2, wz.data_ptr(), wz.data_ptr(), wz.data_ptr(), wz.data_ptr(), None,
                                0, z.data_ptr(), 2, ws_ptr, ws_bytes, st)
        return rc, lib.lt_last_error().decode()

    for ptr, size in ((ws.data_ptr(), need - 1), (None, need), (ws.data_ptr() + 4, need)):
        rc, msg = forward(ptr, size)
        torch.cuda.synchronize()
        assert rc == -4 and str(need) in msg and bool((z == -77.25).all()), (rc, msg)
    assert forward(ws.data_ptr(), need)[0] == 0
    torch.cuda.synchronize()
    assert bool((z == 0).all())


# ---- the reference's own run ------------------------------------------------------------------------------------------------

def _golden_params(g, key, tag, depth, dtype):
    """state_dict arrays ([out, in]) -> the project's [in, out] parameter list."""
    names = ("W1", "W2") if depth == 2 else ("W",)
    out = []
    for nm in names:
        out += [np.ascontiguousarray(g[f"{key}.{tag}.{nm}.weight"].T).astype(dtype), g[f"{key}.{tag}.{nm}.bias"].astype(dtype)]
    return out


@pytest.mark.parametrize("key,depth,loss", [("d2.h16", 2, "ce"), ("d2.h64", 2, "ce"), ("d2.h16.ml5", 2, "bce"), ("d1", 1, "ce")])
def test_against_the_reference_run(key, depth, loss):
    """The per-step loss trajectory and the final parameters against the reference's fp64 run, within twice the deviation of
    the reference's own fp32 run plus the floor; counts equal the fp64 run's up to its fragile predictions."""
    from linkteller_amd import engine
    g = np.load(GOLDEN)
    params = [_dev(p) for p in _golden_params(g, key, "init", depth, np.float32)]
    y = g["y2"] if loss == "ce" else g["y5"]
    tr = engine.MLPTrainer(_dev(g["x"]), _dev(y), *params, depth=depth, batch_size=int(g["batch"]), lr=float(g["lr"]),
                           weight_decay=float(g["decay"]), dropout=0.0, seed=1, loss=loss)
    got_loss, got_count = tr.run(g["orders"].shape[0], g["orders"])
    l64, l32 = g[f"{key}.loss64"], g[f"{key}.loss32"]
    err, gate = np.abs(got_loss.astype(np.float64) - l64).max(), K.gate(np.abs(l32 - l64).max(), l64)
    print(f"  {key} loss: err_hip {err:.3e} gate {gate:.3e}")
    assert got_loss.shape == l64.shape and err <= gate
    assert (np.abs(got_count - g[f"{key}.count64"]) <= g[f"{key}.tiny64"]).all()
    f64, f32 = _golden_params(g, key, "final64", depth, np.float64), _golden_params(g, key, "final32", depth, np.float64)
    for p, a, b in zip(_host(params), f64, f32):
        err, gate = np.abs(p.astype(np.float64) - a).max(), K.gate(np.abs(b - a).max(), a)
        print(f"  {key} final {p.shape}: err_hip {err:.3e} gate {gate:.3e}")
        assert err <= gate

"""The baseline attacks' scores on the GPU: lt_corr_square / lt_corr_pairs (engine.corr_square / corr_pairs) against the shared
restatement (tests/corr_restate.py), and the Attacker's ``baseline_scores = "device"`` route end to end.

Value gate: |float64(got) - restatement| <= 2^-25 + 1e-12 on every cell -- half an fp32 ulp at |s| <= 1 (the one rounding of the
store) plus the slack between two fp64 summation orders on inputs that pass ``corr_restate.well_conditioned`` (asserted per case).
An fp32 Gram errs by 1e-7 and more on these inputs.  The square equals its transpose bit for bit, two calls give equal bits.

Split-K: the Gram's K is cut into corr_slices(k, D) slices of whole 16-column steps (lt_corr.hip).  (k, D) = (64, 259) is the
uneven case: one lower tile -> 16 slices wanted, 17 steps -> 2 steps per slice, 9 slices, the last of ONE step holding the 3-column
K tail; (64, 3170) has 199 steps -> 13 per slice, 16 slices, the last of 4."""
import argparse
import os
import types

import numpy as np
import pytest
import torch

import abi_views as av
import corr_restate as R
from conftest import GOLDEN, csr_from

pytestmark = pytest.mark.gpu

KS = [1, 2, 15, 16, 17, 63, 64, 65, 130]
DS = [1, 2, 3, 4, 5, 7, 63, 64, 65, 259]
N_ROWS = 200
NAN_BITS = 0x7FC00000


def _inputs(D):
    """{name: V [N_ROWS, D] float32}, built once per D and shared by the square and the pair tests (never written to)."""
    hit = _INPUTS.get(D)
    if hit is None:
        rng = np.random.RandomState(1000 + D)
        hit = {"normal": R.normal_rows(rng, N_ROWS, D)}
        if D in (2, 7):
            hit["softmax"] = R.softmax_rows(rng, N_ROWS, D)
        if D >= 63:
            hit["indicator"] = R.indicator_rows(rng, N_ROWS, D)
        for v in hit.values():
            v.setflags(write=False)
        _INPUTS[D] = hit
    return hit


_INPUTS = {}


def _gate(got, exp, tag):
    got = np.asarray(got)
    assert got.dtype == np.float32, tag
    assert np.array_equal(np.isnan(got), np.isnan(exp)), tag
    ok = ~np.isnan(exp)
    err = float(np.abs(got.astype(np.float64)[ok] - exp[ok]).max()) if ok.any() else 0.0
    assert err <= R.GATE, (tag, err, R.GATE)
    return err


def _square(gpu, V, nodes):
    """two engine calls: equal bits, symmetric bit for bit; returns (host square, info dict)"""
    from linkteller_amd import engine
    vt = torch.from_numpy(np.array(V)).to(gpu)
    nt = torch.from_numpy(np.asarray(nodes, dtype=np.int32)).to(gpu)
    a, ia = engine.corr_square(vt, nt)
    b, ib = engine.corr_square(vt, nt)
    assert a.shape == (len(nodes), len(nodes)) and a.dtype == torch.float32
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ia.raw, ib.raw)
    assert torch.equal(a.view(torch.int32), a.t().contiguous().view(torch.int32))
    return a.cpu().numpy(), ia.check()


@pytest.mark.parametrize("k", KS)
def test_square_against_the_restatement(gpu, k):
    worst = 0.0
    for D in DS:
        for name, V in _inputs(D).items():
            rng = np.random.RandomState(11 * k + D)
            nodes = rng.permutation(N_ROWS)[:k]
            tag = f"k={k} D={D} {name}"
            got, info = _square(gpu, V, nodes)
            exp = R.square(V, nodes)
            if k == 1:                                  # the one row IS the mean: 0 / 0
                assert np.isnan(got).all() and info == {"zero_norm": 1, "bad_ids": 0}, tag
                continue
            if k == 2 or D == 1:
                # two rows centre to (t, -t); one column leaves a sign: every score is +-1 whatever the conditioning -- unless a
                # centred row is exactly zero, which the restatement reports as NaN alike
                assert info["bad_ids"] == 0, tag
            else:
                assert R.well_conditioned(V, nodes), tag
                assert info == {"zero_norm": 0, "bad_ids": 0}, tag
            worst = max(worst, _gate(got, exp, tag))
    print(f"k={k}: worst |got - restatement| = {worst:.3e} (gate {R.GATE:.3e})")


def test_square_feature_width(gpu):
    """(64, 3170): the twitch-RU feature width, 16 uneven K slices; (130, 3170): six tiles; standardised 0/1 indicator rows."""
    rng = np.random.RandomState(31)
    V = R.indicator_rows(rng, 160, 3170, density=0.05)
    for k in (64, 130):
        nodes = rng.permutation(160)[:k]
        assert R.well_conditioned(V, nodes)
        got, info = _square(gpu, V, nodes)
        assert info == {"zero_norm": 0, "bad_ids": 0}
        err = _gate(got, R.square(V, nodes), f"k={k} D=3170")
        f32 = float(np.abs(R.fp32_square(V, nodes) - R.square(V, nodes)).max())
        print(f"k={k} D=3170: |got - restatement| = {err:.3e}, the fp32 host route errs by {f32:.3e}")


def test_square_repeated_ids(gpu):
    V = _inputs(65)["normal"]
    nodes = np.array([5, 9, 5, 120, 9, 9, 33, 2, 199, 0, 5, 77, 78, 79, 80, 81, 82], dtype=np.int64)
    assert R.well_conditioned(V, nodes)
    got, info = _square(gpu, V, nodes)
    assert info == {"zero_norm": 0, "bad_ids": 0}
    _gate(got, R.square(V, nodes), "repeated ids")
    assert np.array_equal(got[0].view(np.int32), got[2].view(np.int32)) and np.array_equal(got[1].view(np.int32), got[5].view(np.int32))


# ---- layout: the C ABI on windows of larger buffers --------------------------------------------------------------------------------
def _raw_square(gpu, vview, n, D, nodes, oview):
    from linkteller_amd import _lib, engine
    nt = torch.from_numpy(np.asarray(nodes, dtype=np.int32)).to(gpu)
    k = int(nt.numel())
    info = torch.full((4,), -1, dtype=torch.int64, device=gpu)
    ws = engine._workspace(_lib.lib().lt_corr_workspace_bytes(n, D, k, 0), gpu)
    _lib.check(_lib.lib().lt_corr_square(vview.assert_aligned(), vview.ld, n, D, nt.data_ptr(), k, oview.assert_aligned(), oview.ld,
                                         info.data_ptr(), ws.data_ptr(), ws.numel(), engine._stream()), "lt_corr_square")
    torch.cuda.synchronize()
    return oview.body(), [int(x) for x in info.cpu().tolist()]


@pytest.mark.parametrize("k,D", [(17, 7), (65, 65), (130, 259)])
def test_square_strided_unaligned_operands(gpu, k, D):
    """ldv > D with NaN pad columns (a pad that reaches arithmetic shows as NaN), the base pointer 4 bytes off a 16-byte boundary,
    ldo > k with sentinel pads that must survive."""
    V = _inputs(D)["normal"]
    nodes = np.random.RandomState(k + D).permutation(N_ROWS)[:k]
    exp = R.square(V, nodes)
    for off_v, off_o in ((1, 0), (0, 1), (1, 3)):
        vv = av.View(np.array(V), ld=D + 5, off=off_v)
        ov = av.View.output(k, k, ld=k + 3, off=off_o, fill=-7.0)
        assert vv.ptr % 16 == (4 * off_v) % 16
        got, info = _raw_square(gpu, vv, N_ROWS, D, nodes, ov)
        assert info == [0, 0, 0, 0]
        _gate(got, exp, f"k={k} D={D} off={off_v},{off_o}")
        assert np.array_equal(got.view(np.int32), got.T.copy().view(np.int32))
        assert ov.pads_untouched(), ov.touched_pads()[:8]
        assert vv.pads_untouched()


def test_pairs_strided_unaligned_operands(gpu):
    from linkteller_amd import _lib, engine
    rng = np.random.RandomState(12)
    for D in (7, 65):
        V = _inputs(D)["normal"]
        u, v = rng.randint(0, N_ROWS, 300), rng.randint(0, N_ROWS, 300)
        vv = av.View(np.array(V), ld=D + 3, off=1)
        ut, vt = (torch.from_numpy(x.astype(np.int32)).to(gpu) for x in (u, v))
        out = torch.full((300 + 8,), -7.0, dtype=torch.float32, device=gpu)
        info = torch.full((4,), -1, dtype=torch.int64, device=gpu)
        ws = engine._workspace(_lib.lib().lt_corr_workspace_bytes(N_ROWS, D, 0, 300), gpu)
        _lib.check(_lib.lib().lt_corr_pairs(vv.assert_aligned(), vv.ld, N_ROWS, D, ut.data_ptr(), vt.data_ptr(), 300,
                                            out.data_ptr() + 4, info.data_ptr(), ws.data_ptr(), ws.numel(), engine._stream()), "lt_corr_pairs")
        torch.cuda.synchronize()
        h = out.cpu().numpy()
        assert h[0] == -7.0 and (h[301:] == -7.0).all() and [int(x) for x in info.cpu().tolist()] == [0, 0, 0, 0]
        _gate(h[1:301], R.pairs(V, u, v), f"pairs D={D} strided")
        assert vv.pads_untouched()


# ---- the pair lists --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 4097])
def test_pairs_against_the_restatement(gpu, m):
    """D = 2, 7: eight lanes per pair; D = 65, 259: a wave per pair; D = 64: the last packed width.  u == v is in every list."""
    from linkteller_amd import engine
    for D in (2, 7, 64, 65, 259):
        for name, V in _inputs(D).items():
            tag = f"m={m} D={D} {name}"
            # (two-class softmax rows centre to (t, -t): every score is +-1 whatever the conditioning)
            assert R.well_conditioned(V) or (D == 2 and name == "softmax"), tag
            rng = np.random.RandomState(m + D)
            u, v = rng.randint(0, N_ROWS, m), rng.randint(0, N_ROWS, m)
            v[0] = u[0]                                                    # the reference's balanced-full sample produces u == v
            vt = torch.from_numpy(np.array(V)).to(gpu)
            ut, wt = (torch.from_numpy(x.astype(np.int32)).to(gpu) for x in (u, v))
            a, ia = engine.corr_pairs(vt, ut, wt)
            b, ib = engine.corr_pairs(vt, ut, wt)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ia.raw, ib.raw), tag
            assert ia.check() == {"zero_norm": 0, "bad_ids": 0}, tag
            got = a.cpu().numpy()
            _gate(got, R.pairs(V, u, v), tag)
            assert abs(float(got[0]) - 1.0) <= R.GATE, tag


# ---- degenerate inputs -------------------------------------------------------------------------------------------------------------------
def test_constant_matrix_is_all_nan(gpu):
    from linkteller_amd import engine
    V = np.full((50, 9), 0.3, dtype=np.float32)
    for k in (5, 17, 40):
        got, info = _square(gpu, V, np.arange(k))
        assert np.isnan(got).all() and info == {"zero_norm": k, "bad_ids": 0}
    vt = torch.from_numpy(V).to(gpu)
    idx = torch.arange(20, dtype=torch.int32, device=gpu)
    out, info = engine.corr_pairs(vt, idx, idx.flip(0))
    assert torch.isnan(out).all() and info.check() == {"zero_norm": 20, "bad_ids": 0}
    with pytest.raises(ValueError, match="zero-norm"):
        info.check(nan_ok=False)


def test_a_duplicated_constant_row_among_normal_ones(gpu):
    """Small-integer rows in +- pairs plus one all-zero row listed twice: every column sum is exact and zero, so the zero row's
    centred vector is exactly zero -- its rows and columns are NaN (info[0] == 2), every other cell passes the gate."""
    rng = np.random.RandomState(8)
    half = np.round(rng.standard_normal((20, 11)) * 4).astype(np.float32)
    half[(half == 0).all(axis=1)] = 1.0
    V = np.concatenate([half, -half, np.zeros((1, 11), dtype=np.float32)])
    nodes = np.r_[np.arange(40), 40, 40][rng.permutation(42)]
    got, info = _square(gpu, V, nodes)
    assert info == {"zero_norm": 2, "bad_ids": 0}
    exp = R.square(V, nodes)
    z = nodes == 40
    assert np.isnan(exp[z]).all() and np.isnan(exp[:, z]).all() and not np.isnan(exp[~z][:, ~z]).any()
    assert R.well_conditioned(V, nodes)
    _gate(got, exp, "duplicated constant row")


def test_out_of_range_ids(gpu):
    """Each runs once; a bad id is never an address (its row is staged as zeros), so nothing is provoked.  Its cells are NaN, the
    engine raises IndexError, every other cell is the correlation over the valid listed rows, and the pads stay."""
    from linkteller_amd import engine
    D, k = 65, 70
    V = _inputs(D)["normal"]
    nodes = np.random.RandomState(4).permutation(N_ROWS)[:k].astype(np.int64)
    bad = np.array([3, 66])
    listed = nodes.copy()
    listed[3], listed[66] = N_ROWS, -1
    vv = av.View(np.array(V), ld=D + 1, off=0)
    ov = av.View.output(k, k, ld=k + 2, off=0, fill=-7.0)
    got, info = _raw_square(gpu, vv, N_ROWS, D, listed, ov)
    assert info == [0, 2, 0, 0] and ov.pads_untouched()
    good = np.setdiff1d(np.arange(k), bad)
    assert np.isnan(got[bad]).all() and np.isnan(got[:, bad]).all()
    _gate(got[np.ix_(good, good)], R.square(V, nodes[good]), "valid rows next to bad ids")
    vt = torch.from_numpy(np.array(V)).to(gpu)
    out, ci = engine.corr_square(vt, torch.from_numpy(listed.astype(np.int32)).to(gpu))
    with pytest.raises(IndexError, match="2 node ids"):
        ci.check()
    u = np.array([0, 5, N_ROWS, 7, -1], dtype=np.int32)
    v = np.array([1, -4, 2, 7, 2 ** 31 - 1], dtype=np.int32)
    out, ci = engine.corr_pairs(vt, torch.from_numpy(u).to(gpu), torch.from_numpy(v).to(gpu))
    h = out.cpu().numpy()
    assert np.isnan(h[[1, 2, 4]]).all() and [int(x) for x in ci.raw.cpu().tolist()] == [0, 4, 0, 0]
    _gate(h[[0, 3]], R.pairs(V, [0, 7], [1, 7]), "valid pairs next to bad ids")
    with pytest.raises(IndexError, match="4 node ids"):
        ci.check()


def test_wrapper_checks_and_empty_input(gpu):
    from linkteller_amd import _lib, engine
    vt = torch.zeros((8, 3), dtype=torch.float32, device=gpu)
    idx = torch.zeros(4, dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.LinkTellerHipError):
        engine.corr_square(vt.cpu(), idx)
    with pytest.raises(_lib.LinkTellerHipError):
        engine.corr_pairs(vt, idx.cpu(), idx)
    with pytest.raises(TypeError):
        engine.corr_square(vt.double(), idx)
    with pytest.raises(TypeError):
        engine.corr_square(vt, idx.long())
    with pytest.raises(ValueError):
        engine.corr_pairs(vt, idx, idx[:3])
    with pytest.raises(ValueError):
        engine.corr_square(vt.t(), idx)                                    # last-dimension stride 1
    out, info = engine.corr_square(vt, idx[:0])
    assert out.shape == (0, 0) and info.check() == {"zero_norm": 0, "bad_ids": 0}
    out, info = engine.corr_pairs(vt, idx[:0], idx[:0])
    assert out.shape == (0,) and info.check() == {"zero_norm": 0, "bad_ids": 0}
    # a strided view: the columns 1 .. 3 of a wider matrix
    rng = np.random.RandomState(2)
    W = rng.standard_normal((40, 6)).astype(np.float32)
    view = torch.from_numpy(W).to(gpu)[:, 1:4]
    assert view.stride(0) == 6 and not view.is_contiguous()
    nodes = np.arange(0, 40, 3)
    out, info = engine.corr_square(view, torch.from_numpy(nodes.astype(np.int32)).to(gpu))
    _gate(out.cpu().numpy(), R.square(W[:, 1:4], nodes), "strided view")


# ---- golden ----------------------------------------------------------------------------------------------------------------------------
def _world(gpu, prefix_adj, xkey):
    from linkteller_amd import graph
    g = np.load(os.path.join(GOLDEN, "next_rows.npz"), allow_pickle=False)
    a = csr_from(g, prefix_adj)
    x = torch.from_numpy(g[xkey]).to(gpu)
    adj_t = graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(a)).to(gpu)
    return g, types.SimpleNamespace(features_2=x, adj_2=adj_t, adj_ori=a, n_nodes=a.shape[0])


def _golden_model(gpu, g):
    from linkteller_amd.gcn import GCN
    model = GCN(64, 32, 2, 0.5)
    model.load_state_dict({k: torch.from_numpy(g[f"sd.{k}"]) for k in ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias")})
    return model.to(gpu).eval()


def _args(**kw):
    base = dict(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=40, sample_seed=42, influence=1e-4, mode="vanilla-clean",
                attack_mode="baseline-feat", baseline_scores="device")
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize("mode", ["baseline-feat", "baseline"])
def test_golden_sample(gpu, tmp_path, monkeypatch, mode):
    """The device route's result file at the golden sample (n_test = 40): within ref_err + 2^-25 of the reference's fp32 scores,
    ref_err the golden's own distance from the restatement; with two classes every score is +-1 with the restatement's sign."""
    from linkteller_amd.attacker import Attacker
    g, w = _world(gpu, "adj", "x")
    monkeypatch.chdir(tmp_path)
    atk = Attacker(_args(attack_mode=mode), _golden_model(gpu, g), w)
    atk.prepare_test_data()
    nodes = np.asarray(atk.test_nodes, dtype=np.int64)
    assert np.array_equal(nodes, g[f"{mode}.test_nodes"])
    atk.baseline_attack()
    saved = torch.load(atk.result_filename(), weights_only=False)
    pred, y = np.asarray(saved["result"]["pred"], dtype=np.float64), np.asarray(saved["result"]["y"])
    gold = np.r_[g[f"{mode}.norm_exist"], g[f"{mode}.norm_nonexist"]]
    assert pred.shape == gold.shape and int(y.sum()) == g[f"{mode}.norm_exist"].size
    V = atk._baseline_vectors_device().cpu().numpy()
    sq = R.square(V, nodes)
    ind = np.full(int(nodes.max()) + 1, -1, dtype=np.int64)
    ind[nodes] = np.arange(len(nodes))
    pairs = np.concatenate([np.asarray(atk.exist_edges).reshape(-1, 2), np.asarray(atk.nonexist_edges).reshape(-1, 2)])
    exp = sq[ind[pairs[:, 0]], ind[pairs[:, 1]]]
    if mode == "baseline-feat":
        assert R.well_conditioned(V, nodes)
        ref_err = float(np.abs(gold - exp).max())
        err = float(np.abs(pred - gold).max())
        print(f"{mode}: |device - golden| = {err:.3e}, ref_err = {ref_err:.3e}")
        assert err <= ref_err + 2.0 ** -25
        assert float(np.abs(pred - exp).max()) <= R.GATE
    else:
        assert V.shape[1] == 2
        assert np.abs(np.abs(pred) - 1.0).max() <= 1e-6 and np.array_equal(np.sign(pred), np.sign(exp))
        assert np.abs(np.abs(gold) - 1.0).max() <= 1e-6 and np.array_equal(np.sign(pred), np.sign(gold))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def _wide_model(gpu):
    """64 -> 32 -> 7: posteriors of seven classes (two classes leave only a sign)."""
    from linkteller_amd.gcn import GCN
    torch.manual_seed(5)
    return GCN(64, 32, 7, 0.5).to(gpu).eval()


def _sk_curves(y, s):
    from sklearn import metrics as skm
    s64 = np.asarray(s).astype(np.float64)
    fpr, tpr, thr = skm.roc_curve(y, s64)
    precision, recall, thr2 = skm.precision_recall_curve(y, s64)
    return {"auc": {"fpr": fpr, "tpr": tpr, "thresholds": thr}, "pr": {"precision": precision, "recall": recall, "thresholds": thr2}}


def _curves_equal(c, exp):
    for side, keys in (("auc", ("fpr", "tpr", "thresholds")), ("pr", ("precision", "recall", "thresholds"))):
        for k in keys:
            got, want = c[side][k], exp[side][k]
            assert got.dtype == want.dtype == np.float64 and np.array_equal(got, want), (side, k)


@pytest.mark.parametrize("mode", ["baseline", "baseline-feat"])
@pytest.mark.parametrize("prep", ["host", "device"])
def test_evaluate_unbalanced(gpu, tmp_path, monkeypatch, mode, prep):
    """evaluate(curves=True) on the square: the six arrays sklearn gives on the device's own scores read back, bit for bit; the
    result file of baseline_attack() has the host route's schema and scores within the gate of the restatement; recover_edges()
    equals its host restatement on the read-back square."""
    from curve_restate import ap_bound
    from test_recover_gpu import _check_recovered
    from linkteller_amd import engine
    from linkteller_amd.attacker import Attacker
    g, w = _world(gpu, "adj", "x")
    monkeypatch.chdir(tmp_path)
    args = _args(attack_mode=mode, n_test=48)
    atk = Attacker(args, _wide_model(gpu), w)
    atk.prepare_test_data(pairs=prep)
    nodes = np.asarray(atk.test_nodes, dtype=np.int64)
    out = atk.evaluate(curves=True)
    assert not os.path.exists("eval_twitch")                                # evaluate writes nothing
    V = atk._baseline_vectors_device()
    sq, ci = engine.corr_square(V, torch.from_numpy(nodes.astype(np.int32)).to(gpu))
    sq = sq.cpu().numpy()
    ci.check()
    ex, nex = np.asarray(atk.exist_edges).reshape(-1, 2), np.asarray(atk.nonexist_edges).reshape(-1, 2)
    ind = np.full(int(nodes.max()) + 1, -1, dtype=np.int64)
    ind[nodes] = np.arange(len(nodes))
    pairs = np.concatenate([ex, nex])
    s = sq[ind[pairs[:, 1]], ind[pairs[:, 0]]]
    y = np.r_[np.ones(len(ex), dtype=np.int64), np.zeros(len(nex), dtype=np.int64)]
    assert out["n_pos"] == len(ex) and out["n_neg"] == len(nex)
    _curves_equal(out["curves"], _sk_curves(y, s))
    # the result file: the host route's schema, the device's scores
    atk.baseline_attack()
    dev_file = torch.load(atk.result_filename(), weights_only=False)
    assert abs(atk.auc - out["auc"]) <= ap_bound(out["n_thresholds"]) and abs(atk.ap - out["ap"]) <= ap_bound(out["n_thresholds"])
    os.remove(atk.result_filename())
    args.baseline_scores = "host"
    atk.baseline_attack()
    host_file = torch.load(atk.result_filename(), weights_only=False)
    args.baseline_scores = "device"
    assert sorted(dev_file) == sorted(host_file) == ["auc", "pr", "result"]
    for side in ("auc", "pr", "result"):
        assert sorted(dev_file[side]) == sorted(host_file[side])
    assert dev_file["result"]["y"] == host_file["result"]["y"]
    pred = np.asarray(dev_file["result"]["pred"])
    assert pred.dtype == np.float64 and np.array_equal(pred, s.astype(np.float64))
    Vh = V.cpu().numpy()
    assert R.well_conditioned(Vh, nodes)
    exp = R.square(Vh, nodes)[ind[pairs[:, 0]], ind[pairs[:, 1]]]
    assert float(np.abs(pred - exp).max()) <= R.GATE
    host_pred = np.asarray(host_file["result"]["pred"])
    print(f"{mode}: |device - restatement| = {np.abs(pred - exp).max():.3e}, |host fp32 - restatement| = {np.abs(host_pred - exp).max():.3e}")
    # recover_edges on the square
    rec = atk.recover_edges(beliefs=[0.5, 0.05])
    _check_recovered(atk, rec, sq, w.adj_ori, [0.5, 0.05])


def test_recover_edges_refuses_a_zero_norm_row(gpu):
    """Constant features: every centred row is zero, the square is NaN, and recover_edges raises instead of ranking NaNs (the set
    lt_top_pairs_lower selects from a matrix holding NaNs is unspecified)."""
    from linkteller_amd.attacker import Attacker
    g, w = _world(gpu, "adj", "x")
    w.features_2 = torch.full_like(w.features_2, 0.25)
    atk = Attacker(_args(attack_mode="baseline-feat", n_test=24), None, w)
    atk.prepare_test_data()
    with pytest.raises(ValueError, match="zero-norm"):
        atk.recover_edges(beliefs=[0.1])


@pytest.mark.parametrize("mode", ["baseline", "baseline-feat"])
@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_evaluate_balanced_full(gpu, tmp_path, monkeypatch, mode, rng):
    from linkteller_amd import engine
    from linkteller_amd.attacker import Attacker
    g, w = _world(gpu, "bf.adj", "bf.x")
    monkeypatch.chdir(tmp_path)
    args = _args(attack_mode=mode, sample_type="balanced-full", n_test=7, sample_seed=82)
    atk = Attacker(args, _wide_model(gpu), w)
    atk.prepare_test_data(rng=rng)
    out = atk.evaluate(curves=True)
    if rng == "philox":
        assert "_exist_edges" not in atk.__dict__                           # the pair lists never left the device
    ex, nex = np.asarray(atk.exist_edges).reshape(-1, 2), np.asarray(atk.nonexist_edges).reshape(-1, 2)
    pairs = np.concatenate([ex, nex])
    V = atk._baseline_vectors_device()
    u, v = (torch.from_numpy(np.ascontiguousarray(pairs[:, c], dtype=np.int32)).to(gpu) for c in (0, 1))
    s, ci = engine.corr_pairs(V, u, v)
    s = s.cpu().numpy()
    ci.check()
    y = np.r_[np.ones(len(ex), dtype=np.int64), np.zeros(len(nex), dtype=np.int64)]
    _curves_equal(out["curves"], _sk_curves(y, s))
    Vh = V.cpu().numpy()
    assert R.well_conditioned(Vh)
    assert float(np.abs(s.astype(np.float64) - R.pairs(Vh, pairs[:, 0], pairs[:, 1])).max()) <= R.GATE
    # the file of baseline_attack_balanced: the device's scores, the host route's schema
    atk.baseline_attack_balanced()
    saved = torch.load(atk.result_filename(), weights_only=False)
    assert sorted(saved) == ["auc", "pr", "result"] and saved["result"]["y"] == list(y)
    assert np.array_equal(np.asarray(saved["result"]["pred"]), s.astype(np.float64))
    with pytest.raises(NotImplementedError):
        atk.recover_edges()


def test_cli_metrics_only_and_recover(gpu, tmp_path, monkeypatch, capsys):
    import re
    from curve_restate import ap_bound
    from test_cli_worker_dp import _write_musae
    from linkteller_amd import main as lt_main, synth
    from linkteller_amd.gcn import GCN
    a1, a2 = synth.powerlaw_graph(260, 1200, seed=1), synth.powerlaw_graph(320, 1500, seed=2)
    _write_musae(str(tmp_path), "ES", a1, 400, 1)
    _write_musae(str(tmp_path), "RU", a2, 400, 2)
    torch.manual_seed(0)
    torch.save(GCN(3170, 256, 2, 0.5).state_dict(), tmp_path / "model.pt")
    monkeypatch.chdir(tmp_path)
    base = (f"--mode vanilla-clean --dataset twitch/ES/RU --hidden 256 --norm FirstOrderGCN --test --model-path {tmp_path}/model.pt "
            f"--attack --attack-mode baseline-feat --sample-type unbalanced --n-test 60 --data-root {tmp_path} "
            f"--baseline-scores device").split()
    lt_main.main(base + ["--metrics-only"])
    out = capsys.readouterr().out
    assert "attack results saved" not in out and not os.path.exists("eval_twitch")
    got = [float(re.search(rf"^{k} = (\S+)$", out, flags=re.M).group(1)) for k in ("auc", "ap")]
    lt_main.main(base + ["--recover"])
    out = capsys.readouterr().out
    result_file = "eval_twitch/ES/RU/baseline-feat_unbalanced_60_42.pt"
    recover_file = "eval_twitch/ES/RU/recover_baseline-feat_unbalanced_60_42.pt"
    assert f"attack results saved to: {result_file}" in out and f"recovered edges saved to: {recover_file}" in out
    ref = [float(re.search(rf"^{k} = (\S+)$", out, flags=re.M).group(1)) for k in ("auc", "ap")]
    bound = ap_bound(60 * 59 // 2)
    assert abs(got[0] - ref[0]) <= bound and abs(got[1] - ref[1]) <= bound
    rec = torch.load(recover_file, weights_only=False)
    assert len(rec["beliefs"]) == 5 and out.count("belief = ") == 5
    # the recovered pairs are the top of the saved score list
    saved = torch.load(result_file, weights_only=False)
    pred = np.asarray(saved["result"]["pred"])
    m = int(np.asarray(rec["counts"]).max())
    assert np.array_equal(np.sort(rec["scores"])[::-1][:m], np.sort(pred.astype(np.float32).astype(np.float64))[::-1][:m])

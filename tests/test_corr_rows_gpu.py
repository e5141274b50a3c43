"""Row bands of the baseline attacks' correlation square (lt_corr_rows_prepare / lt_corr_rows, engine.CorrRows) against the
one-piece square (engine.corr_square) BIT FOR BIT, against the shared restatement (tests/corr_restate.py) through the square's
value gate, and the Attacker's chunked edge recovery for the baseline attacks against its one-shot route array for array.

Shapes (200 rows, ``RandomState(1000 + D)``, ``nodes = RandomState(11 k + D).permutation(200)[:k]``, as tests/test_corr_gpu.py):
64-row tile edges (k = 65, 130, 200 and bands that start off a multiple of 64), the 16-column staging step and its K tail
(D = 7, 259), several K slices ((130, 259): 9; (130, 3170): 16) whose partial tiles go through the workspace, and one slice
(D = 7: a single staging step; (2050, 40): 561 tiles, three steps, an 8-column K tail) where the finish is the kernel's epilogue."""
import argparse
import os
import types

import numpy as np
import pytest
import torch

import abi_views as av
import corr_restate as R

pytestmark = pytest.mark.gpu

N_ROWS = 200
SENTINEL = -7.0
CASES = [(k, D) for k in (2, 65, 130, 200) for D in (7, 64, 259)] + [(130, 3170)]
_CACHE = {}


def _case(k, D):
    """(V, nodes, restatement) of a case, built once and never written to."""
    hit = _CACHE.get((k, D))
    if hit is None:
        if D == 3170:
            V = R.indicator_rows(np.random.RandomState(31), 160, 3170, 0.05)
            nodes = np.random.RandomState(11 * k + D).permutation(160)[:k]
        elif k > N_ROWS:
            V = R.normal_rows(np.random.RandomState(1000 + D), k + 50, D)
            nodes = np.random.RandomState(11 * k + D).permutation(k + 50)[:k]
        else:
            V = R.normal_rows(np.random.RandomState(1000 + D), N_ROWS, D)
            nodes = np.random.RandomState(11 * k + D).permutation(N_ROWS)[:k]
        exp = R.square(V, nodes)
        for a in (V, nodes, exp):
            a.setflags(write=False)
        hit = _CACHE[(k, D)] = (V, nodes, exp)
    return hit


def _bits(t):
    return t.contiguous().view(torch.int32)


def _device(gpu, V, nodes):
    return torch.from_numpy(np.array(V)).to(gpu), torch.from_numpy(np.asarray(nodes, dtype=np.int32)).to(gpu)


def _banded(handle, square, chunk, trapezoid):
    """Every band of ``chunk`` rows: (cells that differ from the square's bits, cells right of n_cols that lost the sentinel,
    the assembled matrix).  One wait at the end."""
    k = handle.k
    diff = torch.zeros((), dtype=torch.int64, device=square.device)
    lost = torch.zeros((), dtype=torch.int64, device=square.device)
    full = torch.empty_like(square)
    for b in range(0, k, chunk):
        e = min(b + chunk, k)
        nc = max(e - 1, 1) if trapezoid else k
        handle.rows(b, e - b, 0).fill_(SENTINEL)                 # (n_cols = 0 forms nothing: the view of the reused buffer)
        got = handle.rows(b, e - b, nc)
        assert got.shape == (e - b, k) and got.dtype == torch.float32
        diff += (_bits(got[:, :nc]) != _bits(square[b:e, :nc])).sum()
        lost += (got[:, nc:] != SENTINEL).sum()
        full[b:e] = got
    return int(diff), int(lost), full


@pytest.mark.parametrize("k,D", CASES + [(2050, 40)])
def test_bands_equal_the_square_bit_for_bit(gpu, k, D):
    from linkteller_amd import engine
    V, nodes, exp = _case(k, D)
    assert R.well_conditioned(V, nodes) and not np.isnan(exp).any()
    vt, nt = _device(gpu, V, nodes)
    square, sinfo = engine.corr_square(vt, nt)
    chunks = sorted({1, 63, 64, 65, 100, k}) if k <= N_ROWS else [1000, k]
    handle = engine.CorrRows(vt, nt, max(chunks))
    assert torch.equal(handle.info.raw, sinfo.raw) and handle.info.check(nan_ok=False) == {"zero_norm": 0, "bad_ids": 0}
    for chunk in chunks:
        for trapezoid in (True, False):
            diff, lost, full = _banded(handle, square, min(chunk, k), trapezoid)      # (full: the last, untrimmed assembly)
            assert diff == 0 and lost == 0, (k, D, chunk, trapezoid, diff, lost)
    # two handles give equal bits; the value gate of the square holds for the bands' cells
    again = engine.CorrRows(vt, nt, k)
    got = again.rows(0, k)
    assert torch.equal(_bits(got), _bits(full)) and torch.equal(_bits(got), _bits(square)) and torch.equal(again.info.raw, sinfo.raw)
    h = got.cpu().numpy()
    err = float(np.abs(h.astype(np.float64) - exp).max())
    print(f"k={k} D={D}: worst |band cell - restatement| = {err:.3e} (gate {R.GATE:.3e})")
    assert not np.isnan(h).any() and err <= R.GATE
    if k > N_ROWS:                                   # a band that starts off a multiple of 64, in the one-slice plan
        diff = (_bits(again.rows(997, 130, 1100)[:, :1100]) != _bits(square[997:1127, :1100])).sum()
        assert int(diff) == 0


def _raw(gpu, vview, n, D, nodes, row_begin, n_rows, n_cols, oview, max_rows=None):
    from linkteller_amd import _lib, engine
    nt = torch.from_numpy(np.asarray(nodes, dtype=np.int32)).to(gpu)
    k = int(nt.numel())
    info = torch.full((4,), -1, dtype=torch.int64, device=gpu)
    ws = engine._workspace(_lib.lib().lt_corr_rows_workspace_bytes(n, D, k, n_rows if max_rows is None else max_rows), gpu)
    _lib.check(_lib.lib().lt_corr_rows_prepare(vview.assert_aligned(), vview.ld, n, D, nt.data_ptr(), k, info.data_ptr(), ws.data_ptr(),
                                               ws.numel(), engine._stream()), "lt_corr_rows_prepare")
    _lib.check(_lib.lib().lt_corr_rows(vview.assert_aligned(), vview.ld, n, D, nt.data_ptr(), k, row_begin, n_rows, n_cols,
                                       oview.assert_aligned(), oview.ld, ws.data_ptr(), ws.numel(), engine._stream()), "lt_corr_rows")
    torch.cuda.synchronize()
    return oview.body(), [int(x) for x in info.cpu().tolist()]


@pytest.mark.parametrize("k,D", [(65, 7), (130, 259)])
def test_strided_unaligned_operands(gpu, k, D):
    """ldv > D with NaN pad columns, base pointers 4 bytes off a 16-byte boundary, ldo > k with sentinel pads that must survive;
    the band starts at row 37 (no multiple of 64) and is asked for whole and as a trapezoid."""
    from linkteller_amd import engine
    V, nodes, exp = _case(k, D)
    square = engine.corr_square(*_device(gpu, V, nodes))[0].cpu().numpy()
    b, nr = 37, k - 37 - 3
    for off_v, off_o in ((1, 0), (0, 1), (1, 3)):
        for nc in (k, b + nr - 1, 64, 1):
            vv = av.View(np.array(V), ld=D + 4, off=off_v)                  # 11 and 263: odd leading dimensions
            assert vv.ld % 2 == 1
            ov = av.View.output(nr, k, ld=k + (4 if k % 2 else 3), off=off_o, fill=SENTINEL)      # 69 and 133: odd too
            assert ov.ld % 2 == 1
            assert vv.ptr % 16 == (4 * off_v) % 16
            got, info = _raw(gpu, vv, N_ROWS, D, nodes, b, nr, nc, ov)
            tag = (k, D, off_v, off_o, nc)
            assert info == [0, 0, 0, 0], tag
            assert np.array_equal(got[:, :nc].view(np.int32), square[b:b + nr, :nc].view(np.int32)), tag
            assert (got[:, nc:] == SENTINEL).all() and ov.pads_untouched() and vv.pads_untouched(), tag


# Pairs of fp32 rows (x, y), as int32 bits, for which the two division orders of a score round to DIFFERENT fp32 values:
# float32(g / |x| / |y|) != float32(g / |y| / |x|) with g = <x, y> and the norms in float64.  Found by a search on the CPU (about
# one triple in 10^9 has the property); the test re-derives the property before it relies on it.
DIVISION_ORDER_PAIRS = [
    ((-1087891240, 1062692421), (-1092465101, 1062566020)),
    ((-1096392604, 1076843678), (-1072423906, -1085184750)),
    ((-1101012875, 1049086459), (1043998594, 1066704993)),
]


@pytest.mark.parametrize("D", [2, 40])
def test_division_order_above_the_diagonal(gpu, D):
    """The square forms a cell in its lower position, g / n_row / n_col with row >= col, and mirrors the bits; a band must divide
    in that order above the diagonal too.  The list is (x, -x, y, -y): the column sums are exactly zero, so the centred rows are
    the rows, and g and the norms are sums of two exact products rounded once -- the same doubles on the host and on the device.
    D = 2: one staging step, the epilogue finish; D = 40 (38 zero columns): three slices, the finish kernel."""
    from linkteller_amd import engine
    assert DIVISION_ORDER_PAIRS
    for xb, yb in DIVISION_ORDER_PAIRS:
        x, y = (np.array(b, dtype=np.int32).view(np.float32).astype(np.float64) for b in (xb, yb))
        g, nx, ny = x[0] * y[0] + x[1] * y[1], np.sqrt(x[0] * x[0] + x[1] * x[1]), np.sqrt(y[0] * y[0] + y[1] * y[1])
        lower = np.array([g / ny / nx], dtype=np.float64).astype(np.float32)     # cell (2, 0): row y, column x
        other = np.array([g / nx / ny], dtype=np.float64).astype(np.float32)
        assert lower.view(np.int32)[0] != other.view(np.int32)[0]                # the premise
        V = np.zeros((4, D), dtype=np.float32)
        V[:, :2] = np.array([x, -x, y, -y], dtype=np.float32)
        vt, nt = _device(gpu, V, np.arange(4))
        square, sinfo = engine.corr_square(vt, nt)
        sq = square.cpu().numpy()
        assert sq[2, 0].view(np.int32) == lower.view(np.int32)[0] == sq[0, 2].view(np.int32)
        for chunk in (1, 2, 4):
            handle = engine.CorrRows(vt, nt, chunk)
            assert _banded(handle, square, chunk, False)[:2] == (0, 0), (xb, yb, D, chunk)


def test_repeated_ids(gpu):
    from linkteller_amd import engine
    V = _case(65, 64)[0]
    nodes = np.array([5, 9, 5, 120, 9, 9, 33, 2, 199, 0, 5, 77, 78, 79, 80, 81, 82] * 5, dtype=np.int64)
    vt, nt = _device(gpu, V, nodes)
    square, sinfo = engine.corr_square(vt, nt)
    handle = engine.CorrRows(vt, nt, 33)
    assert torch.equal(handle.info.raw, sinfo.raw)
    for trapezoid in (False, True):
        assert _banded(handle, square, 33, trapezoid)[:2] == (0, 0)
    got = handle.rows(0, 3).cpu().numpy()
    assert np.array_equal(got[0].view(np.int32), got[2].view(np.int32))


def test_bad_ids_and_zero_norm_rows(gpu):
    """Small-integer rows in +- pairs plus an all-zero row listed twice (its centred vector is exactly zero), and two ids outside
    [0, n).  An id is compared, never dereferenced: nothing is provoked.  NaN cells and info as in the square."""
    from linkteller_amd import engine
    rng = np.random.RandomState(8)
    half = np.round(rng.standard_normal((40, 11)) * 4).astype(np.float32)
    half[(half == 0).all(axis=1)] = 1.0
    V = np.concatenate([half, -half, np.zeros((1, 11), dtype=np.float32)])
    nodes = np.r_[np.arange(80), 80, 80][rng.permutation(82)].astype(np.int64)
    listed = np.r_[nodes[:30], 81, nodes[30:70], -1, nodes[70:]]
    vt, nt = _device(gpu, V, listed)
    square, sinfo = engine.corr_square(vt, nt)
    handle = engine.CorrRows(vt, nt, 50)
    assert [int(x) for x in handle.info.raw.cpu().tolist()] == [2, 2, 0, 0] and torch.equal(handle.info.raw, sinfo.raw)
    with pytest.raises(IndexError, match="2 node ids"):
        handle.info.check()
    for trapezoid in (False, True):
        assert _banded(handle, square, 50, trapezoid)[:2] == (0, 0)
    full = _banded(handle, square, 50, False)[2].cpu().numpy()
    nan_rows = np.flatnonzero((listed == 80) | (listed == 81) | (listed == -1))
    good = np.setdiff1d(np.arange(len(listed)), nan_rows)
    assert np.isnan(full[nan_rows]).all() and np.isnan(full[:, nan_rows]).all() and not np.isnan(full[np.ix_(good, good)]).any()
    # zero-norm rows alone: the ValueError of the one-shot route, from four words
    only_zero = engine.CorrRows(vt, torch.from_numpy(nodes.astype(np.int32)).to(gpu), 16)
    with pytest.raises(ValueError, match="zero-norm"):
        only_zero.info.check(nan_ok=False)
    assert only_zero.info.check() == {"zero_norm": 2, "bad_ids": 0}


def test_wrapper_checks(gpu):
    from linkteller_amd import _lib, engine
    vt = torch.zeros((8, 3), dtype=torch.float32, device=gpu)
    idx = torch.arange(4, dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.LinkTellerHipError):
        engine.CorrRows(vt.cpu(), idx, 2)
    with pytest.raises(TypeError):
        engine.CorrRows(vt.double(), idx, 2)
    with pytest.raises(TypeError):
        engine.CorrRows(vt, idx.long(), 2)
    with pytest.raises(ValueError):
        engine.CorrRows(vt.t(), idx, 2)                                       # last-dimension stride 1
    with pytest.raises(ValueError):
        engine.CorrRows(vt, idx, 0)
    with pytest.raises(ValueError):
        engine.CorrRows(vt, idx[:0], 2)
    W = np.random.RandomState(2).standard_normal((40, 6)).astype(np.float32)
    view = torch.from_numpy(W).to(gpu)[:, 1:4]                                # strided rows are allowed
    nodes = torch.arange(0, 40, 3, dtype=torch.int32, device=gpu)
    h = engine.CorrRows(view, nodes, 5)
    assert h.max_rows == 5 and h.device_bytes > 0
    for bad in ((-1, 2), (0, 6), (12, 3), (0, -1)):
        with pytest.raises(ValueError):
            h.rows(*bad)
    with pytest.raises(ValueError):
        h.rows(0, 2, 15)
    square = engine.corr_square(view, nodes)[0]
    assert torch.equal(_bits(h.rows(9, 5)), _bits(square[9:14]))
    assert h.rows(14, 0).shape == (0, 14)


# ---- end to end: the 300-node graph of tests/test_recover_graph_gpu.py -----------------------------------------------------------
@pytest.fixture(scope="module")
def er_world(gpu):
    from linkteller_amd import graph, synth
    adj = synth.erdos_renyi_graph(300, 1500, seed=3)
    x = torch.from_numpy(synth.gaussian_features(300, 32, seed=4)).to(gpu)
    adj_t = graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(adj)).to(gpu)
    return adj, types.SimpleNamespace(features_2=x, adj_2=adj_t, adj_ori=adj, n_nodes=300)


def _attacker(mode, route, w, gpu, n_test=300):
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN
    torch.manual_seed(11)
    model = GCN(32, 16, 2, 0.5).to(gpu).eval()
    args = argparse.Namespace(dataset="twitch/x", sample_type="unbalanced", n_test=n_test, sample_seed=42, influence=1e-4,
                              mode="vanilla-clean", attack_mode=mode, baseline_scores=route)
    return Attacker(args, model, w)


def _same(a, b, tag):
    assert set(a) == set(b), tag
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (tag, k)
        else:
            assert type(x) is type(y) and x == y, (tag, k, x, y)


def _whole_graph_sample(atk, adj):
    """The sample that names every node: what prepare_test_data would leave for test_nodes = arange(N)."""
    import scipy.sparse as sp
    up = sp.triu(sp.csr_matrix(adj), 1).tocoo()
    atk.test_nodes = list(range(adj.shape[0]))
    atk.exist_edges = [(int(a), int(b)) for a, b in zip(up.row, up.col)]
    atk.nonexist_edges = []
    return len(atk.exist_edges)


@pytest.mark.parametrize("mode", ["baseline-feat", "baseline"])
@pytest.mark.parametrize("route", ["device", "stream"])
def test_recover_edges_chunked_equals_one_shot(gpu, er_world, mode, route):
    adj, w = er_world
    atk = _attacker(mode, route, w, gpu)
    _whole_graph_sample(atk, adj)
    want = dict(atk.recover_edges())
    m = int(max(want["counts"]))
    assert len(want["pairs"]) == m > 0
    if mode == "baseline":
        # two classes: the posteriors centre to (t, -t), every score is +-1 -- the selection is decided among ties
        print(f"baseline: m = {m}, above = {want['above']}, tied_total = {want['tied_total']}")
        assert np.abs(np.abs(want["scores"]) - 1.0).max() <= 1e-6 and want["tied_total"] > m
    for chunk in (1, 37, 64, 300, 1000):
        for trapezoid in (True, False):
            atk.corr_trapezoid = trapezoid
            got = atk.recover_edges(chunk=chunk)
            _same(got, want, f"{mode} {route} chunk={chunk} trapezoid={trapezoid}")
            st = atk.recover_stream_stats
            assert st["pushes"] == -(-300 // min(chunk, 300)) and st["rows_device_bytes"] >= 4 * min(chunk, 300) * 300
    with pytest.raises(ValueError):
        atk.recover_edges(chunk=0)


@pytest.mark.parametrize("mode", ["baseline-feat", "baseline"])
def test_recover_graph_equals_recover_edges(gpu, er_world, mode):
    adj, w = er_world
    atk = _attacker(mode, "device", w, gpu)
    n_edges = _whole_graph_sample(atk, adj)
    want = dict(atk.recover_edges())
    fresh = _attacker(mode, "stream", w, gpu)                     # no prepare_test_data(), no pair lists
    got = fresh.recover_graph(chunk=64)
    assert got is fresh.recovered
    _same(got, want, f"{mode} whole graph")
    assert got["n_edges"] == n_edges and got["n_total"] == 300 * 299 // 2
    # a subset: the mean is taken over the listed nodes, as the sampled route takes it over test_nodes
    sub = _attacker(mode, "device", w, gpu, n_test=64)
    sub.prepare_test_data()
    want = dict(sub.recover_edges())
    fresh = _attacker(mode, "stream", w, gpu, n_test=64)
    _same(fresh.recover_graph(nodes=sub.test_nodes, chunk=17), want, f"{mode} subset")
    fresh.args.baseline_scores = "host"
    with pytest.raises(NotImplementedError, match="baseline_scores"):
        fresh.recover_graph(chunk=64)


def test_chunked_calls_refuse_a_zero_norm_row(gpu, er_world):
    """All rows equal: every centred row is zero.  Both chunked calls raise the one-shot route's ValueError before any push."""
    adj, w = er_world
    flat = types.SimpleNamespace(features_2=torch.full_like(w.features_2, 0.25), adj_2=w.adj_2, adj_ori=adj, n_nodes=300)
    atk = _attacker("baseline-feat", "stream", flat, gpu)
    _whole_graph_sample(atk, adj)
    with pytest.raises(ValueError, match="zero-norm"):
        atk.recover_edges()
    with pytest.raises(ValueError, match="zero-norm"):
        atk.recover_edges(chunk=64)
    with pytest.raises(ValueError, match="zero-norm"):
        atk.recover_graph(chunk=64)
    assert not hasattr(atk, "recover_stream_stats")


def test_cli_stream_recover_chunk_and_all_nodes(gpu, tmp_path, monkeypatch, capsys):
    import scipy.sparse as sp
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
            f"--attack --attack-mode baseline-feat --sample-type unbalanced --n-test 60 --data-root {tmp_path}").split()
    recover_file = "eval_twitch/ES/RU/recover_baseline-feat_unbalanced_60_42.pt"
    all_file = "eval_twitch/ES/RU/recover_all_baseline-feat_unbalanced_60_42.pt"

    lt_main.main(base + ["--baseline-scores", "device", "--recover"])
    capsys.readouterr()
    one_shot = torch.load(recover_file, weights_only=False)
    os.remove(recover_file)
    lt_main.main(base + ["--baseline-scores", "stream", "--recover", "--recover-chunk", "64"])
    out = capsys.readouterr().out
    assert f"recovered edges saved to: {recover_file}" in out and not os.path.exists(all_file)
    _same(torch.load(recover_file, weights_only=False), one_shot, "--baseline-scores stream --recover-chunk 64")
    os.remove(recover_file)

    lt_main.main(base + ["--baseline-scores", "stream", "--recover", "--recover-nodes", "all", "--recover-chunk", "64"])
    out = capsys.readouterr().out
    assert "the sampled AUC attack is skipped" in out and "attack results saved" not in out
    assert f"recovered edges saved to: {all_file}" in out and os.path.exists(all_file) and not os.path.exists(recover_file)
    rec = torch.load(all_file, weights_only=False)
    n = 320
    assert set(rec) == set(one_shot) and rec["n_total"] == n * (n - 1) // 2 and rec["n_edges"] == sp.triu(sp.csr_matrix(a2), 1).nnz
    assert len(rec["beliefs"]) == 5 and len(rec["pairs"]) == int(max(rec["counts"])) and out.count("belief = ") == 5
    is_edge = np.asarray(sp.csr_matrix(a2)[rec["pairs"][:, 0], rec["pairs"][:, 1]]).reshape(-1) != 0
    assert rec["is_edge"].dtype == bool and np.array_equal(rec["is_edge"], is_edge)

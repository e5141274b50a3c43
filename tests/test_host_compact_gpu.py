"""lt_influence_matrix_host: the synchronous host-landing entry.  On the fused `delta` route it can send the touched values
packed ("export_compact") while the host zero-fills the matrix; every form must give the matrix of rows + lt_export_rows_f64,
bit for bit."""
import numpy as np
import pytest
import torch

from linkteller_amd import _lib


def _params(w, dev):
    return [torch.from_numpy(w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")]


def _baseline(gpu, adj, f=96, h=64, seed=2):
    from linkteller_amd import engine, graph, synth
    hg = graph.HipGraph(graph.first_order_gcn(adj))
    n = adj.shape[0]
    x = torch.from_numpy(synth.twitch_like_features(n, f, seed=seed, density=0.05)).to(gpu)
    w = synth.gcn_weights(f, h, 2, seed=seed + 1)
    return engine.Baseline(hg, x, *_params(w, gpu))


def _raw(base, probes, obs, mode, dst, ldd, gpu):
    """lt_influence_matrix_host straight through the C ABI into a caller-given pinned buffer of leading dimension ldd."""
    from linkteller_amd import engine
    m = _lib.MODES[mode]
    npb, nob = probes.numel(), obs.numel()
    out = torch.empty((npb, nob), dtype=torch.float32, device=gpu)
    need = _lib.lib().lt_influence_workspace_bytes(base._h, npb, nob, m)
    ws = engine._workspace(need, gpu)
    return _lib.lib().lt_influence_matrix_host(base._h, probes.data_ptr(), npb, obs.data_ptr(), nob, 1e-4, m, out.data_ptr(), nob,
                                               dst.data_ptr(), ldd, ws.data_ptr(), ws.numel(), engine._stream())


def test_entry_checks_its_arguments_without_a_device():
    h = _lib.lib()
    assert h.lt_influence_matrix_host(None, None, 1, None, 1, 1e-4, 2, None, 1, None, 1, None, 0, None) == -1
    _lib.set_tuning("export_compact", 2)
    _lib.set_tuning("export_compact", None)
    assert h.lt_set_tuning(b"export_compact", 3) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("compact", [0, 1, 2])
def test_host_matrix_equals_the_dense_export(gpu, compact):
    from linkteller_amd import engine, synth
    n = 1200
    base = _baseline(gpu, synth.erdos_renyi_graph(n, 5000, seed=1))
    rng = np.random.RandomState(4)
    _lib.set_tuning("export_compact", compact)
    try:
        for nob in (1, 7, 64, 257, 1000):
            obs = torch.from_numpy(rng.choice(n, nob, replace=False).astype(np.int32)).to(gpu)
            probes = obs[: max(1, nob // 2)].contiguous()
            npb = probes.numel()
            base.refresh("delta")
            want = engine.export_rows_f64(base.influence_rows(probes, obs, 1e-4, "delta"))
            for refresh in (True, False):
                got = base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=refresh)
                assert got.dtype == np.float64 and np.array_equal(got, want), (nob, refresh)
            # a dirty pinned buffer with one padding column: the matrix is exact, the padding untouched
            for ldd in (nob, nob + 1):
                dst = torch.full((npb, ldd), 7.0, dtype=torch.float64).pin_memory()
                base.refresh("delta")
                _lib.check(_raw(base, probes, obs, "delta", dst, ldd, gpu), "lt_influence_matrix_host")
                d = dst.numpy()
                assert np.array_equal(d[:, :nob], want), (nob, ldd)
                assert np.all(d[:, nob:] == 7.0), (nob, ldd, "padding")
        # several probe chunks
        obs = torch.from_numpy(rng.choice(n, 301, replace=False).astype(np.int32)).to(gpu)
        probes = obs[:300].contiguous()
        base.refresh("delta")
        want = engine.export_rows_f64(base.influence_rows(probes, obs, 1e-4, "delta"))
        _lib.set_tuning("chunk_budget_bytes", 1 << 20)
        try:
            for refresh in (True, False):
                assert np.array_equal(base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=refresh), want)
        finally:
            _lib.set_tuning("chunk_budget_bytes", None)
    finally:
        _lib.set_tuning("export_compact", None)


@pytest.mark.gpu
def test_every_pair_touched_under_the_forced_packed_form(gpu):
    """A small dense graph: every probe's two-hop set holds every observed node, so the packed rows are full."""
    from linkteller_amd import engine, synth
    n = 64
    base = _baseline(gpu, synth.erdos_renyi_graph(n, 900, seed=5), f=48, h=32, seed=6)
    obs = torch.arange(n, dtype=torch.int32, device=gpu)
    base.refresh("delta")
    want = engine.export_rows_f64(base.influence_rows(obs, obs, 1e-4, "delta"))
    assert np.count_nonzero(want) > 0.9 * want.size
    _lib.set_tuning("export_compact", 2)
    try:
        for refresh in (True, False):
            assert np.array_equal(base.influence_matrix_host(obs, obs, 1e-4, "delta", refresh=refresh), want)
        dst = torch.full((n, n + 1), 7.0, dtype=torch.float64).pin_memory()
        _lib.check(_raw(base, obs, obs, "delta", dst, n + 1, gpu), "lt_influence_matrix_host")
        assert np.array_equal(dst.numpy()[:, :n], want) and np.all(dst.numpy()[:, n] == 7.0)
    finally:
        _lib.set_tuning("export_compact", None)


@pytest.mark.gpu
@pytest.mark.parametrize("graph_kind,mode", [("powerlaw", "delta"), ("er", "sparse"), ("er", "full"), ("powerlaw", "sparse")])
def test_routes_without_records_land_the_same_matrix(gpu, graph_kind, mode):
    """Calls off the fused route (hub rows: no records; `sparse`, `full`) take lt_influence_rows_f64 and the wait, whatever
    "export_compact" says."""
    from linkteller_amd import engine, synth
    n = 1200
    adj = synth.powerlaw_graph(n, 6000, seed=7) if graph_kind == "powerlaw" else synth.erdos_renyi_graph(n, 5000, seed=7)
    base = _baseline(gpu, adj, seed=8)
    rng = np.random.RandomState(9)
    obs = torch.from_numpy(rng.choice(n, 200, replace=False).astype(np.int32)).to(gpu)
    probes = obs[:120].contiguous()
    base.refresh(mode)
    want = engine.export_rows_f64(base.influence_rows(probes, obs, 1e-4, mode))
    for compact in (0, 2):
        _lib.set_tuning("export_compact", compact)
        try:
            assert np.array_equal(base.influence_matrix_host(probes, obs, 1e-4, mode, refresh=True), want), compact
            dst = torch.full((120, 201), 7.0, dtype=torch.float64).pin_memory()
            base.refresh(mode)
            _lib.check(_raw(base, probes, obs, mode, dst, 201, gpu), "lt_influence_matrix_host")
            assert np.array_equal(dst.numpy()[:, :200], want) and np.all(dst.numpy()[:, 200] == 7.0), compact
        finally:
            _lib.set_tuning("export_compact", None)


@pytest.mark.gpu
@pytest.mark.parametrize("compact", [0, 2])
def test_bad_node_id_still_raises(gpu, compact):
    from linkteller_amd import engine, synth
    n = 1200
    base = _baseline(gpu, synth.erdos_renyi_graph(n, 5000, seed=1))
    rng = np.random.RandomState(10)
    probes = rng.choice(n, 24, replace=False).astype(np.int32)
    obs = rng.choice(n, 40, replace=False).astype(np.int32)
    tp, to = torch.from_numpy(probes).to(gpu), torch.from_numpy(obs).to(gpu)
    _lib.set_tuning("export_compact", compact)
    try:
        good = base.influence_matrix_host(tp, to, 1e-4, "delta", refresh=True)
        for bad_list in ("probe", "observed"):
            p2, o2 = probes.copy(), obs.copy()
            (p2 if bad_list == "probe" else o2)[7] = n + 3
            with pytest.raises(IndexError):
                base.influence_matrix_host(torch.from_numpy(p2).to(gpu), torch.from_numpy(o2).to(gpu), 1e-4, "delta", refresh=True)
            engine.node_check()                            # cleared by the report
        assert np.array_equal(base.influence_matrix_host(tp, to, 1e-4, "delta", refresh=True), good)
    finally:
        _lib.set_tuning("export_compact", None)

"""lt_influence_matrix_host, packed form in two halves: the indices of the touched positions leave with the probes' record blocks
(the step's first launch), the fp32 values with the finish kernel, and a single-chunk call may consume the index run before the
stream wait ("export_early").  Every form must give the matrix of rows + lt_export_rows_f64, bit for bit; a stale index, ready
word or cursor of an earlier call must never reach the matrix; the publication of the index run must hold (export_early = 2)."""
import ctypes as C

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


def _raw(base, probes, obs, dst, ldd, gpu):
    from linkteller_amd import engine
    m = _lib.MODES["delta"]
    npb, nob = probes.numel(), obs.numel()
    out = torch.empty((npb, nob), dtype=torch.float32, device=gpu)
    need = _lib.lib().lt_influence_workspace_bytes(base._h, npb, nob, m)
    ws = engine._workspace(need, gpu)
    return _lib.lib().lt_influence_matrix_host(base._h, probes.data_ptr(), npb, obs.data_ptr(), nob, 1e-4, m, out.data_ptr(), nob,
                                               dst.data_ptr(), ldd, ws.data_ptr(), ws.numel(), engine._stream())


def _want(base, probes, obs):
    from linkteller_amd import engine
    base.refresh("delta")
    return engine.export_rows_f64(base.influence_rows(probes, obs, 1e-4, "delta"))


def _packed(base):
    s = base.host_landing_stats()
    return s["early"] + s["late"]


class _knobs:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            _lib.set_tuning(k, v)

    def __exit__(self, *a):
        for k in self.kv:
            _lib.set_tuning(k, None)


def test_new_entry_and_knob_check_their_arguments_without_a_device():
    h = _lib.lib()
    o = (C.c_int64 * 4)()
    assert h.lt_host_landing_stats(None, o) == -1
    assert h.lt_host_landing_stats(None, None) == -1
    for v in (0, 1, 2):
        _lib.set_tuning("export_early", v)
    _lib.set_tuning("export_early", None)
    assert h.lt_set_tuning(b"export_early", 3) == -1
    assert h.lt_set_tuning(b"export_early", -1) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("compact", [1, 2])
@pytest.mark.parametrize("early", [0, 1])
def test_host_matrix_equals_the_dense_export(gpu, early, compact):
    from linkteller_amd import synth
    n = 1200
    rng = np.random.RandomState(4)
    # (aggregate_first = 0: graphs of this size would form the pre-activation aggregate-first, which is not the fused route)
    with _knobs(export_early=early, export_compact=compact, aggregate_first=0):
        base = _baseline(gpu, synth.erdos_renyi_graph(n, 5000, seed=1))
        for nob in (1, 7, 64, 257, 1000):
            obs = torch.from_numpy(rng.choice(n, nob, replace=False).astype(np.int32)).to(gpu)
            probes = obs[: max(1, nob // 2)].contiguous()
            npb = probes.numel()
            want = _want(base, probes, obs)
            c0 = _packed(base)
            for refresh in (True, False):      # (the record blocks ride in different launches, or run as a launch of their own)
                got = base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=refresh)
                assert got.dtype == np.float64 and np.array_equal(got, want), (nob, refresh)
            if compact == 2:
                assert _packed(base) - c0 == 2, (nob, "the calls were not packed: the test would prove nothing")
            dst = torch.full((npb, nob + 1), 7.0, dtype=torch.float64).pin_memory()
            for refresh in (True, False):
                dst.fill_(7.0)
                if refresh:
                    base.refresh("delta")
                _lib.check(_raw(base, probes, obs, dst, nob + 1, gpu), "lt_influence_matrix_host")
                d = dst.numpy()
                assert np.array_equal(d[:, :nob], want), (nob, refresh, "ldd = n_obs + 1")
                assert np.all(d[:, nob:] == 7.0), (nob, refresh, "padding")
        # a repeated observed node
        obs_np = rng.choice(n, 65, replace=False).astype(np.int32)
        obs_np[64] = obs_np[3]
        obs = torch.from_numpy(obs_np).to(gpu)
        probes = obs[:40].contiguous()
        want = _want(base, probes, obs)
        assert np.array_equal(want[:, 64], want[:, 3])
        for refresh in (True, False):
            assert np.array_equal(base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=refresh), want), refresh
        # a chunked call
        obs = torch.from_numpy(rng.choice(n, 301, replace=False).astype(np.int32)).to(gpu)
        probes = obs[:300].contiguous()
        want = _want(base, probes, obs)
        for budget in (1 << 20, 1 << 14):      # (16 KiB: ~ 50 probes of this graph to a chunk, so the call IS chunked)
            with _knobs(chunk_budget_bytes=budget):
                s0 = base.host_landing_stats()
                for refresh in (True, False):
                    assert np.array_equal(base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=refresh), want), (budget, refresh)
                s1 = base.host_landing_stats()
                if compact == 2:      # (1 packs by the graph's touched share: this one's is above the bar)
                    assert (s1["early"] - s0["early"]) + (s1["late"] - s0["late"]) == 2, budget
                if budget == 1 << 14:
                    assert s1["early"] == s0["early"], "a chunked call took the early path"


@pytest.mark.gpu
@pytest.mark.parametrize("early", [0, 1])
def test_every_pair_touched(gpu, early):
    from linkteller_amd import synth
    n = 64
    obs = torch.arange(n, dtype=torch.int32, device=gpu)
    with _knobs(export_early=early, export_compact=2, aggregate_first=0):
        base = _baseline(gpu, synth.erdos_renyi_graph(n, 900, seed=5), f=48, h=32, seed=6)
        want = _want(base, obs, obs)
        assert np.count_nonzero(want) > 0.9 * want.size
        for refresh in (True, False):
            assert np.array_equal(base.influence_matrix_host(obs, obs, 1e-4, "delta", refresh=refresh), want)
        assert _packed(base) == 2
        dst = torch.full((n, n + 1), 7.0, dtype=torch.float64).pin_memory()
        _lib.check(_raw(base, obs, obs, dst, n + 1, gpu), "lt_influence_matrix_host")
        assert np.array_equal(dst.numpy()[:, :n], want) and np.all(dst.numpy()[:, n] == 7.0)


@pytest.mark.gpu
@pytest.mark.parametrize("compact", [1, 2])
@pytest.mark.parametrize("early", [0, 1])
def test_bad_node_id_still_raises(gpu, early, compact):
    from linkteller_amd import engine, synth
    n = 1200
    rng = np.random.RandomState(10)
    probes = rng.choice(n, 24, replace=False).astype(np.int32)
    obs = rng.choice(n, 40, replace=False).astype(np.int32)
    tp, to = torch.from_numpy(probes).to(gpu), torch.from_numpy(obs).to(gpu)
    with _knobs(export_early=early, export_compact=compact, aggregate_first=0):
        base = _baseline(gpu, synth.erdos_renyi_graph(n, 5000, seed=1))
        good = base.influence_matrix_host(tp, to, 1e-4, "delta", refresh=True)
        assert compact != 2 or _packed(base) == 1
        for bad_list in ("probe", "observed"):
            p2, o2 = probes.copy(), obs.copy()
            (p2 if bad_list == "probe" else o2)[7] = n + 3
            with pytest.raises(IndexError):
                base.influence_matrix_host(torch.from_numpy(p2).to(gpu), torch.from_numpy(o2).to(gpu), 1e-4, "delta", refresh=True)
            engine.node_check()                            # cleared by the report
        assert np.array_equal(base.influence_matrix_host(tp, to, 1e-4, "delta", refresh=True), good)


@pytest.mark.gpu
@pytest.mark.parametrize("early", [0, 1])
def test_stale_state_never_reaches_the_matrix(gpu, early):
    """Large, small, large again on one baseline (the small call leaves most of the large call's indices and values in the staging
    block, and a ready word of its own), and two baselines used alternately."""
    from linkteller_amd import synth
    n = 1200
    rng = np.random.RandomState(21)
    big = torch.from_numpy(rng.choice(n, 400, replace=False).astype(np.int32)).to(gpu)
    small = torch.from_numpy(rng.choice(n, 9, replace=False).astype(np.int32)).to(gpu)
    other = torch.from_numpy(rng.choice(n, 400, replace=False).astype(np.int32)).to(gpu)
    _lib.set_tuning("aggregate_first", 0)
    try:
        _stale_state(gpu, early, n, big, small, other)
    finally:
        _lib.set_tuning("aggregate_first", None)


def _stale_state(gpu, early, n, big, small, other):
    from linkteller_amd import synth
    a = _baseline(gpu, synth.erdos_renyi_graph(n, 5000, seed=1))
    b = _baseline(gpu, synth.erdos_renyi_graph(n, 4000, seed=11), seed=12)
    want = {("a", "big"): _want(a, big, big), ("a", "small"): _want(a, small, small), ("a", "other"): _want(a, other, other),
            ("b", "big"): _want(b, big, big), ("b", "small"): _want(b, small, small)}
    lists = {"big": big, "small": small, "other": other}
    with _knobs(export_early=early, export_compact=2):
        for refresh in (True, False):
            for which, name in (("a", "big"), ("a", "small"), ("a", "big"), ("a", "other"), ("a", "small"), ("a", "big")):
                got = a.influence_matrix_host(lists[name], lists[name], 1e-4, "delta", refresh=refresh)
                assert np.array_equal(got, want[(which, name)]), (which, name, refresh)
            for rep in range(3):
                for which, base, name in (("a", a, "big"), ("b", b, "big"), ("a", a, "small"), ("b", b, "small"), ("b", b, "big")):
                    got = base.influence_matrix_host(lists[name], lists[name], 1e-4, "delta", refresh=refresh)
                    assert np.array_equal(got, want[(which, name)]), (which, name, refresh, rep)
        assert _packed(a) == 2 * (6 + 3 * 2) and _packed(b) == 2 * 3 * 3


def _headline(gpu):
    from linkteller_amd import engine, graph, synth
    adj, x_np, w = synth.twitch_like_problem("twitch-RU", hidden=256, n_classes=2, seed=0)
    base = engine.Baseline(graph.HipGraph(graph.first_order_gcn(adj)), torch.from_numpy(x_np).to(gpu), *_params(w, gpu))
    base.enable_fp64()
    np.random.seed(42)
    nodes = torch.from_numpy(np.random.choice(np.arange(adj.shape[0]), 500, replace=False).astype(np.int32)).to(gpu)
    return base, nodes


@pytest.mark.gpu
def test_the_publication_holds_over_2000_headline_calls(gpu):
    """export_early = 2: the host keeps the indices it consumed before the stream wait and compares them with the finished run.
    Not one word may differ over 2 000 consecutive headline-shape calls, and the early path must have been taken (else the
    comparison proves nothing)."""
    base, nodes = _headline(gpu)
    want = _want(base, nodes, nodes)
    with _knobs(export_early=2):
        s0 = base.host_landing_stats()
        for i in range(2000):
            got = base.influence_matrix_host(nodes, nodes, 1e-4, "delta", refresh=True)
            if i % 100 == 0:
                assert np.array_equal(got, want), i
        s1 = base.host_landing_stats()
    early, late = s1["early"] - s0["early"], s1["late"] - s0["late"]
    print(f"early {early}, late {late}, mismatch {s1['mismatch'] - s0['mismatch']}, "
          f"post-wait {(s1['post_ns'] - s0['post_ns']) / 2000:.0f} ns per call")
    assert early + late == 2000
    assert s1["mismatch"] - s0["mismatch"] == 0
    assert early > 0, ("the early path was never taken on this machine in 2 000 headline calls: the ready word never arrived "
                       "before the stream was done, so this test proved nothing about the publication")


@pytest.mark.gpu
def test_counters_name_the_path_taken(gpu):
    """Single-chunk packed calls behind a refresh take the early path, chunked calls and export_early = 0 the late one, calls
    that are not packed neither."""
    base, nodes = _headline(gpu)
    want = _want(base, nodes, nodes)

    def run(k, **kv):
        with _knobs(**kv):
            s0 = base.host_landing_stats()
            for _ in range(k):
                assert np.array_equal(base.influence_matrix_host(nodes, nodes, 1e-4, "delta", refresh=True), want)
            s1 = base.host_landing_stats()
        return {k_: s1[k_] - s0[k_] for k_ in s0}

    d = run(50, export_early=1)
    assert d["early"] + d["late"] == 50 and d["early"] > 0 and d["post_ns"] > 0, d
    d = run(20, export_early=0)
    assert d["early"] == 0 and d["late"] == 20, d
    d = run(20, export_early=1, chunk_budget_bytes=1 << 16)      # (a few dozen probes to a chunk at this shape)
    assert d["early"] == 0 and d["late"] == 20, d
    d = run(5, export_compact=0)
    assert d["early"] == 0 and d["late"] == 0 and d["post_ns"] == 0, d

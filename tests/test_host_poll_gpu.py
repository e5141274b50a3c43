"""The packed host landing with "host_poll" (lt_influence.hip influence_host_impl, lt_host_landing.h): the host places every value as
its word in the staging block stops reading as the sentinel and returns without the stream wait.  The matrix must equal the late
form's ("host_poll" = 0) bit for bit on every shape of run; the value region must be armed again after every kind of call, so that
nothing of an earlier call is ever taken for a value; the sentinel may be a value the matrix holds; the counters name the path."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from linkteller_amd import _lib

pytestmark = pytest.mark.gpu
N, NA, F = 64, 48, 48          # nodes; nodes [0, NA) and [NA, N) are two components; features
CLIQUE = (3, 9, 14, 20, 27, 31)
FORCE = dict(export_compact=2, aggregate_first=0)      # (pack whatever the touched share; small graphs would aggregate first)


class _knobs:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            _lib.set_tuning(k, v)

    def __exit__(self, *a):
        for k in self.kv:
            _lib.set_tuning(k, None)


def _adjacency():
    """Two components, a 6-clique in the first: a pair of clique nodes is a position of more than 4 entries."""
    from linkteller_amd import synth
    a = synth.erdos_renyi_graph(NA, 110, seed=31).tolil()
    for u in CLIQUE:
        for v in CLIQUE:
            if u != v:
                a[u, v] = 1.0
    b = synth.erdos_renyi_graph(N - NA, 30, seed=32)
    return sp.block_diag([a.tocsr(), b]).tocsr()


def _baseline(gpu, h=64):
    from linkteller_amd import engine, graph, synth
    hg = graph.HipGraph(graph.first_order_gcn(_adjacency()))
    x = torch.from_numpy(synth.twitch_like_features(N, F, seed=33, density=0.08)).to(gpu)
    w = synth.gcn_weights(F, h, 2, seed=34)
    return engine.Baseline(hg, x, *[torch.from_numpy(w[k]).to(gpu) for k in ("W1", "b1", "W2", "b2")])


def _t(gpu, nodes):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(nodes, dtype=np.int32))).to(gpu)


def _lists():
    rng = np.random.RandomState(35)
    first = rng.permutation(NA).astype(np.int32)
    second = (NA + rng.permutation(N - NA)).astype(np.int32)
    rep = first[:30].copy()
    rep[29] = rep[4]
    rep[17] = rep[4]
    return {
        # probes, observed
        "plain": (first[:20], first[5:40]),
        "one probe without a touched position": (np.concatenate([first[:10], second[:1], first[10:14]]), first[:33]),
        "no entry at all": (second[:7], first[:19]),
        "one probe": (first[7:8], first[:41]),
        "repeated observed nodes": (first[:12], rep),
        "clique": (np.array(CLIQUE + (40, 41), dtype=np.int32), np.array((1, 2) + CLIQUE + (44,), dtype=np.int32)),
        "everything": (np.arange(N, dtype=np.int32), np.arange(N, dtype=np.int32)),
    }


def _delta(s1, s0):
    return {k: s1[k] - s0[k] for k in s0}


@pytest.mark.parametrize("h", [64, 132, 256])
def test_polled_matrix_equals_the_late_form(gpu, h):
    with _knobs(**FORCE):
        late, polled = _baseline(gpu, h), _baseline(gpu, h)
        for name, (p, o) in _lists().items():
            tp, to = _t(gpu, p), _t(gpu, o)
            for refresh in (True, False):
                with _knobs(host_poll=0):
                    s0 = late.host_landing_stats()
                    want = late.influence_matrix_host(tp, to, 1e-4, "delta", refresh=refresh).copy()
                    d = _delta(late.host_landing_stats(), s0)
                    assert d["early"] + d["late"] == 1 and d["polled"] == 0, (name, d)
                s0 = polled.host_landing_stats()
                got = polled.influence_matrix_host(tp, to, 1e-4, "delta", refresh=refresh)
                d = _delta(polled.host_landing_stats(), s0)
                assert d["polled"] == 1 and d["fallback"] == 0, (name, refresh, d, "the call was not polled: the case would prove nothing")
                assert np.array_equal(got, want), (name, refresh, h)
            if name == "one probe without a touched position":
                assert not want[10].any() and want[:10].any(axis=1).all()
            if name == "no entry at all":
                assert not want.any()
            if name == "repeated observed nodes":
                assert np.array_equal(want[:, 29], want[:, 4]) and np.array_equal(want[:, 17], want[:, 4]) and want[:, 4].any()
            if name == "clique":
                assert np.all(want[:6, 2:8] > 0)
        # ldd > n_obs: the padding columns are left as they were
        from linkteller_amd import engine
        p, o = _lists()["plain"]
        tp, to = _t(gpu, p), _t(gpu, o)
        npb, nob = len(p), len(o)
        with _knobs(host_poll=0):
            want = late.influence_matrix_host(tp, to, 1e-4, "delta", refresh=True).copy()
        dst = torch.full((npb, nob + 3), 7.0, dtype=torch.float64).pin_memory()
        out = torch.empty((npb, nob), dtype=torch.float32, device=gpu)
        m = _lib.MODES["delta"]
        ws = engine._workspace(_lib.lib().lt_influence_workspace_bytes(polled._h, npb, nob, m), gpu)
        s0 = polled.host_landing_stats()
        _lib.check(_lib.lib().lt_influence_matrix_host(polled._h, tp.data_ptr(), npb, to.data_ptr(), nob, 1e-4, m, out.data_ptr(), nob,
                                                       dst.data_ptr(), nob + 3, ws.data_ptr(), ws.numel(), engine._stream()),
                   "lt_influence_matrix_host")
        assert _delta(polled.host_landing_stats(), s0)["polled"] == 1
        assert np.array_equal(dst.numpy()[:, :nob], want) and np.all(dst.numpy()[:, nob:] == 7.0)
        assert np.array_equal(out.cpu().numpy().astype(np.float64), want)


@pytest.fixture(scope="module")
def fresh(gpu):
    """The matrix of every list on a baseline of its own (nothing of an earlier call in its staging block), computed once."""
    with _knobs(**FORCE):
        return {name: _baseline(gpu).influence_matrix_host(_t(gpu, p), _t(gpu, o), 1e-4, "delta", refresh=True).copy()
                for name, (p, o) in _lists().items()}


def _call(base, gpu, name, refresh=True):
    p, o = _lists()[name]
    return base.influence_matrix_host(_t(gpu, p), _t(gpu, o), 1e-4, "delta", refresh=refresh)


def test_the_value_region_is_armed_again_after_every_kind_of_call(gpu, fresh):
    from linkteller_amd import engine
    with _knobs(**FORCE):
        # a large call, a small one, a large one
        base = _baseline(gpu)
        for name in ("everything", "one probe", "everything", "plain", "no entry at all", "clique", "everything"):
            for refresh in (True, False):
                assert np.array_equal(_call(base, gpu, name, refresh), fresh[name]), (name, refresh)
        s = base.host_landing_stats()
        assert s["polled"] == 14 and s["fallback"] == 0, s
        # the staging block regrows: small first
        base = _baseline(gpu)
        for name in ("one probe", "plain", "everything", "one probe", "plain"):
            assert np.array_equal(_call(base, gpu, name), fresh[name]), name
        s = base.host_landing_stats()
        assert s["polled"] == 5 and s["fallback"] == 0, s
        # a refused call (LT_ERR_WORKSPACE) in between
        base = _baseline(gpu)
        assert np.array_equal(_call(base, gpu, "everything"), fresh["everything"])
        p, o = _lists()["plain"]
        tp, to = _t(gpu, p), _t(gpu, o)
        dst = torch.full((len(p), len(o)), 7.0, dtype=torch.float64).pin_memory()
        out = torch.empty((len(p), len(o)), dtype=torch.float32, device=gpu)
        ws = engine._workspace(256, gpu)
        rc = _lib.lib().lt_influence_step_host(base._h, tp.data_ptr(), len(p), to.data_ptr(), len(o), 1e-4, _lib.MODES["delta"],
                                               out.data_ptr(), len(o), dst.data_ptr(), len(o), ws.data_ptr(), 256, engine._stream(),
                                               _lib.STEP_REFRESH | _lib.STEP_DST_PINNED, None, None)
        assert rc == _lib.LT_ERR_WORKSPACE and np.all(dst.numpy() == 7.0)
        for name in ("plain", "everything", "clique"):
            assert np.array_equal(_call(base, gpu, name), fresh[name]), name
        # a multi-chunk call in between (the late form: its values are consumed behind the wait)
        base = _baseline(gpu)
        assert np.array_equal(_call(base, gpu, "everything"), fresh["everything"])
        with _knobs(chunk_budget_bytes=1 << 12):
            s0 = base.host_landing_stats()
            assert np.array_equal(_call(base, gpu, "everything"), fresh["everything"])
            d = _delta(base.host_landing_stats(), s0)
            assert d["early"] + d["late"] == 1 and d["polled"] == 0, (d, "the call was not chunked: the case would prove nothing")
        for name in ("plain", "everything", "one probe"):
            s0 = base.host_landing_stats()
            assert np.array_equal(_call(base, gpu, name), fresh[name]), name
            d = _delta(base.host_landing_stats(), s0)
            assert d["polled"] == 1 and d["fallback"] == 0, (name, d)


def test_the_sentinel_may_be_a_value_of_the_matrix(gpu, fresh):
    want = fresh["plain"]
    values = np.unique(want[want != 0])
    pattern = int(np.float32(values[len(values) // 2]).view(np.uint32))
    hits = int(np.count_nonzero(want.astype(np.float32).view(np.uint32) == pattern))
    assert hits >= 1
    with _knobs(**FORCE):
        base = _baseline(gpu)
        assert np.array_equal(_call(base, gpu, "plain"), want)
        with _knobs(host_poll_sentinel=pattern):
            for refresh in (True, False):
                s0 = base.host_landing_stats()
                got = _call(base, gpu, "plain", refresh)
                d = _delta(base.host_landing_stats(), s0)
                assert np.array_equal(got, want), refresh
                assert d["polled"] == 1 and d["fallback"] == 1, d
        s0 = base.host_landing_stats()
        assert np.array_equal(_call(base, gpu, "plain"), want)
        assert np.array_equal(_call(base, gpu, "everything"), fresh["everything"])
        d = _delta(base.host_landing_stats(), s0)
        assert d["polled"] == 2 and d["fallback"] == 0, d


def test_counters_name_the_route(gpu, fresh):
    with _knobs(**FORCE):
        base = _baseline(gpu)

        def run(k, **kv):
            with _knobs(**kv):
                s0 = base.host_landing_stats()
                for _ in range(k):
                    assert np.array_equal(_call(base, gpu, "everything"), fresh["everything"])
                return _delta(base.host_landing_stats(), s0)

        d = run(4)
        assert d["polled"] == 4 and d["fallback"] == 0 and d["early"] + d["late"] == 4, d
        d = run(3, host_poll=0)
        assert d["polled"] == 0 and d["late"] == 3 and d["looks"] == 0, d
        d = run(3, chunk_budget_bytes=1 << 12)
        assert d["polled"] == 0 and d["late"] == 3, d
        d = run(3, export_early=1)
        assert d["polled"] == 3 and d["early"] == 3 and d["late"] == 0, d
        d = run(3, export_early=2)
        assert d["polled"] == 3 and d["early"] == 3 and d["mismatch"] == 0, d
    with _knobs(aggregate_first=0, export_compact=0):
        s0 = base.host_landing_stats()
        assert np.array_equal(_call(base, gpu, "everything"), fresh["everything"])
        d = _delta(base.host_landing_stats(), s0)
        assert d["polled"] == 0 and d["early"] + d["late"] == 0, d


def test_new_entry_and_knobs_check_their_arguments(gpu):
    h = _lib.lib()
    o = (C.c_int64 * 4)()
    assert h.lt_host_landing_stats2(None, o) == -1
    assert h.lt_host_landing_stats2(None, None) == -1
    assert h.lt_set_tuning(b"host_poll", 2) == -1 and h.lt_set_tuning(b"host_poll", -1) == -1
    assert h.lt_set_tuning(b"host_poll_sentinel", 1 << 32) == -1 and h.lt_set_tuning(b"host_poll_sentinel", -1) == -1
    for k, v in (("host_poll", 0), ("host_poll", 1), ("host_poll_sentinel", 0), ("host_poll_sentinel", 0xFFFFFFFF)):
        _lib.set_tuning(k, v)
        _lib.set_tuning(k, None)


def test_the_late_form_keeps_its_early_look(gpu, fresh):
    """"host_poll" = 0 with "export_early" = 1 / 2: the look bounded by hipStreamQuery, the walk ahead over the index run, and
    (2) the comparison of the indices it consumed with the finished run -- on the small lists, and over 300 calls at the headline
    shape, where the look must have been in time at least once (else the comparison proves nothing)."""
    from linkteller_amd import engine, graph, synth
    with _knobs(host_poll=0, **FORCE):
        base = _baseline(gpu)
        for early in (1, 2):
            with _knobs(export_early=early):
                for name in ("everything", "one probe", "no entry at all", "clique", "everything"):
                    s0 = base.host_landing_stats()
                    assert np.array_equal(_call(base, gpu, name), fresh[name]), (early, name)
                    d = _delta(base.host_landing_stats(), s0)
                    assert d["polled"] == 0 and d["looks"] == 0 and d["early"] + d["late"] == 1 and d["mismatch"] == 0, (early, name, d)
    adj, x_np, w = synth.twitch_like_problem("twitch-RU", hidden=256, n_classes=2, seed=0)
    base = engine.Baseline(graph.HipGraph(graph.first_order_gcn(adj)), torch.from_numpy(x_np).to(gpu),
                           *[torch.from_numpy(w[k]).to(gpu) for k in ("W1", "b1", "W2", "b2")])
    nodes = _t(gpu, np.random.RandomState(42).choice(adj.shape[0], 500, replace=False))
    want = base.influence_matrix_host(nodes, nodes, 1e-4, "delta", refresh=True).copy()      # (polled: the default)
    assert base.host_landing_stats()["polled"] == 1
    with _knobs(host_poll=0, export_early=2):
        s0 = base.host_landing_stats()
        for i in range(300):
            got = base.influence_matrix_host(nodes, nodes, 1e-4, "delta", refresh=True)
            if i % 50 == 0:
                assert np.array_equal(got, want), i
        d = _delta(base.host_landing_stats(), s0)
    assert d["polled"] == 0 and d["early"] + d["late"] == 300 and d["mismatch"] == 0 and d["early"] > 0, d

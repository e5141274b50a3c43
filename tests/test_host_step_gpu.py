"""lt_influence_step_host / Baseline.influence_matrix_host: refresh, rows, wait and node check in ONE library call.  Every case
compares it with the separate calls -- refresh(mode), lt_influence_matrix_host, lt_node_check -- on a SECOND baseline over the same
tensors: the host matrices with np.array_equal, `out` with torch.equal.  dst is resolved lazily (only where the GPU writes it), so
every route is taken once."""
import ctypes as C

import numpy as np
import pytest
import torch

from linkteller_amd import _lib

import boundary_cases as B

pytestmark = pytest.mark.gpu
N, F, NP, NO = 600, 64, 37, 41
REFRESH, PINNED = _lib.STEP_REFRESH, _lib.STEP_DST_PINNED


class _knobs:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            _lib.set_tuning(k, v)

    def __exit__(self, *a):
        for k in self.kv:
            _lib.set_tuning(k, None)


def _pair(gpu, h=64, kind="er"):
    """(the baseline under test, the baseline of the separate calls) over the SAME graph, feature and weight tensors."""
    from linkteller_amd import engine, graph, synth
    if kind == "hub":
        hg = graph.HipGraph(B.graph_of("hub").a)
        x = torch.from_numpy(B.features("hub")).to(gpu)
        w = B.weights(24, 2)
    else:
        hg = graph.HipGraph(graph.first_order_gcn(synth.erdos_renyi_graph(N, 2400, seed=3)))
        x = torch.from_numpy(synth.twitch_like_features(N, F, seed=4, density=0.05)).to(gpu)
        w = synth.gcn_weights(F, h, 2, seed=5)
    p = [torch.from_numpy(w[k]).to(gpu) for k in ("W1", "b1", "W2", "b2")]
    return engine.Baseline(hg, x, *p), engine.Baseline(hg, x, *p)


def _two_chunk_budget(npb=NP, c=2):
    """The "chunk_budget_bytes" under which a `delta` call of npb probes on the default graph runs as exactly two probe chunks: the
    per-probe scratch of the mode (its longest column's entries, C floats and one int2 each, and a counter) times half the probes."""
    import scipy.sparse as sp
    from linkteller_amd import graph, synth
    a = sp.csc_matrix(graph.first_order_gcn(synth.erdos_renyi_graph(N, 2400, seed=3)))
    maxc = int(np.diff(a.indptr).max())
    return (maxc * c * 4 + 4 + maxc * 8) * ((npb + 1) // 2)


def _lists(gpu, kind="er", npb=NP, nob=NO):
    if kind == "hub":
        probes, obs = B.node_lists("hub")
    else:
        rng = np.random.RandomState(6)
        obs = rng.choice(N, max(nob, npb), replace=False).astype(np.int32)
        probes, obs = obs[::-1][:npb].copy(), obs[:nob]
    return torch.from_numpy(np.ascontiguousarray(probes)).to(gpu), torch.from_numpy(np.ascontiguousarray(obs)).to(gpu)


def _ws(base, probes, obs, mode, gpu):
    from linkteller_amd import engine
    need = _lib.lib().lt_influence_workspace_bytes(base._h, probes.numel(), obs.numel(), _lib.MODES[mode])
    return engine._workspace(need, gpu)


def _calls(ref, probes, obs, mode, refresh, gpu, fill=7.0, pad=1):
    """The separate calls through the C ABI into a dirty pinned buffer with `pad` padding columns: (rc of lt_node_check, dst, out)."""
    from linkteller_amd import engine
    npb, nob = probes.numel(), obs.numel()
    if mode == "delta":
        ref.enable_fp64()
    if refresh:
        ref.refresh(mode)
    dst = torch.full((npb, nob + pad), fill, dtype=torch.float64).pin_memory()
    out = torch.zeros((npb, nob), dtype=torch.float32, device=gpu)
    ws = _ws(ref, probes, obs, mode, gpu)
    _lib.check(_lib.lib().lt_influence_matrix_host(ref._h, probes.data_ptr(), npb, obs.data_ptr(), nob, 1e-4, _lib.MODES[mode],
                                                   out.data_ptr(), nob, dst.data_ptr(), nob + pad, ws.data_ptr(), ws.numel(),
                                                   engine._stream()), "lt_influence_matrix_host")
    return _lib.lib().lt_node_check(None, None), dst.numpy(), out


def _step(base, probes, obs, mode, flags, gpu, fill=7.0, pad=1, out="own", ws=None):
    """lt_influence_step_host through the C ABI, the same way: (rc, bad_probe, bad_observe, dst, out)."""
    from linkteller_amd import engine
    npb, nob = probes.numel(), obs.numel()
    if mode == "delta":
        base.enable_fp64()
    dst = torch.full((npb, nob + pad), fill, dtype=torch.float64).pin_memory()
    if out == "own":
        out = torch.zeros((npb, nob), dtype=torch.float32, device=gpu)
    ws = _ws(base, probes, obs, mode, gpu) if ws is None else ws
    bp, bo = C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib().lt_influence_step_host(base._h, probes.data_ptr(), npb, obs.data_ptr(), nob, 1e-4, _lib.MODES[mode],
                                           None if out is None else out.data_ptr(), nob, dst.data_ptr(), nob + pad, ws.data_ptr(),
                                           ws.numel(), engine._stream(), flags, C.byref(bp), C.byref(bo))
    return rc, bp.value, bo.value, dst.numpy(), out


def _packed(base):
    s = base.host_landing_stats()
    return s["early"] + s["late"]


def _scratch(base):
    return next(iter(base._host_scratch.values()))


ROUTES = {
    # name: (mode, graph, H, knobs, packed calls expected per call)
    "packed-h64": ("delta", "er", 64, dict(aggregate_first=0, export_compact=2), 1),
    "packed-h132": ("delta", "er", 132, dict(aggregate_first=0, export_compact=2), 1),
    "rows-h64": ("delta", "er", 64, dict(aggregate_first=0, export_compact=0), 0),
    "rows-h132": ("delta", "er", 132, dict(aggregate_first=0, export_compact=0), 0),
    "sparse": ("sparse", "er", 64, dict(), 0),
    "full": ("full", "er", 64, dict(), 0),
    "hub-items": ("delta", "hub", 24, dict(export_compact=2), 0),
    "two-chunks": ("delta", "er", 64, dict(aggregate_first=0, export_compact=2), 1),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_one_call_equals_the_separate_calls_on_every_route(gpu, route):
    mode, kind, h, kn, packed = ROUTES[route]
    with _knobs(**kn):
        base, ref = _pair(gpu, h, kind)
        probes, obs = _lists(gpu, kind)
        npb, nob = probes.numel(), obs.numel()
        whole = _ws(base, probes, obs, mode, gpu).numel()      # the workspace of the call as ONE probe chunk
    if route == "two-chunks":
        # (_knobs restores DEFAULTS on exit: the budget is the last knob set and nothing nested below touches it)
        kn = dict(kn, chunk_budget_bytes=_two_chunk_budget())
        with _knobs(chunk_budget_bytes=_two_chunk_budget() * 2 // 3):
            thirds = _ws(base, probes, obs, mode, gpu).numel()
    with _knobs(**kn):

        def chunked():
            """The budget is in force: the workspace is carved for a chunk of half the probes -- smaller than for one chunk, larger
            than for chunks of a third."""
            return route != "two-chunks" or thirds < _ws(base, probes, obs, mode, gpu).numel() < whole

        assert chunked()
        for refresh in (True, False):
            rc, want, want_out = _calls(ref, probes, obs, mode, refresh, gpu)
            assert rc == 0
            assert np.count_nonzero(want[:, :nob]) > 0 and chunked()
            # the wrapper: a block of torch's pinned cache (the flag LT_STEP_DST_PINNED is set)
            c0 = _packed(base)
            got = base.influence_matrix_host(probes, obs, 1e-4, mode, refresh=refresh)
            assert _packed(base) - c0 == packed, "the route the case is about was not taken"
            assert got.dtype == np.float64 and np.array_equal(got, want[:, :nob]), (route, refresh)
            assert torch.equal(_scratch(base), want_out), (route, refresh)
            # the raw entry into a dirty buffer with a padding column, with and without the caller's word that dst is pinned
            for flags in (PINNED, 0):
                rc, bp, bo, d, out = _step(base, probes, obs, mode, flags | (REFRESH if refresh else 0), gpu)
                assert (rc, bp, bo) == (0, 0, 0)
                assert np.array_equal(d[:, :nob], want[:, :nob]), (route, refresh, flags)
                assert np.all(d[:, nob:] == 7.0), (route, refresh, flags, "padding")
                assert torch.equal(out, want_out), (route, refresh, flags)
            assert chunked(), "the knobs of the case were lost on the way"


@pytest.mark.parametrize("npb,nob", [(1, NO), (NP, 1), (0, NO), (NP, 0), (0, 0)])
def test_single_and_empty_lists(gpu, npb, nob):
    with _knobs(aggregate_first=0):
        base, ref = _pair(gpu)
        probes, obs = _lists(gpu, npb=npb, nob=nob)
        assert (probes.numel(), obs.numel()) == (npb, nob)
        got = base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=True)
        assert got.shape == (npb, nob) and got.dtype == np.float64
        if npb and nob:
            rc, want, want_out = _calls(ref, probes, obs, "delta", True, gpu)
            assert rc == 0 and np.array_equal(got, want[:, :nob]) and torch.equal(_scratch(base), want_out)
        rc, bp, bo, d, _ = _step(base, probes, obs, "delta", REFRESH | PINNED, gpu)
        assert (rc, bp, bo) == (0, 0, 0) and np.all(d[:, nob:] == 7.0)
        if npb and nob:
            assert np.array_equal(d[:, :nob], want[:, :nob])
        assert _lib.lib().lt_node_check(None, None) == 0


@pytest.mark.parametrize("mode", ["delta", "sparse"])
def test_refresh_flag_follows_edited_weights(gpu, mode):
    from linkteller_amd import engine
    with _knobs(aggregate_first=0):
        base, ref = _pair(gpu)
        probes, obs = _lists(gpu)
        before = base.influence_matrix_host(probes, obs, 1e-4, mode, refresh=True).copy()
        rc, d, _ = _calls(ref, probes, obs, mode, True, gpu)
        assert np.array_equal(before, d[:, :obs.numel()])
        base.w1.mul_(1.25)
        base.b1.add_(0.01)
        # not refreshed: what the separate calls give without a refresh, bit for bit -- in `delta` the stale baseline's matrix
        # (`sparse` forms the perturbed rows from the weights as they are now, against the stale layers)
        stale = base.influence_matrix_host(probes, obs, 1e-4, mode, refresh=False)
        rc, d, _ = _calls(ref, probes, obs, mode, False, gpu)
        assert np.array_equal(stale, d[:, :obs.numel()])
        if mode == "delta":
            assert np.array_equal(stale, before)
        rc, d, _ = _calls(ref, probes, obs, mode, True, gpu)      # (ref shares the tensors: it sees the edited weights)
        fresh = engine.Baseline(base.graph, base.x, base.w1, base.b1, base.w2, base.b2)
        want = fresh.influence_matrix_host(probes, obs, 1e-4, mode, refresh=False)
        assert not np.array_equal(want, before)
        got = base.influence_matrix_host(probes, obs, 1e-4, mode, refresh=True)
        assert np.array_equal(got, want) and np.array_equal(got, d[:, :obs.numel()])


def test_refresh_follows_an_in_place_edit_of_the_features(gpu):
    from linkteller_amd import engine
    with _knobs(aggregate_first=0):
        base, ref = _pair(gpu)
        probes, obs = _lists(gpu)
        before = base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=True).copy()
        base.x[probes[:8].long()] *= 1.5
        base.x[obs[-1].long(), :5] += 0.25
        got = base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=True)
        fresh = engine.Baseline(base.graph, base.x, base.w1, base.b1, base.w2, base.b2)
        want = fresh.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=False)
        assert not np.array_equal(want, before)
        assert np.array_equal(got, want)
        rc, d, _ = _calls(ref, probes, obs, "delta", True, gpu)
        assert rc == 0 and np.array_equal(got, d[:, :obs.numel()])


@pytest.mark.parametrize("compact", [0, 2])
def test_bad_node_id_raises_from_that_very_call(gpu, compact):
    with _knobs(aggregate_first=0, export_compact=compact):
        base, ref = _pair(gpu)
        probes, obs = _lists(gpu)
        rc, want, want_out = _calls(ref, probes, obs, "delta", True, gpu)
        for which in ("probe", "observed"):
            p2, o2 = probes.clone(), obs.clone()
            (p2 if which == "probe" else o2)[5] = N + 3
            with pytest.raises(IndexError):
                base.influence_matrix_host(p2, o2, 1e-4, "delta", refresh=True)
            assert _lib.lib().lt_node_check(None, None) == 0, "the call did not clear the flag it reported"
            rc, bp, bo, _, _ = _step(base, p2, o2, "delta", REFRESH | PINNED, gpu)
            assert (rc, bp, bo) == (_lib.LT_ERR_INDEX, int(which == "probe"), int(which == "observed"))
            # the next call, good lists: succeeds, equals the separate calls, and the flag is clear
            got = base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=True)
            assert np.array_equal(got, want[:, :obs.numel()]) and torch.equal(_scratch(base), want_out)
            assert _lib.lib().lt_node_check(None, None) == 0


def test_a_refused_call_marks_nothing_stale(gpu):
    with _knobs(aggregate_first=0):
        base, _ = _pair(gpu)
        probes, obs = _lists(gpu)
        before = base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=True).copy()
        base.w1.mul_(1.25)
        rc, bp, bo, d, _ = _step(base, probes, obs, "delta", REFRESH | PINNED, gpu, out=None)      # out = NULL
        assert rc == -1 and (bp, bo) == (0, 0) and np.all(d == 7.0)
        small = torch.empty(256, dtype=torch.uint8, device=gpu)
        rc, bp, bo, d, _ = _step(base, probes, obs, "delta", REFRESH | PINNED, gpu, ws=small)
        assert rc == _lib.LT_ERR_WORKSPACE and np.all(d == 7.0)
        need = _ws(base, probes, obs, "delta", gpu).numel()
        assert f"needs {need} bytes" in _lib.lib().lt_last_error().decode()
        assert _lib.lib().lt_influence_step_host(base._h, probes.data_ptr(), NP, obs.data_ptr(), NO, 1e-4, 2, small.data_ptr(), NO,
                                                 d.ctypes.data, NO + 1, small.data_ptr(), 256, None, 4, None, None) == -1   # unknown flag
        # had any of them marked the baseline stale, this call would form it again from the edited weights
        assert np.array_equal(base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=False), before)
        assert not np.array_equal(base.influence_matrix_host(probes, obs, 1e-4, "delta", refresh=True), before)


class _Counting:
    """The library handle, counting the calls of some of its entries."""

    def __init__(self, handle, names):
        self._handle, self.count = handle, {k: 0 for k in names}

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if name not in self.count:
            return fn

        def counted(*a):
            self.count[name] += 1
            return fn(*a)
        return counted


def test_workspace_regrows_with_one_retry(gpu, monkeypatch):
    with _knobs(aggregate_first=0):
        base, ref = _pair(gpu)
        probes, obs = _lists(gpu, npb=120, nob=150)
        base.influence_matrix_host(probes[:4], obs[:5], 1e-4, "delta", refresh=True)
        small = next(iter(base._ws.values())).numel()
        cnt = _Counting(_lib.lib(), ("lt_influence_step_host", "lt_influence_workspace_bytes"))
        monkeypatch.setattr(_lib, "lib", lambda: cnt)

        def run(p, o):
            before = dict(cnt.count)
            m = base.influence_matrix_host(p, o, 1e-4, "delta", refresh=True)
            return m, {k: cnt.count[k] - before[k] for k in before}

        # a larger call after a smaller one: refused once, asked once, called again
        got, d = run(probes, obs)
        assert d == {"lt_influence_step_host": 2, "lt_influence_workspace_bytes": 1}
        assert next(iter(base._ws.values())).numel() > small
        rc, want, _ = _calls(ref, probes, obs, "delta", True, gpu)
        assert np.array_equal(got, want[:, :150])
        # the same call again: the cached workspace as it is
        got, d = run(probes, obs)
        assert d == {"lt_influence_step_host": 1, "lt_influence_workspace_bytes": 0} and np.array_equal(got, want[:, :150])
        # a knob change that enlarges the workspace of the same shapes.  "delta_fused" = 0 moves the call to the item kernels but the
        # workspace is carved for both routes whatever the knob says: same size, no retry, same matrix ...
        fused = next(iter(base._ws.values())).numel()
        with _knobs(delta_fused=0):
            assert _ws(base, probes, obs, "delta", gpu).numel() == fused
            got, d = run(probes, obs)
            assert d == {"lt_influence_step_host": 1, "lt_influence_workspace_bytes": 0}
            rc, want0, _ = _calls(ref, probes, obs, "delta", True, gpu)
            assert np.array_equal(got, want0[:, :150]) and np.array_equal(want0, want)
        # ... the probe chunk's budget does size it: a workspace cached under a small budget is too small once the budget is back
        with _knobs(chunk_budget_bytes=_two_chunk_budget(120)):
            base._ws = {}
            got, d = run(probes, obs)
            assert d == {"lt_influence_step_host": 1, "lt_influence_workspace_bytes": 1} and np.array_equal(got, want[:, :150])
            chunked = next(iter(base._ws.values())).numel()
        assert chunked < fused
        got, d = run(probes, obs)
        assert d == {"lt_influence_step_host": 2, "lt_influence_workspace_bytes": 1} and np.array_equal(got, want[:, :150])
        assert next(iter(base._ws.values())).numel() == fused

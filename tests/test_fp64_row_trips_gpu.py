"""The two fp64 arrays of the delta step read back as stored (lt_baseline_fp64_arrays / Baseline.fp64_arrays), and the reference
vector's product m W1 that the last slab block of the product rows' launch sums (fd_slab_block, lt_fp64.hip): that sum is a chain
of loads that pass the L2, cut from eight dependent trips to two with the order of every addition kept -- so cref is compared BIT FOR
BIT with the documented association restated in numpy (`delta`'s own output rounds the pre-activation once to fp32 and would hardly
see a reordered fp64 sum), at the slab counts and widths where the new loop changes its path."""
import contextlib
import functools
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu
DELTA = 1e-4


@contextlib.contextmanager
def knobs(**kn):
    from linkteller_amd import _lib
    try:
        for k, v in kn.items():
            _lib.set_tuning(k, v)
        yield
    finally:
        for k in kn:
            _lib.set_tuning(k, None)


def _ref_vector(x):
    """k_ref_vector: the more frequent of (min, max) of each column over the first <= 64 rows, the minimum on a tie."""
    head = x[:64]
    mn, mx = head.min(axis=0), head.max(axis=0)
    return np.where(2 * (head == mn).sum(axis=0) >= head.shape[0], mn, mx)


def restate_cref(m, w1):
    """cref = m W1 in the association of fd_slab_block: slice z holds columns k in [64 z, 64 z + 64); quarter kq of it is an fma chain
    over its 16 k's in order from +0 (the product of two fp32 values is exact in fp64, so fma(a, b, c) is a * b + c rounded once);
    the slice is ((q0 + q1) + q2) + q3; partial sum p of the last block adds the slices p, p + 4, ... in order from +0; cref is
    ((p0 + p1) + p2) + p3."""
    f, h = w1.shape
    m64, w64 = m.astype(np.float64), w1.astype(np.float64)
    nslab = (f + 63) // 64
    slabs = np.zeros((nslab, h))
    for z in range(nslab):
        q = np.zeros((4, h))
        for kq in range(4):
            for k in range(64 * z + 16 * kq, min(f, 64 * z + 16 * kq + 16)):
                q[kq] = q[kq] + m64[k] * w64[k]
        slabs[z] = ((q[0] + q[1]) + q[2]) + q[3]
    p = np.zeros((4, h))
    for z in range(nslab):
        p[z % 4] = p[z % 4] + slabs[z]
    return ((p[0] + p[1]) + p[2]) + p[3]


@functools.lru_cache(maxsize=None)
def _case(n, f, h):
    from linkteller_amd import graph, synth
    x = synth.twitch_like_features(n, f, seed=f + h, density=0.02)
    w = synth.gcn_weights(f, h, 2, seed=h)
    a_hat = graph.first_order_gcn(synth.erdos_renyi_graph(n, 4 * n, seed=3))
    rng = np.random.RandomState(n + f)
    probes = rng.choice(n, 24, replace=False).astype(np.int64)
    return types.SimpleNamespace(a_hat=a_hat, hg=graph.HipGraph(a_hat), x=x, w=w, n=n, f=f, h=h, probes=probes, obs=np.arange(n, dtype=np.int64))


def _baseline(cs, **kn):
    """A baseline on the feature-difference route with the `delta` rows formed once; the weights' device tensors (borrowed)."""
    from linkteller_amd import engine
    dev = torch.device("cuda")
    par = [torch.from_numpy(cs.w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")]
    base = engine.Baseline(cs.hg, torch.from_numpy(cs.x).to(dev), *par).enable_fp64()
    assert base.fp64_route() == 1
    rows = base.influence_rows(cs.probes, cs.obs, DELTA, "delta").clone()
    return base, par, rows


# F = 3170 / 3171: 50 slices, one pass of the sum's 52; 3328 + 1: 53 slices, the second pass holds one; 4200: 66; 192: 3 slices (the
# fourth partial sum has none); 200: a last slice of 8 columns.  H = 256: two column trips; 132: the second trip holds 4 live columns of
# 128; 64: one trip, its second group clamped; 8: two live lanes.
SHAPES = [(3170, 256), (3171, 256), (3329, 256), (4200, 256), (192, 256), (200, 132), (3170, 132), (3170, 64), (200, 8)]


@pytest.mark.parametrize("f,h", SHAPES)
def test_the_last_slab_block_sums_in_the_documented_order(gpu, f, h):
    """cref, as the launch left it, equals the restated association bit for bit -- before and behind a refresh with changed weights
    (the gate word must have been left ready for the second launch)."""
    cs = _case(301, f, h)
    with knobs(feature_delta=1, defer_cref=1, aggregate_first=0):
        base, par, rows = _baseline(cs)
        a = base.fp64_arrays()
        assert a["deferred_cref"], "the slab blocks did not run: the case does not reach the changed code"
        m = _ref_vector(cs.x)
        assert np.array_equal(a["cref"].cpu().numpy()[:h], restate_cref(m, cs.w["W1"]))
        assert not a["cref"].cpu().numpy()[h:].any()
        par[0].mul_(1.25)
        base.refresh()
        again = base.influence_rows(cs.probes, cs.obs, DELTA, "delta")
        assert not torch.equal(rows, again)
        w1 = par[0].cpu().numpy()
        assert np.array_equal(base.fp64_arrays()["cref"].cpu().numpy()[:h], restate_cref(m, w1))
        torch.cuda.synchronize()


def _check_arrays(cs, a, fixed, deferred):
    """What fp64_arrays returned against numpy float64: the product rows (fixed point x scale, or doubles; plus cref where it is
    deferred) against X W1 within one unit of the 31-bit fixed point of the STORED row (2^-31 of its largest value -- the row
    without cref where cref is deferred, which for features far from their reference vector is larger than the row itself; fp64
    rows: 1e-12), the pre-activation against A_hat S1 + b1 within its fp32 rounding (2^-23 |z|; fp64: none) plus the rows'
    storage error through the row's entries (2^-30 sum|A| max|stored|)."""
    assert a["deferred_cref"] == deferred
    assert (a["scales"] is not None) == fixed
    assert a["valid"].all()
    s1 = cs.x.astype(np.float64) @ cs.w["W1"].astype(np.float64)
    got = a["product"].cpu().numpy().astype(np.float64)
    if fixed:
        assert a["product"].dtype == torch.int32
        got = got * a["scales"].cpu().numpy()[:, None]
    if a["deferred_cref"]:
        got = got + a["cref"].cpu().numpy()[None, :]
    h = cs.w["W1"].shape[1]
    assert not got[:, h:].any()          # (pad columns: zeros as stored)
    got = got[:, :h]
    # (what is stored, and scaled by its own largest value, is the row WITHOUT cref where cref is deferred)
    stored = s1 - a["cref"].cpu().numpy()[None, :h] if a["deferred_cref"] else s1
    top = np.abs(stored).max(axis=1, keepdims=True)
    err = np.abs(got - s1) / top
    print(f"product rows: largest error {err.max():.3g} of the stored row's largest value")
    assert err.max() <= (2.0 ** -31 if fixed else 1e-12)
    av = sp.csr_matrix(cs.a_hat).astype(np.float32).astype(np.float64)
    z = av @ s1 + cs.w["b1"].astype(np.float64)[None, :]
    pre = a["preact"].cpu().numpy()
    assert pre.dtype == (np.float32 if fixed else np.float64)
    bound = 2.0 ** -23 * np.abs(z) + 2.0 ** -30 * np.asarray(abs(av).sum(axis=1)).reshape(-1, 1) * np.abs(stored).max()
    assert np.all(np.abs(pre[:, :h].astype(np.float64) - z) <= bound)


@pytest.mark.parametrize("s1_f32", [1, 0])
@pytest.mark.parametrize("defer_cref", [1, 0])
def test_arrays_hold_the_fp64_product_and_pre_activation(gpu, s1_f32, defer_cref):
    cs = _case(301, 3170, 256)
    with knobs(feature_delta=1, defer_cref=defer_cref, s1_f32=s1_f32, aggregate_first=0, z_on_demand=0):
        base, par, rows = _baseline(cs)
        a = base.fp64_arrays()
        torch.cuda.synchronize()
    _check_arrays(cs, a, s1_f32 == 1 and defer_cref == 1, bool(defer_cref))


@functools.lru_cache(maxsize=None)
def _ladder_case(name, h):
    """boundary_cases' ladders: short_ladder (rows of exactly K - 1, K, K + 1 entries up to 128, 0 / 1 / 2; the fused route) and
    hub_ladder (hub rows: the segment blocks and k_spmm_f64_long), with their own features, weights and node lists."""
    import boundary_cases as B
    from linkteller_amd import graph
    g = B.graph_of(name)
    probes, obs = B.node_lists(name)
    return types.SimpleNamespace(a_hat=g.a, hg=graph.HipGraph(g.a), x=B.features(name), w=B.weights(h, 2), n=g.n, probes=probes, obs=obs)


@functools.lru_cache(maxsize=None)
def _directed_case(h):
    """A small directed graph: n = 203 (no multiple of 4), a pool of 190 nodes (self loop + two pool entries each), rows of exactly
    15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64 and 65 pool entries, a row of one entry; twitch-like features."""
    from linkteller_amd import graph, synth
    lengths = (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)
    n_pool, n = 190, 203
    rng = np.random.RandomState(7)
    rows, cols, vals = [], [], []
    for r in range(n_pool):
        c = np.concatenate([[r], (r + 1 + rng.choice(n_pool - 1, 2, replace=False)) % n_pool])
        rows += [r] * 3; cols += list(c); vals += [0.5, 0.2, 0.3]
    for k, d in enumerate(lengths):
        rows += [n_pool + k] * d; cols += list(np.sort(rng.choice(n_pool, d, replace=False))); vals += list(rng.uniform(0.5, 1.5, d) / d)
    rows += [n - 1]; cols += [3]; vals += [1.0]
    a = sp.csr_matrix((np.asarray(vals), (np.asarray(rows), np.asarray(cols))), shape=(n, n))
    a.sort_indices()
    assert sorted(np.diff(a.indptr)[n_pool:n_pool + len(lengths)]) == list(lengths)
    f = 192
    nodes = np.arange(n).astype(np.int64)
    return types.SimpleNamespace(a_hat=a, hg=graph.HipGraph(a), x=synth.twitch_like_features(n, f, seed=5, density=0.05),
                                 w=synth.gcn_weights(f, h, 2, seed=h), n=n, probes=nodes[:n_pool:3], obs=nodes)


@pytest.mark.parametrize("kind,h", [("short", 256), ("short", 130), ("hub", 256), ("hub", 132), ("directed", 130), ("directed", 256)])
def test_arrays_on_the_ladders_and_a_directed_graph(gpu, kind, h):
    """The same value checks where the SpMM changes its path: every row length up to 128, hub rows in segments, rows of 15 .. 65
    entries in a directed graph whose n is no multiple of 4; H = 256, 132 (33 live lanes) and 130 (Hp != H: no deferred cref,
    fp64 rows)."""
    cs = _directed_case(h) if kind == "directed" else _ladder_case(kind, h)
    with knobs(feature_delta=1, aggregate_first=0, z_on_demand=0):
        base, par, rows = _baseline(cs)
        a = base.fp64_arrays()
        torch.cuda.synchronize()
    assert rows.max() > 0
    _check_arrays(cs, a, h % 4 == 0, h % 4 == 0)


def test_ring_form_sums_the_slices_in_the_same_order(gpu):
    """k_s1d_feature_ring ("feature_ring" = 1) runs the same slab blocks in front of its workgroups: cref bit for bit as restated;
    that the ring form ran shows in the product rows, which differ from the row-per-wave form's in fp64 summation order."""
    cs = _case(301, 3170, 256)
    got = {}
    for ring in (0, 1):
        with knobs(feature_delta=1, defer_cref=1, aggregate_first=0, feature_ring=ring, s1_f32=0):
            base, par, rows = _baseline(cs)
            a = base.fp64_arrays()
            assert a["deferred_cref"]
            got[ring] = (a["cref"].cpu().numpy(), a["product"].cpu().numpy())
            torch.cuda.synchronize()
    want = restate_cref(_ref_vector(cs.x), cs.w["W1"])
    assert np.array_equal(got[0][0], want) and np.array_equal(got[1][0], want)
    assert not np.array_equal(got[0][1], got[1][1]), "the ring form did not run: its rows carry the row-per-wave form's bits"
    assert np.abs(got[0][1] - got[1][1]).max() <= 1e-12 * np.abs(got[0][1]).max()


def test_delta_against_the_fp64_oracle(gpu):
    """`delta` within 1e-5 of the largest score of the fp64 oracle with exact zeros, as the route tests hold it."""
    from test_gpu_parity import _oracle_matrix
    cs = _case(301, 3170, 256)
    ref64 = _oracle_matrix(cs.a_hat, cs.x, cs.w, cs.probes[:8], cs.obs, DELTA, torch.float64)
    with knobs(feature_delta=1, aggregate_first=0):
        got = _baseline(cs)[2].cpu().numpy().astype(np.float64)[:8]
    top = ref64.max()
    print(f"largest error {np.abs(got - ref64).max() / top:.3g} of the largest score")
    assert top > 0 and np.abs(got - ref64).max() <= 1e-5 * top
    assert np.all(got[ref64 == 0] == 0)


def test_rows_formed_on_demand_are_marked(gpu):
    """"z_on_demand" = 1: a call forms the rows its items read; "valid" names them and they carry the bits of the all-rows form."""
    cs = _case(301, 3170, 256)
    few = types.SimpleNamespace(**{**cs.__dict__, "probes": cs.probes[:3]})
    with knobs(feature_delta=1, aggregate_first=0, z_on_demand=0):
        every = _baseline(few)[0].fp64_arrays()
    with knobs(feature_delta=1, aggregate_first=0, z_on_demand=1):
        some = _baseline(few)[0].fp64_arrays()
        torch.cuda.synchronize()
    assert every["valid"].all()
    v = some["valid"]
    assert 0 < int(v.sum()) < cs.n, "the call formed every row: not the on-demand route"
    assert some["preact"].dtype == every["preact"].dtype and torch.equal(some["preact"][v], every["preact"][v])


def test_refused_without_product_rows_and_before_the_first_call(gpu):
    from linkteller_amd import _lib, engine
    cs = _case(301, 3170, 256)
    dev = torch.device("cuda")
    par = [torch.from_numpy(cs.w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")]
    with knobs(aggregate_first=1):      # (hub_ladder: the graph test_boundary_gpu takes this route on)
        import boundary_cases as B
        from linkteller_amd import graph
        wl = B.weights(64, 3)
        agg = engine.Baseline(graph.HipGraph(B.graph_of("hub").a), torch.from_numpy(B.features("hub")).to(dev),
                              *[torch.from_numpy(wl[k]).to(dev) for k in ("W1", "b1", "W2", "b2")]).enable_fp64()
        assert agg.fp64_route() == 2
        with pytest.raises(_lib.LinkTellerHipError):
            agg.fp64_arrays()
    with knobs(aggregate_first=0, feature_delta=1):
        base = engine.Baseline(cs.hg, torch.from_numpy(cs.x).to(dev), *par).enable_fp64()
        base.fp64_arrays()          # (enable_fp64 forms the product once)
        base.refresh()
        with pytest.raises(_lib.LinkTellerHipError):
            base.fp64_arrays()

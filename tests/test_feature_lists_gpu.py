"""The difference lists of X kept per baseline ("feature_lists", lt_fp64.hip): the refresh of the feature-difference route reads each
row's differing columns from lists built once by lt_baseline_enable_fp64 instead of listing them from X again.  The lists are the
wave's own LDS list entry for entry, so every result keeps its bits across the knob; `delta` stays within 1e-5 of the largest
score of the fp64 oracle with exact zeros (the bounds of the route tests); a refresh announces changed weights, changed features
are seen through torch's version counter or announced with features_changed()."""
import contextlib
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DELTA = 1e-4


@contextlib.contextmanager
def knobs(**kn):
    from linkteller_amd import _lib
    for k, v in kn.items():
        _lib.set_tuning(k, v)
    try:
        yield
    finally:
        for k in kn:
            _lib.set_tuning(k, None)


def _params(w, dev):
    return [torch.from_numpy(w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")]


def _ref_vector(x):
    """k_ref_vector: the more frequent of (min, max) of each column over the first <= 64 rows, the minimum on a tie."""
    head = x[:64]
    mn, mx = head.min(axis=0), head.max(axis=0)
    return np.where(2 * (head == mn).sum(axis=0) >= head.shape[0], mn, mx)


def _hand_made(n, f):
    """Rows (behind the 64 the reference vector is taken from) with exactly 0, 1, 6, 7, 198, 199 and 384 differing columns: around
    FD_PU = 6, around fd_hint_cap(3170) = 198, and a full list."""
    from linkteller_amd import synth
    x = synth.twitch_like_features(n, f, seed=11, density=0.006)
    m = _ref_vector(x)
    rs = np.random.RandomState(5)
    rows = {}
    for k, cnt in enumerate((0, 1, 6, 7, 198, 199, 384)):
        r = 70 + 13 * k
        x[r] = m
        cols = rs.choice(f, cnt, replace=False)
        x[r, cols] = m[cols] + 1.5 + 0.25 * rs.randint(0, 4, cnt).astype(np.float32)
        rows[cnt] = r
    return x, rows


@functools.lru_cache(maxsize=None)
def _case(name):
    """Graph, features, weights, node lists with nodes 0 and n - 1 probed and observed (the first row of X and the shifted last
    window), the fp64 oracle of the first 8 probes: once per case."""
    from test_gpu_parity import _oracle_matrix
    from linkteller_amd import graph, synth
    n, f, h, pl, pin = {"er": (1301, 3170, 256, False, False), "odd_f": (1301, 3171, 256, False, False),
                        "two_trips": (1301, 4200, 256, False, False), "h30": (1301, 3170, 30, False, False),
                        "h64": (1301, 3170, 64, False, False), "hand_made": (1301, 3170, 256, False, True),
                        "row_385": (1301, 3170, 256, False, True), "power_law": (1301, 3170, 256, True, False)}[name]
    adj = synth.powerlaw_graph(n, 6000, seed=3) if pl else synth.erdos_renyi_graph(n, 5000, seed=3)
    a_hat = graph.first_order_gcn(adj)
    special = []
    if name == "hand_made":
        x, rows = _hand_made(n, f)
        special = sorted(rows.values())
    else:
        x = synth.twitch_like_features(n, f, seed=f + h, density=0.006)
        x[n - 1, f - 1] = 2.5
        x[0, 0] = -1.5
        if name == "row_385":
            m = _ref_vector(x)
            cols = np.random.RandomState(2).choice(f, 385, replace=False)
            x[200] = m
            x[200, cols] = m[cols] + 2.0
            special = [200]
    w = synth.gcn_weights(f, h, 2, seed=h)
    rng = np.random.RandomState(f + h)
    inner = np.setdiff1d(np.arange(1, n - 1), special)
    probes = np.concatenate([[0, n - 1], special, rng.choice(inner, 30 - len(special), replace=False)]).astype(np.int64)
    obs = np.concatenate([[n - 1, 0], special, rng.choice(inner, 120, replace=False)]).astype(np.int64)
    ref64 = _oracle_matrix(a_hat, x, w, probes[:8], obs, DELTA, torch.float64)
    assert ref64.max() > 0
    diffs = int((x != _ref_vector(x)[None, :]).sum())
    return types.SimpleNamespace(a_hat=a_hat, hg=graph.HipGraph(a_hat), x=x, w=w, n=n, f=f, h=h, probes=probes, obs=obs, ref64=ref64,
                                 pin=pin, diffs=diffs)


def _build(cs, gpu, lists, want_lists=True, x_dev=None):
    """One baseline under "feature_lists" = lists: the `delta` rows, the host matrix, and the rows again behind a refresh."""
    from linkteller_amd import engine
    kn = {"feature_lists": lists}
    if cs.pin:
        kn["feature_delta"] = 1          # (rows beyond the hint cap would retire the route at the probe of enable_fp64)
    with knobs(**kn):
        xt = torch.from_numpy(cs.x).to(gpu) if x_dev is None else x_dev
        base = engine.Baseline(cs.hg, xt, *_params(cs.w, gpu)).enable_fp64()
        assert base.fp64_route() == 1
        # (the lists are built whatever the knob says: the knob chooses the kernel of a refresh)
        assert base.feature_list_entries() == (cs.diffs if want_lists else -1)
        rows = base.influence_rows(cs.probes, cs.obs, DELTA, "delta").clone()
        host = base.influence_matrix_host(cs.probes, cs.obs, DELTA, "delta").copy()
        base.refresh()
        again = base.influence_rows(cs.probes, cs.obs, DELTA, "delta")
        assert torch.equal(rows, again)
        torch.cuda.synchronize()
    return rows, host


def _check_oracle(cs, rows):
    got = rows.cpu().numpy().astype(np.float64)[:8]
    top = cs.ref64.max()
    print(f"largest error {np.abs(got - cs.ref64).max() / top:.3g} of the largest score")
    assert np.abs(got - cs.ref64).max() <= 1e-5 * top
    assert np.all(got[cs.ref64 == 0] == 0)


@pytest.mark.parametrize("name", ["er", "odd_f", "two_trips", "h30", "h64", "hand_made", "power_law"])
def test_listed_rows_keep_every_bit(gpu, name):
    """n = 1301 (no multiple of a block's 4 waves), F = 3170 / 3171 (VEC = 1) / 4200 (two trips: the ballot order on every row),
    H = 256 / 64 / 30 (the lanes' scalar walk, Hp != H), rows of 0, 1, 6, 7, 198, 199 and exactly 384 differing columns, a
    power-law graph (the hub blocks and the SpMM's long rows read the listed rows)."""
    cs = _case(name)
    r0, h0 = _build(cs, gpu, 0)
    r1, h1 = _build(cs, gpu, 1)
    assert torch.equal(r0, r1)
    assert np.array_equal(h0, h1)
    _check_oracle(cs, r1)


def test_a_row_beyond_the_list_keeps_the_baseline_without_lists(gpu):
    """385 differing columns in one row: no lists are built, "feature_lists" = 1 is "feature_lists" = 0."""
    cs = _case("row_385")
    r0, h0 = _build(cs, gpu, 0, want_lists=False)
    r1, h1 = _build(cs, gpu, 1, want_lists=False)
    assert torch.equal(r0, r1) and np.array_equal(h0, h1)
    _check_oracle(cs, r1)


def test_strided_offset_window_of_x(gpu):
    """X as a window with ldx = F + 3 at element offset 1 (rows at odd alignment: the VEC = 1 instantiation builds the lists)
    through the raw C ABI."""
    import abi_views as V
    from linkteller_amd import _lib
    cs = _case("er")
    out = {}
    for lists in (0, 1):
        with knobs(feature_lists=lists):
            base = V.RawBaseline(cs.hg, V.View(cs.x, cs.f + 3, 1), cs.f, *[V.View(cs.w[k]) for k in ("W1", "b1")], cs.h,
                                 *[V.View(cs.w[k]) for k in ("W2", "b2")], 2)
            try:
                base.enable_fp64()
                assert base.fp64_route() == 1
                e = C.c_int64(-2)
                _lib.check(_lib.lib().lt_baseline_feature_list_entries(base._h, C.byref(e)), "lt_baseline_feature_list_entries")
                assert e.value == cs.diffs
                a = base.rows(cs.probes, cs.obs, DELTA, "delta", V.View.output(len(cs.probes), len(cs.obs))).copy()
                dst = torch.full((len(cs.probes) * len(cs.obs),), -1.0, dtype=torch.float64).pin_memory()
                base.matrix_host(cs.probes, cs.obs, DELTA, "delta", V.View.output(len(cs.probes), len(cs.obs)), dst, len(cs.obs))
                host = dst.numpy().reshape(len(cs.probes), len(cs.obs)).copy()
                base.refresh()
                b = base.rows(cs.probes, cs.obs, DELTA, "delta", V.View.output(len(cs.probes), len(cs.obs)))
                assert np.array_equal(a, b)
                out[lists] = (a, host)
            finally:
                base.destroy()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    got = out[1][0].astype(np.float64)[:8]
    assert np.abs(got - cs.ref64).max() <= 1e-5 * cs.ref64.max()
    assert np.all(got[cs.ref64 == 0] == 0)


def _hip():
    """The HIP runtime torch itself loaded (hipMemcpy: a write torch's version counter does not see)."""
    import os
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    lib = C.CDLL(path if os.path.exists(path) else "libamdhip64.so")
    lib.hipMemcpy.restype = C.c_int
    return lib


def _fresh_rows(cs, gpu, xt, params):
    from linkteller_amd import engine
    fresh = engine.Baseline(cs.hg, xt.clone(), *[p.clone() for p in params]).enable_fp64()
    assert fresh.fp64_route() == 1 and fresh.feature_list_entries() >= 0
    return fresh.influence_rows(cs.probes, cs.obs, DELTA, "delta").clone()


def test_changed_weights_and_changed_features(gpu):
    """W1 changed in place + refresh(); x[3, 17] = 4.0 through torch + refresh() (the version counter); the same write through
    the raw pointer + features_changed(): each gives the bits of a fresh baseline, and differs from what went before."""
    from linkteller_amd import engine
    cs = _case("er")
    xt = torch.from_numpy(cs.x).to(gpu)
    params = _params(cs.w, gpu)
    base = engine.Baseline(cs.hg, xt, *params).enable_fp64()
    assert base.feature_list_entries() == cs.diffs
    probes = np.concatenate([[3], cs.probes])
    cs3 = types.SimpleNamespace(**{**vars(cs), "probes": probes})
    first = base.influence_rows(probes, cs.obs, DELTA, "delta").clone()
    params[0].mul_(0.75)
    base.refresh()
    got = base.influence_rows(probes, cs.obs, DELTA, "delta").clone()
    assert base.feature_list_entries() == cs.diffs
    assert torch.equal(got, _fresh_rows(cs3, gpu, xt, params)) and not torch.equal(got, first)
    # through torch: refresh() sees the version counter
    assert cs.x[3, 17] != 4.0
    xt[3, 17] = 4.0
    base.refresh()
    got2 = base.influence_rows(probes, cs.obs, DELTA, "delta").clone()
    assert base.feature_list_entries() == cs.diffs + 1
    assert torch.equal(got2, _fresh_rows(cs3, gpu, xt, params)) and not torch.equal(got2, got)
    # behind torch's back: the same write through the raw pointer, to a baseline of its own, announced with features_changed()
    xr = torch.from_numpy(cs.x).to(gpu)
    raw = engine.Baseline(cs.hg, xr, *params).enable_fp64()
    before = raw.influence_rows(probes, cs.obs, DELTA, "delta").clone()
    word = torch.tensor([4.0], dtype=torch.float32)
    torch.cuda.synchronize()
    assert _hip().hipMemcpy(C.c_void_p(xr.data_ptr() + 4 * (3 * cs.f + 17)), C.c_void_p(word.data_ptr()), C.c_size_t(4), 1) == 0
    version = xr._version
    raw.features_changed()
    assert xr._version == version and float(xr[3, 17]) == 4.0
    got3 = raw.influence_rows(probes, cs.obs, DELTA, "delta").clone()
    assert raw.feature_list_entries() == cs.diffs + 1
    assert torch.equal(got3, got2) and not torch.equal(got3, before)


def test_flag_knob_changed_after_the_build(gpu):
    """Lists built under "feature_flags" = 1 are not used under 0 (the knob decides their order): the result is that of a baseline
    that never had lists under "feature_flags" = 0."""
    from linkteller_amd import engine
    cs = _case("er")
    xt = torch.from_numpy(cs.x).to(gpu)
    with knobs(feature_flags=0, feature_lists=0):
        want = engine.Baseline(cs.hg, xt, *_params(cs.w, gpu)).enable_fp64().influence_rows(cs.probes, cs.obs, DELTA, "delta").clone()
    base = engine.Baseline(cs.hg, xt, *_params(cs.w, gpu)).enable_fp64()
    assert base.feature_list_entries() == cs.diffs
    base.influence_rows(cs.probes, cs.obs, DELTA, "delta")
    with knobs(feature_flags=0):
        base.refresh()
        got = base.influence_rows(cs.probes, cs.obs, DELTA, "delta").clone()
    assert torch.equal(got, want)


def _small_sparse(n, f, seed):
    from linkteller_amd import graph, synth
    a_hat = graph.first_order_gcn(synth.powerlaw_graph(n, 1400, seed=seed))
    x = synth.twitch_like_features(n, f, seed=seed + 1, density=0.02)
    rng = np.random.RandomState(seed)
    return graph.HipGraph(a_hat), x, rng.choice(n, 37, replace=False), rng.choice(n, 50, replace=False)


def _across_the_knob(make, probes, obs, entries):
    out = []
    for lists in (0, 1):
        with knobs(feature_lists=lists):
            base = make()
            a = base.influence_rows(probes, obs, DELTA, "delta").clone()
            assert entries(base) >= 0
            base.refresh()
            assert torch.equal(a, base.influence_rows(probes, obs, DELTA, "delta"))
            base.features_changed()
            assert torch.equal(a, base.influence_rows(probes, obs, DELTA, "delta"))
            out.append(a)
    assert torch.equal(out[0], out[1]) and float(out[1].abs().max()) > 0


def test_wide_baseline_across_the_knob(gpu):
    """WideBaseline (H = 320: slices of 256 and 64, 12 classes in two slices) on sparse-difference features: every slice's baseline
    keeps lists, refresh() and features_changed() reach them."""
    from linkteller_amd import engine, synth
    hg, x, probes, obs = _small_sparse(300, 512, seed=3)
    w = synth.gcn_weights(512, 320, 12, seed=5)
    xt = torch.from_numpy(x).to(gpu)

    def make():
        base = engine.baseline_for(hg, xt, *_params(w, gpu))
        assert isinstance(base, engine.WideBaseline)
        return base

    _across_the_knob(make, probes, obs, lambda b: min(sub.feature_list_entries() for sub, _ in b._subs.values()))


def test_baseline3_across_the_knob(gpu):
    """Baseline3: the inner 2-layer baseline keeps the lists; lt_baseline3_refresh / lt_baseline3_features_changed forward."""
    from linkteller_amd import _lib, engine
    hg, x, probes, obs = _small_sparse(300, 512, seed=9)
    rng = np.random.RandomState(4)
    f, h1, h2, c = 512, 64, 32, 3

    def u(shape, fan):
        s = 1.0 / np.sqrt(fan)
        return torch.from_numpy(rng.uniform(-s, s, size=shape).astype(np.float32)).to(gpu)

    p = [u((f, h1), h1), u((h1,), h1), u((h1, h2), h2), u((h2,), h2), u((h2, c), c), u((c,), c)]
    xt = torch.from_numpy(x).to(gpu)
    _across_the_knob(lambda: engine.Baseline3(hg, xt, *p).enable_fp64(), probes, obs, lambda b: 0)

"""The wide 2-layer handle (lt_baseline2w_create, lt_influence2w_rows, lt_influence2w_pairs) at the shapes and on the storage forms the
rest of the suite leaves out (wide2_shape_cases.py; their conditions: test_wide2_shapes_cpu.py):

  1. the (H, C) ladder over every lane-group width of k3d_items1<LPR>, k3dw_stageC<LPR> and k3dw_stageC_pairs<LPR> and over the tile
     edges of the product dS2x = dH1x W2, on two small graphs: `delta` within 1e-5 of the largest score of the fp64 oracle
     (oracle.linkteller_oracle.influence_matrix, as test_wide2_handle_gpu._oracle calls it) on both routes of the probes' product
     rows, exact zeros, the all-zero probe, logits() against the fp64 forward; on four padded shapes the relations that need no
     tolerance: chunking, subsets of either list, the pair list, a workspace full of NaN, a weight update;
  2. every storage form the inner fp64 baseline can hold (int8 split with one and with several K slices, f64 matrix cores, fixed-point
     and plain fp64 rows, the feature-difference route with its cref deferred and carried, the tiled fp64 SpMM, the 128-wide tiles),
     each PROVEN by a narrow twin: the rules that pick a form depend on shapes, knobs and X alone, so engine.Baseline on the same
     (graph, X, W1, b1) under the same knobs (plus aggregate_first = 0, which the handle's inner baseline is pinned to) decides as the
     inner baseline does, and lt_baseline_fp64_route / lt_baseline_fp64_arrays show what it decided;
  3. probe bitmaps of 516 words, a chunk of 300 probes, the cap of 65534 probes per chunk, and item counts at the 64-row tile edges
     of the product over the items;
  4. strided and 4-byte aligned operands through the C ABI;
  5. the same storage forms behind the 3-layer handles, which read them through the same two functions.

Every case builds its own handle inside its knobs (the storage knobs are read when the fp64 product is formed); the oracle matrices
are computed once per process and shared with the CPU file."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import abi_views as V
import gcn3_shape_cases as S
import wide2_shape_cases as W
from linkteller_amd import _lib
from test_gcn3_shapes_gpu import knobs
from test_gcn3_wide_attack_gpu import _wide3
from test_wide2_handle_gpu import DELTA, KEYS, _hip, _pairs

pytestmark = pytest.mark.gpu

GATE = W.GATE


# ---- handles, checks -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hg(name):
    from linkteller_amd import graph
    a_hat = {"big": lambda: W.big_graph2()[0], "er29": lambda: S.small_graph("er29")[0]}.get(name, lambda: W.small_graph(name)[0])()
    return graph.HipGraph(a_hat)


def _dev(params, keys, gpu):
    return [torch.from_numpy(np.array(params[k], dtype=np.float32)).to(gpu) for k in keys]


def _make(name, x, params, gpu):
    from linkteller_amd import engine
    dev = _dev(params, KEYS, gpu)
    xt = torch.from_numpy(np.array(x, dtype=np.float32)).to(gpu)
    base = engine.Baseline2W(_hg(name), xt, *dev)
    assert (base.h, base.c) == params["W2"].shape
    return base, dev, xt


def _rows(base, probes, obs):
    """into an output full of NaN: a cell nobody wrote keeps it"""
    out = torch.full((len(probes), len(obs)), float("nan"), dtype=torch.float32, device=base.x.device)
    got = base.influence_rows(probes, obs, DELTA, "delta", out=out).cpu().numpy()
    assert np.isfinite(got).all()
    return got


def _cells(base, probes, ptr, pobs):
    out = torch.full((len(pobs),), float("nan"), dtype=torch.float32, device=base.x.device)
    got = base.influence_pairs(probes, ptr, pobs, DELTA, "delta", out=out).cpu().numpy()
    assert np.isfinite(got).all()
    return got


def _check_delta(got, ref, zrow, what):
    got = got.astype(np.float64)
    err = np.abs(got - ref).max() / ref.max()
    print(f"wide2shape {what}: max {ref.max():.3g} zeros {(ref == 0).mean():.2f} |ours - ref64| / max = {err:.2e}")
    assert ref.max() > 0 and err <= GATE, (what, err)
    assert np.all(got[ref == 0] == 0) and not np.signbit(got).any(), what
    if zrow is not None:
        assert np.all(ref[zrow] == 0) and np.all(got[zrow] == 0), what      # the all-zero feature row: nothing to perturb
    return err


def _check_logits(base, a_hat, x, params, what):
    ref = W.logits64(a_hat, x, params)
    got = base.logits().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max()
    print(f"wide2shape {what}: logits |ours - ref64| = {err:.2e} of max {np.abs(ref).max():.3g}")
    assert got.shape == ref.shape and err <= 2e-5 * np.abs(ref).max() + 1e-6, (what, err)


def _finish():
    from linkteller_amd import engine
    torch.cuda.synchronize()
    engine.node_check()


def _need(base, n_probe, n_obs):
    return _lib.lib().lt_influence2w_workspace_bytes(base._h, n_probe, n_obs)


# ---- 1. the lane-group ladder ----------------------------------------------------------------------------------------------------
SMALL = [(g, s) for g in W.GRAPHS for s in W.LADDER]


@pytest.mark.parametrize("name,shape", SMALL, ids=[f"{g}-{W.shape_id(s)}" for g, s in SMALL])
def test_delta_and_logits_on_the_ladder(gpu, name, shape):
    a_hat, x, probes, obs, zrow = W.small_graph(name)
    ref = W.ladder_ref(name, shape)
    params = W.small_params(shape)
    base, _, _ = _make(name, x, params, gpu)
    # the probes' fp64 product rows read off the inner baseline's storage (1), or formed again by the gathered product (0: the route
    # that clears the pad columns of Spd itself); each against the oracle, no bit claim between them
    for gather in (1, 0):
        with knobs(gcn3_product_gather=gather):
            _check_delta(_rows(base, probes, obs), ref, zrow, f"{name} {W.shape_id(shape)} gather={gather}")
    _check_logits(base, a_hat, x, params, f"{name} {W.shape_id(shape)}")
    _finish()


REL = [(g, s) for g in W.GRAPHS for s in W.RELATIONS]


@pytest.mark.parametrize("name,shape", REL, ids=[f"{g}-{W.shape_id(s)}" for g, s in REL])
def test_chunks_subsets_pairs_and_refresh(gpu, name, shape):
    a_hat, x, probes, obs, zrow = W.small_graph(name)
    params = W.small_params(shape)
    base, dev, _ = _make(name, x, params, gpu)
    want = _rows(base, probes, obs)
    assert len(probes) > 8
    # one probe per chunk, then a chunk budget of twice one probe's workspace
    need1, need_all = _need(base, 1, len(obs)), _need(base, len(probes), len(obs))
    for budget in (1, 2 * need1):
        with knobs(chunk_budget_bytes=budget):
            need = _need(base, len(probes), len(obs))
            assert need < min(need_all, 4 * need1), (budget, need, need1, need_all)          # chunks of 1 .. 3 probes
            assert np.array_equal(_rows(base, probes, obs), want), budget
    sel, cols = np.array([9, 2, 24, 2, 17]), np.array([30, 1, 1, 12])
    assert np.array_equal(_rows(base, probes, obs), want)                                    # two runs
    assert np.array_equal(_rows(base, probes[sel], obs), want[sel])
    assert np.array_equal(_rows(base, probes, obs[cols]), want[:, cols])
    # the pair list: the rectangle's cells, also at one probe per chunk
    ptr, pobs, col, row = _pairs(name)
    cells = _cells(base, probes, ptr, pobs)
    assert cells.shape == (len(pobs),) and np.array_equal(cells, want[row, col])
    with knobs(chunk_budget_bytes=1):
        assert np.array_equal(_cells(base, probes, ptr, pobs), cells)
    # a workspace that holds 0xFF bytes (NaN as a float) when the call starts: the pad columns of dH1x and dS2x are carried along, and
    # nothing reads a pad column, a pad lane or a table entry that the call itself has not written -- the same bits
    _rows(base, probes, obs)                           # (the handle keeps the workspace of its last call's list lengths)
    (ws,) = base._ws.values()
    ws.fill_(0xFF)
    assert np.array_equal(_rows(base, probes, obs), want) and next(iter(base._ws.values())) is ws
    _cells(base, probes, ptr, pobs)
    (ws,) = base._ws.values()
    ws.fill_(0xFF)
    assert np.array_equal(_cells(base, probes, ptr, pobs), cells) and next(iter(base._ws.values())) is ws
    # a weight update in place + refresh(): other scores, still the oracle's
    with torch.no_grad():
        dev[2].mul_(1.25)
    base.refresh()
    p2 = dict(params)
    p2["W2"] = (p2["W2"] * np.float32(1.25)).astype(np.float32)
    assert np.array_equal(dev[2].cpu().numpy(), p2["W2"])
    ref2 = W.oracle(a_hat, x, p2, probes, obs)
    after = _rows(base, probes, obs)
    _check_delta(after, ref2, zrow, f"{name} {W.shape_id(shape)} after W2 * 1.25")
    assert np.abs(after.astype(np.float64) - want).max() > 1e-3 * ref2.max()
    _finish()


# ---- 2. every storage form of the inner baseline ---------------------------------------------------------------------------------
def _twin(c, gpu, **more):
    """The narrow twin of a storage case under the knobs in force: (route, forms, product rows as stored)."""
    from linkteller_amd import engine
    name = "big" if c["form"].get("big") else "er"
    d = _dev(c["w"], KEYS, gpu)
    with knobs(aggregate_first=0, **more):
        twin = engine.Baseline(_hg(name), torch.from_numpy(np.array(c["x"])).to(gpu), d[0], d[1], d[2][:, :1].contiguous(),
                               d[3][:1].contiguous()).enable_fp64()
        route, arrays = twin.fp64_route(), twin.fp64_arrays()
        arrays["list_entries"] = twin.feature_list_entries()
        torch.cuda.synchronize()
    return route, arrays


def _prove_form(case, c, gpu):
    """Called inside the case's knobs: the narrow twin took the route and holds the forms the case claims."""
    form = c["form"]
    route, arrays = _twin(c, gpu)
    fixed, deferred, cref = arrays["scales"] is not None, arrays["deferred_cref"], arrays["cref"] is not None
    print(f"wide2shape storage {case}: twin route {route} fixed {fixed} deferred_cref {deferred} cref {cref} list entries "
          f"{arrays['list_entries']} knobs {c['knobs']}")
    assert route == form["route"], (case, route)
    assert fixed == form["fixed"] and deferred == form["deferred"] and cref == (form["route"] == 1), (case, fixed, deferred, cref)
    assert arrays["product"].dtype == (torch.int32 if fixed else torch.float64)
    if form["i8"]:
        # the int8 split is what formed the rows: without it the f64 matrix cores round some of the fixed-point words otherwise
        _, plain = _twin(c, gpu, i8_split=0)
        assert plain["scales"] is not None, case
        assert not (torch.equal(plain["product"], arrays["product"]) and torch.equal(plain["scales"], arrays["scales"])), case
    if form.get("tiled"):
        assert _lib.lib().lt_spmm_route(_hg("er").handle, W.round_up4(c["shape"][1])) == 1
    elif not form.get("big"):
        assert _lib.lib().lt_spmm_route(_hg("er").handle, W.round_up4(c["shape"][1])) == 0
    if c["knobs"].get("feature_lists") == 1:
        assert arrays["list_entries"] > 0, case          # (the lists exist: "feature_lists" = 0 is another kernel instance)


_storage_bits = {}


def _storage_run(case, gpu):
    """rows (gather = 1) of a storage case, every check of the case made on the way; once per process"""
    if case in _storage_bits:
        return _storage_bits[case]
    c = W.storage_case(case)
    name = "big" if c["form"].get("big") else "er"
    ref = W.storage_ref(case)
    probes, obs = c["probes"], c["obs"]
    if name == "big":
        rng = np.random.RandomState(78)
        counts = rng.randint(2, 6, len(probes))
        counts[2] = 0
        col = np.concatenate([rng.randint(0, len(obs), k) for k in counts]).astype(np.int64)
        ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        row, pobs = np.repeat(np.arange(len(probes)), counts), obs[col]
    else:
        ptr, pobs, col, row = _pairs("er")
    if case == "g":
        # without "feature_delta" the detector of lt_baseline_enable_fp64 leaves these features to the matrix cores
        assert _twin(c, gpu)[0] == 0
    with knobs(**c["knobs"]):
        _prove_form(case, c, gpu)
        base, _, _ = _make(name, c["x"], c["w"], gpu)
        bits = {}
        for gather in (1, 0):
            with knobs(gcn3_product_gather=gather):
                got = _rows(base, probes, obs)
                _check_delta(got, ref, c["zrow"], f"storage {case} rows gather={gather}")
                cells = _cells(base, probes, ptr, pobs)
                _check_delta(cells, ref[row, col], None, f"storage {case} pairs gather={gather}")
                assert np.array_equal(cells, got[row, col]), (case, gather)
                bits[gather] = got
        with knobs(chunk_budget_bytes=1):
            assert _need(base, len(probes), len(obs)) < 2 * _need(base, 1, len(obs))
            assert np.array_equal(_rows(base, probes, obs), bits[1]), case
            assert np.array_equal(_cells(base, probes, ptr, pobs), bits[1][row, col]), case
        _check_logits(base, c["a_hat"], c["x"], c["w"], f"storage {case}")
    _finish()
    _storage_bits[case] = bits[1]
    return bits[1]


@pytest.mark.parametrize("case", list(W.STORAGE))
def test_every_storage_form_of_the_inner_baseline(gpu, case):
    got = _storage_run(case, gpu)
    same = W.STORAGE[case][5].get("same_as")
    if same is not None:
        # "feature_lists" 1 and 0 (test_feature_lists_gpu.py: the lists keep every bit), the tiled fp64 SpMM
        # (test_tiled_fp64_preactivation_keeps_every_bit): the bits of the case without the knob
        assert np.array_equal(got, _storage_run(same, gpu)), (case, same)
    if case == "k1":
        assert np.array_equal(got, _storage_run("k0", gpu))


@pytest.mark.parametrize("case", W.REFRESH)
def test_refresh_follows_weights_and_features_on_the_stored_forms(gpu, case):
    from linkteller_amd import engine
    c = W.storage_case(case)
    probes, obs = c["probes"], c["obs"]
    with knobs(**c["knobs"]):
        _prove_form(case, c, gpu)
        base, dev, xt = _make("er", c["x"], c["w"], gpu)

        def fresh():
            f = engine.Baseline2W(_hg("er"), xt.clone(), *[t.clone() for t in dev])
            return f.logits(), f.influence_rows(probes, obs, DELTA, "delta")
        before = _rows(base, probes, obs)
        _check_delta(before, W.storage_ref(case), c["zrow"], f"storage {case} before the updates")
        # W1 in place + refresh(): the digits of W1, the scales of the fixed-point rows, cref -- all of them stale
        _, w1 = W.updated(case, "w1")
        with torch.no_grad():
            dev[0][:, ::2] *= 1.25
        assert np.array_equal(dev[0].cpu().numpy(), w1["W1"])
        base.refresh()
        lg, rw = base.logits(), base.influence_rows(probes, obs, DELTA, "delta").clone()
        _check_delta(rw.cpu().numpy(), W.updated_ref(case, "w1"), c["zrow"], f"storage {case} after W1")
        assert not np.array_equal(rw.cpu().numpy(), before)
        f_lg, f_rw = fresh()
        assert torch.equal(lg, f_lg) and torch.equal(rw, f_rw)
        # a feature row edited in place through torch + refresh(): the engine announces it (lt_baseline2w_features_changed: the
        # feature route keeps lists of X built once) and the handle follows
        x2, _ = W.updated(case, "x")
        r_, c_ = np.nonzero(x2 != c["x"])
        with torch.no_grad():
            for i, j in zip(r_, c_):
                xt[int(i), int(j)] = float(x2[i, j])
        assert np.array_equal(xt.cpu().numpy(), x2)
        base.refresh()
        lg2, rw2 = base.logits(), base.influence_rows(probes, obs, DELTA, "delta").clone()
        _check_delta(rw2.cpu().numpy(), W.updated_ref(case, "x"), c["zrow"], f"storage {case} after X")
        f_lg, f_rw = fresh()
        assert torch.equal(lg2, f_lg) and torch.equal(rw2, f_rw) and not torch.equal(rw2, rw)
        # the same kind of edit behind torch's back (a raw copy): announced with features_changed()
        row, j = int(r_[0]), int(c_[0])
        word = torch.tensor([float(c["x"][row, j])], dtype=torch.float32)
        torch.cuda.synchronize()
        assert _hip().hipMemcpy(C.c_void_p(xt.data_ptr() + 4 * (row * xt.shape[1] + j)), C.c_void_p(word.data_ptr()), C.c_size_t(4), 1) == 0
        version = xt._version
        assert base.features_changed() is base and xt._version == version
        lg3, rw3 = base.logits(), base.influence_rows(probes, obs, DELTA, "delta").clone()
        f_lg, f_rw = fresh()
        assert torch.equal(lg3, f_lg) and torch.equal(rw3, f_rw) and not torch.equal(rw3, rw2)
    _finish()


# ---- 3. bitmap words, chunk sizes, item counts -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", W.BIG, ids=W.shape_id)
def test_bitmaps_of_516_words(gpu, shape):
    a_hat, x, probes, obs, zrow = W.big_graph2()
    assert (a_hat.shape[0] + 31) // 32 == 516
    ref = W.big_ref(shape)
    base, _, _ = _make("big", x, W.small_params(shape), gpu)
    want = None
    for gather in (1, 0):
        with knobs(gcn3_product_gather=gather):
            got = _rows(base, probes, obs)
            _check_delta(got, ref, zrow, f"big {W.shape_id(shape)} gather={gather}")
            want = got if want is None else want
    with knobs(chunk_budget_bytes=1):
        assert _need(base, len(probes), len(obs)) < 2 * _need(base, 1, len(obs))
        assert np.array_equal(_rows(base, probes, obs), want)
    _finish()


@pytest.mark.parametrize("shape", W.ALL_PROBES, ids=W.shape_id)
def test_three_hundred_probes_in_one_chunk(gpu, shape):
    a_hat, x, _, obs, _ = W.small_graph("er")
    n = a_hat.shape[0]
    probes = np.arange(n, dtype=np.int32)
    base, _, _ = _make("er", x, W.small_params(shape), gpu)
    # the workspace grows with every probe of a chunk, so the bytes of a chunk of 300 are reached only by a chunk of 300: the default
    # budget cuts nothing, a budget of 2^50 bytes could not take more
    need = {k: _need(base, k, len(obs)) for k in (256, 299, 300)}
    with knobs(chunk_budget_bytes=1 << 50):
        assert _need(base, 300, len(obs)) == need[300]
    # (beyond a cut only the checked copy of the node list would grow: 4 bytes a probe)
    assert need[256] < need[299] < need[300] and need[300] - need[299] > 512 and need[300] - need[256] > 44 * 512
    got = _rows(base, probes, obs)
    zero = int(np.flatnonzero(~x.any(axis=1))[0])
    _check_delta(got, W.all_probes_ref(shape), zero, f"er {W.shape_id(shape)} 300 probes")
    with knobs(chunk_budget_bytes=1):
        assert _need(base, 300, len(obs)) < need[256]
        assert np.array_equal(_rows(base, probes, obs), got)
    _finish()


def test_the_cap_of_65534_probes_per_chunk(gpu):
    """65537 probes (the 28 of the graph `loops`, tiled) against three observed nodes under a chunk budget of 2^40 bytes: the chunk
    is cut at 65534 probes by the cap alone, three probes follow in a chunk of their own."""
    a_hat, x, _, _, _ = W.small_graph("loops")
    probes, tiled, obs = W.cap_lists()
    base, _, _ = _make("loops", x, W.small_params(W.CAP_SHAPE), gpu)
    small = _rows(base, probes, obs)
    _check_delta(small, W.cap_ref(), W.small_graph("loops")[4], f"loops {W.shape_id(W.CAP_SHAPE)} 28 probes")
    with knobs(chunk_budget_bytes=1 << 40):
        need = {k: _need(base, k, len(obs)) for k in (W.CAP - 1, W.CAP, W.CAP_PROBES)}
        # beyond the cap only the checked copy of the node list grows: a chunk of 65537 would add three probes' tables
        assert 0 <= need[W.CAP_PROBES] - need[W.CAP] <= 512 < need[W.CAP] - need[W.CAP - 1], need
        print(f"wide2shape cap: workspace {need[W.CAP_PROBES] / 1e6:.1f} MB")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = _rows(base, tiled, obs)
        t1 = time.perf_counter()
        idx = np.arange(W.CAP_PROBES) % len(probes)
        assert np.array_equal(got, small[idx])
        # the pair list over the same probes, one pair each
        ptr = np.arange(W.CAP_PROBES + 1, dtype=np.int64)
        which = np.arange(W.CAP_PROBES) % len(obs)
        cells = _cells(base, tiled, ptr, obs[which])
        t2 = time.perf_counter()
        assert np.array_equal(cells, small[idx, which])
        print(f"wide2shape cap: rows call {t1 - t0:.3f} s, pairs call {t2 - t1:.3f} s (with their copies to the host)")
    _finish()


def test_item_counts_at_the_tile_edges_of_the_item_product(gpu):
    """One probe per chunk: lt_launch_gemm_mdev sees 1, 63, 64, 65, 128, 129 and 513 rows on the device; two per chunk and all in
    one: other counts -- the same bits every time."""
    a_hat, x, _, _, _ = W.small_graph("hub")
    probes, obs = W.hub_lists()
    base, _, _ = _make("hub", x, W.small_params(W.HUB_SHAPE), gpu)
    need1, need_all = _need(base, 1, len(obs)), _need(base, len(probes), len(obs))
    assert need_all > 6 * need1                       # the default budget takes the seven probes in one chunk
    want = _rows(base, probes, obs)
    _check_delta(want, W.hub_ref(), None, f"hub {W.shape_id(W.HUB_SHAPE)} item counts")
    for budget, most in ((1, 2), (2 * need1, 4)):
        with knobs(chunk_budget_bytes=budget):
            assert _need(base, len(probes), len(obs)) < most * need1
            assert np.array_equal(_rows(base, probes, obs), want), budget
    with knobs(gcn3_product_gather=0):
        _check_delta(_rows(base, probes, obs), W.hub_ref(), None, f"hub {W.shape_id(W.HUB_SHAPE)} item counts gather=0")
    _finish()


# ---- 4. strides through the C ABI ------------------------------------------------------------------------------------------------
class _Raw2W:
    """lt_baseline2w_* / lt_influence2w_* on abi_views.View operands (what engine.Baseline2W does with contiguous tensors)."""

    def __init__(self, hg, x, f, w1, b1, h, w2, b2, c):
        from linkteller_amd import engine
        assert w1.ld == h and w2.ld == c                # (the ABI gives the weights no leading dimension)
        self.n, self.c, self.dev, self.keep = hg.n, c, x.buf.device, (hg, x, w1, b1, w2, b2)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().lt_baseline2w_create(hg.handle, x.assert_aligned(), x.ld, f, w1.assert_aligned(), b1.assert_aligned(), h,
                                                   w2.assert_aligned(), b2.assert_aligned(), c, engine._stream(), C.byref(self._h)),
                   "lt_baseline2w_create")

    def destroy(self):
        torch.cuda.synchronize()
        _lib.lib().lt_baseline2w_destroy(self._h)

    def logits(self):
        from linkteller_amd import engine
        out = torch.empty((self.n, self.c), dtype=torch.float32, device=self.dev)
        _lib.check(_lib.lib().lt_baseline2w_logits(self._h, out.data_ptr(), engine._stream()), "lt_baseline2w_logits")
        return out.cpu().numpy()

    def rows(self, probes, obs):
        from linkteller_amd import engine
        lib = _lib.lib()
        p, o = torch.from_numpy(np.array(probes)).to(self.dev), torch.from_numpy(np.array(obs)).to(self.dev)
        out = torch.full((p.numel(), o.numel()), float("nan"), dtype=torch.float32, device=self.dev)
        ws = engine._workspace(lib.lt_influence2w_workspace_bytes(self._h, p.numel(), o.numel()), self.dev)
        _lib.check(lib.lt_influence2w_rows(self._h, p.data_ptr(), p.numel(), o.data_ptr(), o.numel(), DELTA, _lib.MODE_DELTA,
                                           out.data_ptr(), o.numel(), ws.data_ptr(), ws.numel(), engine._stream()), "lt_influence2w_rows")
        return out.cpu().numpy()

    def pairs(self, probes, ptr, pobs):
        from linkteller_amd import engine
        lib = _lib.lib()
        p, o = torch.from_numpy(np.array(probes)).to(self.dev), torch.from_numpy(np.array(pobs)).to(self.dev)
        ptr = np.ascontiguousarray(ptr, dtype=np.int64)
        out = torch.full((o.numel(),), float("nan"), dtype=torch.float32, device=self.dev)
        ws = engine._workspace(lib.lt_influence2w_pairs_workspace_bytes(self._h, p.numel(), o.numel()), self.dev)
        _lib.check(lib.lt_influence2w_pairs(self._h, p.data_ptr(), p.numel(), ptr.ctypes.data, o.data_ptr(), o.numel(), DELTA,
                                            _lib.MODE_DELTA, out.data_ptr(), ws.data_ptr(), ws.numel(), engine._stream()),
                   "lt_influence2w_pairs")
        return out.cpu().numpy()


# (ldx, element offset of X, element offset of every weight): F = 29, so ldx = 32 keeps rows 16-byte aligned behind an aligned base
# and ldx = 33 puts them off 16 bytes whatever the base; offset 1: 4-byte aligned only.  The header states no alignment for these
# operands beyond that of a float, and test_abi_layout_gpu.py hands lt_baseline_create the same layouts.
LAYOUTS = ((32, 0, 0), (32, 1, 1), (33, 0, 1), (33, 1, 0))


@pytest.mark.parametrize("shape", W.ER29, ids=W.shape_id)
def test_strided_operands_give_the_bits_of_contiguous_ones(gpu, shape):
    a_hat, x, probes, obs, zrow = S.small_graph("er29")
    f, (h, c) = x.shape[1], shape
    assert f == 29 and LAYOUTS[2][0] == f + 4 and LAYOUTS[0][0] == f + 3
    params = W.er29_params(shape)
    ptr, _, col, row = _pairs("er")                    # (the offsets and columns of that list, over this graph's observed nodes)
    assert len(ptr) == len(probes) + 1 and col.max() < len(obs)
    pobs = obs[col]
    control, _, _ = _make("er29", x, params, gpu)
    want = {}
    for gather in (1, 0):
        with knobs(gcn3_product_gather=gather):
            want[gather] = (_rows(control, probes, obs), _cells(control, probes, ptr, pobs))
            assert np.array_equal(want[gather][1], want[gather][0][row, col])
    assert want[1][0].max() > 0 and np.all(want[1][0][zrow] == 0)
    want_logits = control.logits().cpu().numpy()
    for ldx, x_off, w_off in LAYOUTS:
        xv = V.View(x, ldx, x_off)
        ws = [V.View(params[k], off=w_off) for k in KEYS]
        raw = _Raw2W(_hg("er29"), xv, f, ws[0], ws[1], h, ws[2], ws[3], c)
        for gather in (1, 0):
            with knobs(gcn3_product_gather=gather):
                assert np.array_equal(raw.rows(probes, obs), want[gather][0]), (ldx, x_off, w_off, gather)
                assert np.array_equal(raw.pairs(probes, ptr, pobs), want[gather][1]), (ldx, x_off, w_off, gather)
        assert np.array_equal(raw.logits(), want_logits), (ldx, x_off, w_off)
        raw.destroy()
        for v in [xv] + ws:
            assert v.pads_untouched(), v.touched_pads()[:8]
    _finish()


# ---- 5. the same storage forms behind the 3-layer handles ------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.REFRESH)
@pytest.mark.parametrize("kind", list(W.BEHIND3))
def test_storage_forms_behind_three_layers(gpu, case, kind):
    from linkteller_amd import engine
    c = W.storage_case(case)
    probes, obs = c["probes"], c["obs"]
    params = W.behind3_params(case, kind)
    ref = W.behind3_ref(case, kind)
    with knobs(**c["knobs"]):
        _prove_form(case, c, gpu)
        make = _wide3 if kind == "wide" else engine.Baseline3
        base = make(_hg("er"), torch.from_numpy(np.array(c["x"])).to(gpu), *_dev(params, W.KEYS3, gpu))
        assert base.wide == (kind == "wide") and (base.h1, base.h2, base.c) == (64,) + W.BEHIND3[kind]
        for gather in (1, 0):
            with knobs(gcn3_product_gather=gather):
                out = torch.full((len(probes), len(obs)), float("nan"), dtype=torch.float32, device=gpu)
                got = base.influence_rows(probes, obs, DELTA, "delta", out=out).cpu().numpy()
                assert np.isfinite(got).all()
                _check_delta(got, ref, c["zrow"], f"storage {case} behind three layers ({kind}) gather={gather}")
    _finish()

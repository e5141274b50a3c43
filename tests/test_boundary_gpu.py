"""Every graph kernel at its row, column and list length boundaries: the ladder graphs of boundary_cases.py (rows, columns and
member lists of exactly K - 1, K and K + 1 entries for every length a kernel cuts at) through every entry point and every route
knob.  test_boundary_cpu.py shows that a dropped or doubled entry at a cut moves the fp64 references used here by at least 100 x
the tolerances applied here.  No tolerance of its own: each is the one tests/test_gpu_parity.py (or the training tests) uses for
the same quantity."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import boundary_cases as B
from conftest import noise_gate

pytestmark = pytest.mark.gpu

SHAPES = pytest.mark.parametrize("h,c", B.MODEL_SHAPES)


@contextlib.contextmanager
def knobs(**kw):
    from linkteller_amd import _lib
    try:
        for k, v in kw.items():
            _lib.set_tuning(k, v)
        yield
    finally:
        for k in kw:
            _lib.set_tuning(k, None)


@functools.lru_cache(maxsize=None)
def _hg(name):
    from linkteller_amd import graph
    return graph.HipGraph(B.graph_of(name).a)


@functools.lru_cache(maxsize=None)
def _dev_inputs(name, h, c):
    w = B.weights(h, c)
    return torch.from_numpy(B.features(name)).cuda(), [torch.from_numpy(w[k]).cuda() for k in ("W1", "b1", "W2", "b2")]


def _baseline(name, h, c):
    from linkteller_amd import engine
    x, w = _dev_inputs(name, h, c)
    return engine.Baseline(_hg(name), x, *w)


def _launches(fn, classes):
    """{class: launches} of the named kernel classes while fn runs (lt_profile_enable / lt_profile_summary)."""
    from linkteller_amd import _lib
    lib = _lib.lib()
    lib.lt_profile_reset()
    lib.lt_profile_enable(sum(1 << _lib.KERNEL_IDS[k] for k in classes))
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        for k in classes:
            tot, cnt = C.c_double(), C.c_int64()
            _lib.check(lib.lt_profile_summary(_lib.KERNEL_IDS[k], C.byref(tot), C.byref(cnt)), "lt_profile_summary")
            out[k] = cnt.value
    finally:
        lib.lt_profile_enable(0)
        lib.lt_profile_reset()
    return out


_rows_cache = {}


def _sentinel(rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=torch.float32, device="cuda")


def _rows(name, h, c, mode, want_route=None, **kn):
    """One fresh baseline under the knobs, one lt_influence_rows call over node_lists(name); float64 [n_probe, n_obs].  Cached per
    knob set.  ``want_route``: the value lt_baseline_fp64_route must report (DELTA)."""
    key = (name, h, c, mode, tuple(sorted(kn.items())))
    if key not in _rows_cache:
        probes, obs = B.node_lists(name)
        with knobs(**kn):
            base = _baseline(name, h, c)
            if mode == "delta":
                base.enable_fp64()
                if want_route is not None:
                    assert base.fp64_route() in want_route, (base.fp64_route(), want_route)
            got = base.influence_rows(probes, obs, B.DELTA, mode, out=_sentinel(len(probes), len(obs))).cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()          # (a cell nobody wrote keeps its NaN)
        _rows_cache[key] = got
    return _rows_cache[key]


# ---- lt_spmm_csr_f32 --------------------------------------------------------------------------------------------------------
def _spmm(name, ncols, epilogue, **kn):
    """lt_spmm_csr_f32 into a NaN-filled result (a row no kernel writes keeps its NaN); (result, lt_spmm_route)."""
    from linkteller_amd import _lib, engine
    s, b, _ = B.spmm_inputs(name, ncols)
    hg = _hg(name)
    ds, db = torch.from_numpy(s).cuda(), torch.from_numpy(b).cuda()
    out = _sentinel(hg.n, ncols)
    with knobs(**kn):
        route = _lib.lib().lt_spmm_route(hg.handle, ncols)
        _lib.check(_lib.lib().lt_spmm_csr_f32(hg.handle, ds.data_ptr(), ncols, ncols, db.data_ptr() if epilogue else None, int(epilogue),
                                              out.data_ptr(), ncols, engine._stream()), "lt_spmm_csr_f32")
        torch.cuda.synchronize()
    return out.cpu().numpy(), route


@pytest.mark.parametrize("epilogue", [True, False], ids=["bias_relu", "plain"])
@pytest.mark.parametrize("ncols", B.SPMM_COLS)
@pytest.mark.parametrize("name", ["hub", "short"])
def test_spmm_on_the_ladders(gpu, name, ncols, epilogue):
    """Rows of 0 .. 2049 entries (classes of 16 in the tiled route, segments of 128, three segments, 1024 + 1): the row route, the
    tiled route and the tiled route with 64-bit gather offsets give the same bits, within 1e-5 max(1, |want|) of the fp64 product,
    and on the ladder rows the bits of the documented canonical order."""
    g = B.graph_of(name)
    want = B.spmm_want(name, ncols, epilogue)
    rows, r_rows = _spmm(name, ncols, epilogue)
    tiled, r_tiled = _spmm(name, ncols, epilogue, tiled_min_bytes=0)
    big, r_big = _spmm(name, ncols, epilogue, tiled_min_bytes=0, tiled_big=1)
    assert (r_rows, r_tiled, r_big) == (0, 1, 1)
    assert np.isfinite(rows).all() and np.isfinite(tiled).all() and np.isfinite(big).all()
    err = np.abs(rows - want).max()
    print(f"{name} ncols {ncols}: |got - fp64| = {err:.3e}, bound {1e-5 * max(1.0, np.abs(want).max()):.3e}")
    assert err <= 1e-5 * max(1.0, np.abs(want).max())
    assert np.array_equal(rows, tiled) and np.array_equal(rows, big)
    ladder = sorted(g.u.values())
    canon = B.canonical_spmm_rows(name, ncols, epilogue, ladder)
    for d, u in B.ladder_rows(g):
        assert np.array_equal(rows[u], canon[u]), (d, int((rows[u] != canon[u]).sum()))
    empty = np.flatnonzero(np.diff(g.a.indptr) == 0)
    assert np.array_equal(rows[empty], np.broadcast_to(want[empty[0]].astype(np.float32), (len(empty), ncols)))


# ---- lt_gcn2_forward / lt_baseline_logits -------------------------------------------------------------------------------------
@SHAPES
@pytest.mark.parametrize("name", ["hub", "short"])
def test_forward_logits_on_the_ladders(gpu, name, h, c):
    from linkteller_amd import engine
    x, w = _dev_inputs(name, h, c)
    ref = B.oracle_logits(name, h, c)
    tol = 2e-5 * np.abs(ref).max() + 1e-6
    out = engine.gcn2_forward(_hg(name), x, *w).cpu().numpy()
    print(f"{name} H {h} C {c}: |logits - fp64| = {np.abs(out - ref).max():.3e}, bound {tol:.3e}")
    assert np.abs(out - ref).max() <= tol
    assert np.array_equal(_baseline(name, h, c).logits().cpu().numpy(), out)
    with knobs(tiled_min_bytes=0):
        assert np.array_equal(engine.gcn2_forward(_hg(name), x, *w).cpu().numpy(), out)


# ---- lt_influence_rows ----------------------------------------------------------------------------------------------------------
def _check_zeros(got, ref64):
    assert np.all(got[ref64 == 0] == 0)


@SHAPES
def test_influence_modes_on_hub_ladder(gpu, h, c):
    """DELTA within 1e-5 of the largest score of the fp64 oracle; FULL == SPARSE bit for bit; FULL against fp64 in units of the
    oracle's own fp32 error (noise_gate: ceiling 2, recorded); exact zeros where the oracle has exact zeros; the two copies of
    u_1025 in the observed list give the same column."""
    ref64 = B.oracle_matrix("hub", h, c, "float64")
    e32 = np.abs(B.oracle_matrix("hub", h, c, "float32") - ref64).max()
    scale = ref64.max()
    probes, obs = B.node_lists("hub")
    delta = _rows("hub", h, c, "delta")
    lib_classes = ("full_stageA", "full_stageB", "item_stageA", "item_stageB")
    res = {}
    base = _baseline("hub", h, c)
    for m in ("full", "sparse"):
        n_l = _launches(lambda: res.__setitem__(m, base.influence_rows(probes, obs, B.DELTA, m, out=_sentinel(len(probes), len(obs))).cpu().numpy().astype(np.float64)), lib_classes)
        if m == "full":
            assert n_l["full_stageA"] > 0 and n_l["full_stageB"] > 0 and n_l["item_stageA"] == 0, n_l
        else:
            assert n_l["item_stageA"] > 0 and n_l["item_stageB"] > 0 and n_l["full_stageA"] == 0, n_l
    _rows_cache[("hub", h, c, "full", ())] = res["full"]
    _rows_cache[("hub", h, c, "sparse", ())] = res["sparse"]
    e_delta, e_full = np.abs(delta - ref64).max(), np.abs(res["full"] - ref64).max()
    print(f"hub_ladder H {h} C {c}: max score {scale:.3f}; |ref32 - ref64| = {e32:.3e}; |delta - ref64| = {e_delta:.3e} "
          f"({e_delta / scale:.2e} of max); |full - ref64| = {e_full:.3e} (ratio {e_full / e32:.3f})")
    assert np.array_equal(res["full"], res["sparse"])
    assert e_delta <= 1e-5 * scale
    noise_gate(f"boundary.hub_ladder.h{h}c{c}.full", e_full / max(e32, 1e-4 * scale))
    # the member-ladder cells (w_m, u_1025) are an influence matrix of their own: 1e-5 of THEIR largest score
    # (test_boundary_cpu.test_mutation_margin_of_the_member_ladder: a lost member moves its cell by >= 100 x that)
    m_rows, m_col = B.member_cells()
    sub = ref64[m_rows, m_col]
    print(f"  member ladder: largest score {sub.max():.3e}, |delta - ref64| = {np.abs(delta[m_rows, m_col] - sub).max():.3e}")
    assert np.abs(delta[m_rows, m_col] - sub).max() <= 1e-5 * sub.max()
    for got in (delta, res["full"]):
        _check_zeros(got, ref64)
        dup = np.flatnonzero(obs == B.hub_ladder().u[B.HUB])
        assert len(dup) == 2 and np.array_equal(got[:, dup[0]], got[:, dup[1]])


FULL_KNOBS = [dict(full_p=p, long_par=lp) for p in (8, 16, 32) for lp in (0, 1)]
ITEM_KNOBS = [dict(stageb_rows=0), dict(pair_marks=0, pair_list=0), dict(pair_marks=0, pair_list=1),
              dict(bits_max_bytes=0, hub_short_side=0), dict(bits_max_bytes=0, hub_short_side=1), dict(item_bits=0),
              # (without a bitmap row per probe a call joins over the middle nodes unless "pair_marks" is negative: the per-pair
              #  kernel with the big probes' bitmap slots -- a column of 512 against 513 entries decides a slot -- and with none)
              dict(bits_max_bytes=0, pair_marks=-1, hub_short_side=0), dict(bits_max_bytes=0, pair_marks=-1, hub_short_side=1),
              dict(item_bits=0, pair_marks=-1),
              # (observed hubs with a bitmap row per probe: members from the short side -- the light probes' member lists)
              dict(hub_short_side=1), dict(hub_short_side=1, stageb_rows=0)]
S1D = dict(aggregate_first=0)


def _ids(kn):
    return "-".join(f"{k}{v}" for k, v in kn.items())


@SHAPES
def test_full_knobs_on_hub_ladder(gpu, h, c):
    want = _rows("hub", h, c, "sparse")
    for kn in FULL_KNOBS:
        assert np.array_equal(_rows("hub", h, c, "full", **kn), want), kn


@SHAPES
def test_sparse_knobs_on_hub_ladder(gpu, h, c):
    want = _rows("hub", h, c, "sparse")
    for kn in ITEM_KNOBS:
        assert np.array_equal(_rows("hub", h, c, "sparse", **kn), want), kn


@SHAPES
def test_delta_knobs_on_hub_ladder(gpu, h, c):
    """Aggregate-first (the default at this size: route 2) and the S1d route ("aggregate_first" = 0) differ in fp64 summation
    order only: within 1e-6 of the largest score of each other, each within 1e-5 of the oracle.  On either, every stage-B knob
    gives the bits of that route's default; on the S1d route so do "z_on_demand" 0 / 1 and the tiled fp64 SpMM."""
    ref64 = B.oracle_matrix("hub", h, c, "float64")
    scale = ref64.max()
    agg = _rows("hub", h, c, "delta", (2,), aggregate_first=1)
    assert np.array_equal(agg, _rows("hub", h, c, "delta"))
    s1d = _rows("hub", h, c, "delta", (0, 1), **S1D)
    print(f"H {h} C {c}: |aggregate-first - S1d route| / max = {np.abs(agg - s1d).max() / scale:.2e}")
    assert np.abs(agg - s1d).max() <= 1e-6 * scale
    for got in (agg, s1d):
        assert np.abs(got - ref64).max() <= 1e-5 * scale
        _check_zeros(got, ref64)
    for kn in ITEM_KNOBS:
        assert np.array_equal(_rows("hub", h, c, "delta", (2,), aggregate_first=1, **kn), agg), kn
        assert np.array_equal(_rows("hub", h, c, "delta", (0, 1), **S1D, **kn), s1d), kn
    for z in (0, 1):
        assert np.array_equal(_rows("hub", h, c, "delta", (0, 1), z_on_demand=z, **S1D), s1d), z
    # the tiled fp64 SpMM takes fp64 product rows ("s1_f32" = 0: another storage form, < 1e-6) formed on all rows
    plain = _rows("hub", h, c, "delta", (0, 1), s1_f32=0, z_on_demand=0, **S1D)
    tiled = _rows("hub", h, c, "delta", (0, 1), s1_f32=0, z_on_demand=0, tiled_min_bytes=0, **S1D)
    assert np.array_equal(tiled, plain)
    assert np.abs(plain - s1d).max() <= 1e-6 * scale


@SHAPES
def test_short_ladder_fused_route_and_host_landing(gpu, h, c):
    """short_ladder keeps its incidence records (rows of exactly 128 entries, a column of 513, a node at 4050 of 4096 incidences):
    the fused DELTA route against the item kernels, lt_influence_rows_f64, and the packed host landing against rows + export."""
    from linkteller_amd import engine
    ref64 = B.oracle_matrix("short", h, c, "float64")
    e32 = np.abs(B.oracle_matrix("short", h, c, "float32") - ref64).max()
    scale = ref64.max()
    probes, obs = B.node_lists("short")
    full, sparse = _rows("short", h, c, "full"), _rows("short", h, c, "sparse")
    assert np.array_equal(full, sparse)
    noise_gate(f"boundary.short_ladder.h{h}c{c}.full", np.abs(full - ref64).max() / max(e32, 1e-4 * scale))
    _check_zeros(full, ref64)
    for kn in ITEM_KNOBS:
        assert np.array_equal(_rows("short", h, c, "sparse", **kn), sparse), kn
    got = {}
    with knobs(**S1D):
        base = _baseline("short", h, c).enable_fp64()
        assert base.fp64_route() in (0, 1)
        for fused in (1, 0):
            with knobs(delta_fused=fused):
                base.refresh()
                n_l = _launches(lambda: got.__setitem__(fused, base.influence_rows(probes, obs, B.DELTA, "delta").cpu().numpy()), ("item_stageA",))
            assert (n_l["item_stageA"] == 0) == (fused == 1), (fused, n_l)
        assert np.array_equal(got[1], got[0])
        g64 = got[1].astype(np.float64)
        print(f"short_ladder H {h} C {c}: |delta - ref64| / max = {np.abs(g64 - ref64).max() / scale:.2e}")
        assert np.abs(g64 - ref64).max() <= 1e-5 * scale
        _check_zeros(g64, ref64)
        for kn in ITEM_KNOBS:
            with knobs(delta_fused=0, **kn):
                base.refresh()
                assert np.array_equal(base.influence_rows(probes, obs, B.DELTA, "delta").cpu().numpy(), got[1]), kn
        # rows + export against lt_influence_rows_f64 and the packed lt_influence_matrix_host
        base.refresh()
        want64 = engine.export_rows_f64(base.influence_rows(probes, obs, B.DELTA, "delta"))
        assert np.array_equal(want64, got[1].astype(np.float64))
        base.refresh()
        host = torch.full((len(probes), len(obs)), 7.0, dtype=torch.float64).pin_memory()
        out = base.influence_rows(probes, obs, B.DELTA, "delta", host=host)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), got[1]) and np.array_equal(host.numpy(), want64)
        with knobs(export_compact=2):
            for refresh in (True, False):
                before = base.host_landing_stats()
                mat = base.influence_matrix_host(probes, obs, B.DELTA, "delta", refresh=refresh)
                after = base.host_landing_stats()
                assert np.array_equal(mat, want64), refresh
                assert after["early"] + after["late"] == before["early"] + before["late"] + 1, "the call was not packed"
                assert after["mismatch"] == 0


# ---- the second pass of k_item_stageB_rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sparse", "delta"])
def test_second_pass_of_the_stage_b_rows_kernel(gpu, mode):
    """2049 probes x 2048 observed nodes with "pair_marks" = -1: no probe split (n_obs >= 2048), so a block of k_item_stageB_rows
    has 2049 probes: SPARSE lists its touched pairs in two passes, 2048 probes and then one (DELTA has no list: one loop).  The bits of the per-pair kernel ("stageb_rows" = 0) on the
    whole matrix, and of the default-knob call on the ladder cells."""
    h, c = B.MODEL_SHAPES[0]
    probes, obs = B.node_lists("hub")
    rng = np.random.RandomState(41)
    big_p = np.concatenate([probes, rng.randint(0, B.N_POOL, B.LT_SB_PASS + 1 - len(probes))]).astype(np.int32)
    big_o = np.concatenate([obs, rng.randint(0, B.N_POOL, B.LT_SB_PASS - len(obs))]).astype(np.int32)
    assert len(big_p) == B.LT_SB_PASS + 1 and len(big_o) == B.LT_SB_PASS
    # the last probe -- the one the second pass serves -- is a probe with a long column: its row of the result is not all zeros
    big_p[-1], big_p[len(probes)] = probes[np.flatnonzero(probes == B.hub_ladder().v[2049])[0]], big_p[-1]
    got = {}
    for rows_route in (1, 0):
        with knobs(pair_marks=-1, stageb_rows=rows_route):
            base = _baseline("hub", h, c)
            got[rows_route] = base.influence_rows(big_p, big_o, B.DELTA, mode, out=_sentinel(len(big_p), len(big_o))).cpu().numpy()
    assert np.isfinite(got[1]).all() and np.array_equal(got[1], got[0])
    short_rows = np.diff(B.hub_ladder().a.indptr)[big_o] <= B.LT_ROW_SEG          # (the hubs are stageB_long_block's)
    assert got[1][-1, short_rows].max() > 0
    want = _rows("hub", h, c, mode).astype(np.float32)
    assert np.array_equal(got[1][: len(probes), : len(obs)], want)
    assert np.array_equal(got[1][-1, : len(obs)], want[np.flatnonzero(probes == big_p[-1])[0]])


# ---- the bitmap slots of the big probes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sparse", "delta"])
def test_big_probe_slots_run_out(gpu, mode):
    """Without a bitmap row per probe ("bits_max_bytes" = 0) the probes whose column has more than LT_BIG_RV entries take one of
    LT_BIG_SLOTS = 64 bitmap slots each, in the order their blocks arrive; the others are searched.  63, 64 and 65 big probes in
    one call (the 17 of the ladder repeated): whoever is left without a slot, every row carries the default call's bits."""
    h, c = B.MODEL_SHAPES[0]
    probes, obs = B.node_lists("hub")
    col_len = np.bincount(B.hub_ladder().a.indices, minlength=B.hub_ladder().n)
    big = probes[col_len[probes] > B.LT_BIG_RV]
    small = probes[col_len[probes] <= B.LT_BIG_RV][:8]
    assert 0 < len(big) < B.LT_BIG_SLOTS
    want = _rows("hub", h, c, mode).astype(np.float32)
    where = {int(v): i for i, v in enumerate(probes)}
    for n_big in (B.LT_BIG_SLOTS - 1, B.LT_BIG_SLOTS, B.LT_BIG_SLOTS + 1):
        lst = np.concatenate([small[:4], np.resize(big, n_big), small[4:]]).astype(np.int32)
        for short_side in (0, 1):
            with knobs(bits_max_bytes=0, pair_marks=-1, hub_short_side=short_side):
                base = _baseline("hub", h, c)
                got = base.influence_rows(lst, obs, B.DELTA, mode, out=_sentinel(len(lst), len(obs))).cpu().numpy()
            assert np.array_equal(got, want[[where[int(v)] for v in lst]]), (n_big, short_side)


# ---- lt_influence_pairs -----------------------------------------------------------------------------------------------------------
@SHAPES
def test_pair_list_of_every_ladder_pair(gpu, h, c):
    probes, obs = B.node_lists("hub")
    ptr = (np.arange(len(probes) + 1) * len(obs)).astype(np.int64)
    pair_obs = np.tile(obs, len(probes)).astype(np.int32)
    for mode in ("sparse", "delta"):
        base = _baseline("hub", h, c)
        got = base.influence_pairs(probes, ptr, pair_obs, B.DELTA, mode).cpu().numpy().astype(np.float64)
        assert np.array_equal(got.reshape(len(probes), len(obs)), _rows("hub", h, c, mode)), mode


# ---- lt_influence3_rows_mode ------------------------------------------------------------------------------------------------------
def test_gcn3_modes_on_hub_ladder(gpu):
    """(H1, H2, C) = (32, 16, 2): SPARSE in the reference's fp32 noise class (the gate of test_gcn3_probe_primitive_against_oracle),
    DELTA within 1e-5 of the largest fp64 score (test_gcn3_delta_mode_against_the_fp64_oracle), exact zeros in both."""
    from linkteller_amd import engine
    ref64 = B.oracle_matrix3("float64")
    e32 = np.abs(B.oracle_matrix3("float32") - ref64).max()
    scale = ref64.max()
    probes, obs = B.node_lists("hub")
    P = B.params3()
    x = torch.from_numpy(B.features("hub")).cuda()
    base = engine.Baseline3(_hg("hub"), x, *[torch.from_numpy(P[k]).cuda() for k in ("W1", "b1", "W2", "b2", "W3", "b3")])
    sparse = base.influence_rows(probes, obs, B.DELTA, "sparse").cpu().numpy().astype(np.float64)
    delta = base.influence_rows(probes, obs, B.DELTA, "delta").cpu().numpy().astype(np.float64)
    print(f"gcn3 hub_ladder: max {scale:.3g} |ref32 - ref64| {e32:.2e} |sparse - ref64| {np.abs(sparse - ref64).max():.2e} "
          f"|delta - ref64| / max {np.abs(delta - ref64).max() / scale:.2e}")
    noise_gate("boundary.hub_ladder.gcn3.sparse", np.abs(sparse - ref64).max() / max(e32, 1e-4 * scale))
    assert np.abs(delta - ref64).max() <= 1e-5 * scale
    _check_zeros(sparse, ref64)
    _check_zeros(delta, ref64)
    from oracle import linkteller_oracle as O
    ref_logits = O.gcn3_forward(torch.from_numpy(B.features("hub")).double(), O.to_torch_sparse(B.hub_ladder().a).double(),
                                {k: torch.from_numpy(v).double() for k, v in P.items()}).numpy()
    assert np.abs(base.logits().cpu().numpy() - ref_logits).max() <= 2e-5 * max(1.0, np.abs(ref_logits).max())


# ---- the trainers: the backward walks the columns ---------------------------------------------------------------------------------
def test_gcn2_trainer_epoch_on_hub_ladder(gpu):
    """One epoch, dropout 0, against train_restate.epoch_reference in fp64 with the gates of test_train_backward_gpu.py."""
    import test_train_backward_gpu as TB
    case = B.train_case2()
    params = [TB._dev(p.copy()) for p in case["params"]]
    tr = TB._trainer(case, params)
    start = TB._host(params)
    loss, correct = tr.run(1)
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(TB.K.NAMES, tr.grads())}
    got["Z2"] = tr.logits().cpu().numpy().astype(np.float64)
    got["loss"], got["correct"] = float(loss[0]), int(correct[0])
    TB._compare(case, start, 0, got)


def test_gcn3_trainer_epoch_on_hub_ladder(gpu):
    """The same for the 3-layer trainer, with the gates of test_train3_backward_gpu.py."""
    import test_train3_backward_gpu as TB3
    case = B.train_case3()
    params = [TB3._dev(p.copy()) for p in case["params"]]
    tr = TB3._trainer(case, params)
    start = TB3._host(params)
    loss, correct = tr.run(1)
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(TB3.K3.NAMES, tr.grads())}
    got["Z3"] = tr.logits().cpu().numpy().astype(np.float64)
    got["H1d"] = tr.hidden(1).cpu().numpy().astype(np.float64)
    got["H2d"] = tr.hidden(2).cpu().numpy().astype(np.float64)
    got["loss"], got["correct"] = float(loss[0]), int(correct[0])
    TB3._compare(case, start, 0, got)


# ---- lt_graph_reached_rows ----------------------------------------------------------------------------------------------------------
def test_reached_rows_at_128_and_129(gpu):
    """Probes: one pool node out of each ladder row.  min_entries = 128 keeps the row of exactly 128 entries, 129 drops it."""
    g = B.hub_ladder()
    probes = np.array([g.row_sets[d][d // 2] for d in sorted(g.u) if d > 0], dtype=np.int32)
    csc = g.a.tocsc()
    reach = np.unique(np.concatenate([csc.indices[csc.indptr[v]:csc.indptr[v + 1]] for v in probes]))
    lens = np.diff(g.a.indptr)
    base = _baseline("hub", *B.MODEL_SHAPES[0])
    got = {m: base.reached_rows(probes, m).cpu().numpy() for m in (B.LT_ROW_SEG, B.LT_ROW_SEG + 1)}
    for m, rows in got.items():
        assert np.array_equal(rows, reach[lens[reach] >= m]), m
    assert g.u[128] in got[128] and g.u[128] not in got[129] and g.u[129] in got[129] and g.u[127] not in got[128]


# ---- lt_gemm_f32 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [128, 192, 130])
@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_gemm_at_the_tile_switch(gpu, m, n):
    """M >= 1024 with N % 128 == 0 takes the 128 x 128 tiles; K is summed in chains of 128.  Against fp64 with the bound of
    test_gemm_matches_numpy, and the first 65 rows bit-equal to a 65-row call of the same operands (a row's bits do not depend on
    the row count)."""
    from linkteller_amd import _lib, engine

    def gemm(da, db, rows, k):
        out = _sentinel(rows, n)          # (a tile nobody writes keeps its NaN)
        _lib.check(_lib.lib().lt_gemm_f32(da.data_ptr(), k, db.data_ptr(), n, out.data_ptr(), n, rows, n, k, engine._stream()), "lt_gemm_f32")
        return out.cpu().numpy()

    rng = np.random.RandomState(m + n)
    for k in (15, 16, 17, 127, 128, 129, 257):
        a = rng.standard_normal((m, k)).astype(np.float32)
        b = rng.standard_normal((k, n)).astype(np.float32)
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        got = gemm(da, db, m, k)
        want = a.astype(np.float64) @ b.astype(np.float64)
        assert np.abs(got - want).max() <= 2e-6 * np.sqrt(k) * max(1.0, np.abs(want).max()), k
        assert np.array_equal(got[:65], gemm(da, db, 65, k)), k          # (the first 65 rows of A: the same pointer and lda)

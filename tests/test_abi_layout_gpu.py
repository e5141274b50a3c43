"""The layout contract of the C ABI on the inference side: "All matrices are row-major fp32 with an explicit leading
dimension in elements" (include/linkteller_hip.h), handed over as ``data_ptr()`` of tensors the library did not allocate.

engine.py always passes ld == width and a 512-byte aligned base, so the branches the library selects by ``ld`` and pointer
alignment never ran under the suite: the mixed vector / 8-lane path of lt_spmm_csr_f32 and its fall-backs, AV = 2 / 1 of the
int8 split, VEC = 1 of the feature-difference rows and their shifted last window over a padded X, the ring's fall-back, the
16-byte gathers of the aggregate-first route, ldd > n_obs in the packed host landing, ldo > n_obs everywhere but the pair list.

Every case here is the same call made twice: the CONTROL contiguous and aligned (what the engine does; for a width that
cannot be both -- an odd F -- padded to a multiple of 4 and aligned), and through tests/abi_views.py with the operands as
windows of larger buffers.  Inputs sit in buffers whose pads hold a quiet NaN (a pad value that reaches arithmetic shows in
the result), outputs in sentinel-filled buffers.  Assertions, the strongest the code supports:
  (a) bit-equal to the control wherever the kernel is chosen by shape alone (loads of another width, stores with another
      stride: the same chains);
  (b) where alignment changes the fp64 summation order or the kernel (VEC of the feature rows, ring or rows, narrow or
      vector SpMM): `delta` within 1e-5 of the largest score of the fp64 oracle and within 1e-6 of the control (README /
      header); SpMM within 1e-5 * max(1, |want|.max()) of an fp64 host product (test_spmm_matches_scipy); GEMM within
      2e-6 * (|A| |B|).max() (test_gemm_tile_routes_give_the_same_rows);
  (c) every pad word of every output keeps its bits, and exact zeros where the oracle has exact zeros.
No tolerance of its own.
"""
import contextlib
import functools
import types

import numpy as np
import pytest
import torch

import abi_views as V

pytestmark = pytest.mark.gpu

DELTA = 1e-4


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


def _up4(v):
    return (v + 3) // 4 * 4


# ---- A. lt_gemm_f32 ----------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(65, 33, 17), (130, 257, 70), (1031, 300, 256)]         # (M, K, N); the last one takes the 128 x 128 tiles
GEMM_LAYOUTS = [(1, 1, 1, 1, 1, 1), (2, 2, 2, 2, 2, 2), (4, 4, 4, 0, 0, 0), (3, 5, 7, 1, 2, 3)]   # ld - width x3, offsets x3


@functools.lru_cache(maxsize=None)
def _gemm_case(m, k, n):
    rng = np.random.RandomState(m + k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    b = rng.standard_normal((k, n)).astype(np.float32)
    c = V.View.output(m, n)
    V.gemm(V.View(a), V.View(b), c, m, n, k)
    torch.cuda.synchronize()
    ref = a.astype(np.float64) @ b.astype(np.float64)
    bound = 2e-6 * np.abs(a).astype(np.float64).dot(np.abs(b).astype(np.float64)).max()
    control = c.body()
    assert np.abs(control - ref).max() <= bound
    return a, b, control, ref, bound


@pytest.mark.parametrize("layout", GEMM_LAYOUTS, ids=lambda l: "ld+%d.%d.%d_off%d.%d.%d" % l)
@pytest.mark.parametrize("m,k,n", GEMM_SHAPES)
def test_gemm_strided_operands(gpu, m, k, n, layout):
    """lt_launch_gemm dispatches on (M, N, K) alone and reads A and B through alignment-4 vector types: any lda / ldb / ldc
    and any 4-byte aligned base give the control's bits; the pads of C stay, the NaNs beside A's and B's rows stay out."""
    da, db, dc, oa, ob, oc = layout
    a, b, control, ref, bound = _gemm_case(m, k, n)
    c = V.View.output(m, n, ld=n + dc, off=oc)
    V.gemm(V.View(a, k + da, oa), V.View(b, n + db, ob), c, m, n, k)
    torch.cuda.synchronize()
    got = c.body()
    assert np.array_equal(got, control)
    assert c.pads_untouched(), c.touched_pads()[:8]
    assert np.abs(got - ref).max() <= bound


def test_gemm_k_zero_writes_zeros_and_nothing_else(gpu):
    m, n = 65, 17
    c = V.View.output(m, n, ld=n + 3, off=1)
    V.gemm(V.View(np.zeros((m, 0), np.float32), 1, 1), V.View(np.zeros((0, n), np.float32), n + 1, 1), c, m, n, 0)
    torch.cuda.synchronize()
    got = c.body()
    assert np.all(got == 0) and not np.signbit(got).any()
    assert c.pads_untouched()


# ---- B. lt_spmm_csr_f32 ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spmm_graph():
    from test_gpu_parity import _hub_graph
    from linkteller_amd import graph
    a_hat = graph.first_order_gcn(_hub_graph(1200, 6000, 700, seed=5))       # the hub graph of test_spmm_any_width
    return a_hat, graph.HipGraph(a_hat)


@functools.lru_cache(maxsize=None)
def _spmm_inputs(ncols):
    rng = np.random.RandomState(ncols)
    a_hat, _ = _spmm_graph()
    s = rng.standard_normal((a_hat.shape[0], ncols)).astype(np.float32)
    b = rng.standard_normal(ncols).astype(np.float32)
    return s, b, a_hat.astype(np.float64) @ s.astype(np.float64)


def _spmm_want(ncols, epilogue):
    s, b, prod = _spmm_inputs(ncols)
    return np.maximum(prod + b, 0) if epilogue else prod


def _spmm_run(ncols, epilogue, tiled, lds, ldo, off_s=0, off_o=0, off_b=0, s=None, b=None):
    """One lt_spmm_csr_f32 call on windows; returns the result window after checking the pads of the output."""
    from linkteller_amd import _lib
    _, hg = _spmm_graph()
    if s is None:
        s, b, _ = _spmm_inputs(ncols)
    out = V.View.output(s.shape[0], ncols, ld=ldo, off=off_o)
    with knobs(**({"tiled_min_bytes": 0} if tiled else {})):
        wide = min(ncols // 4 * 4, 256)
        if wide:
            assert _lib.lib().lt_spmm_route(hg.handle, wide) == int(tiled)
        V.spmm(hg, V.View(s, lds, off_s), ncols, V.View(b, off=off_b) if epilogue else None, epilogue, out)
        torch.cuda.synchronize()
    assert out.pads_untouched(), out.touched_pads()[:8]
    return out.body()


ROUTES = pytest.mark.parametrize("tiled", [False, True], ids=["rows", "tiled"])
EPILOGUE = pytest.mark.parametrize("epilogue", [True, False], ids=["bias_relu", "plain"])


@ROUTES
@EPILOGUE
@pytest.mark.parametrize("ncols", [9, 262, 510])
def test_spmm_vector_slices_then_the_tail(gpu, ncols, epilogue, tiled):
    """lds % 4 == 0 with ncols % 4 != 0 (impossible while lds == ncols): 256-column vector slices over ncols / 4 * 4 columns,
    the last ncols % 4 through the 8-lane kernel.  The vector columns carry "the bits a single wide pass would give" -- those of
    a contiguous call of that many columns; the tail sits within the fp64 bound; the NaNs behind every row stay out."""
    ld = _up4(ncols) + 4
    wide = ncols // 4 * 4
    s, b, _ = _spmm_inputs(ncols)
    got = _spmm_run(ncols, epilogue, tiled, ld, ld)
    sw, bw = np.ascontiguousarray(s[:, :wide]), np.ascontiguousarray(b[:wide])
    control = _spmm_run(wide, epilogue, tiled, wide, wide, s=sw, b=bw)
    assert np.array_equal(got[:, :wide], control)
    want = _spmm_want(ncols, epilogue)
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


SPMM_FALLBACKS = [            # (ncols, lds - ncols, ldo - ncols, off S, off out, off bias): what the vector path cannot take
    (256, 1, 1, 0, 0, 0), (260, 1, 1, 0, 0, 0),            # odd leading dimensions
    (260, 4, 4, 1, 0, 0), (260, 4, 4, 0, 1, 0), (260, 4, 4, 0, 0, 1),      # aligned ld, one base 4 bytes off
]
# (a call without bias has no bias pointer to misalign)
SPMM_FALLBACK_PARAMS = [(c, e) for c in SPMM_FALLBACKS for e in (True, False) if e or not c[5]]


@ROUTES
@pytest.mark.parametrize("case,epilogue", SPMM_FALLBACK_PARAMS,
                         ids=["n%d_ld+%d.%d_off%d.%d.%d" % c + ("-bias_relu" if e else "-plain") for c, e in SPMM_FALLBACK_PARAMS])
def test_spmm_unaligned_operands_take_the_narrow_kernel(gpu, case, epilogue, tiled):
    """vec_ok of lt_spmm_csr_f32: an odd lds / ldo, or S, out or bias off a 16-byte boundary, sends ALL columns through the 8-lane
    kernel, 8 per launch (another chain layout: the fp64 bound)."""
    ncols, ds, do, os_, oo, ob = case
    got = _spmm_run(ncols, epilogue, tiled, ncols + ds, ncols + do, os_, oo, ob)
    want = _spmm_want(ncols, epilogue)
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


@ROUTES
@EPILOGUE
@pytest.mark.parametrize("lds,ldo", [(12, 8), (8, 12)])
def test_spmm_eight_columns_with_padded_rows(gpu, lds, ldo, epilogue, tiled):
    """4 or 8 columns, everything aligned: the vector path with another stride -- the control's bits."""
    got = _spmm_run(8, epilogue, tiled, lds, ldo)
    control = _spmm_run(8, epilogue, tiled, 8, 8)
    assert np.array_equal(got, control)
    want = _spmm_want(8, epilogue)
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


# ---- datasets of the probe primitive -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dataset(kind, n, f, h, c=2, graph_kind="er"):
    """Graph, features, weights, node lists (nodes 0 and n - 1 probed and observed: the first row of X and the shifted last
    window), the fp64 oracle once."""
    from test_gpu_parity import _hub_graph, _oracle_matrix
    from linkteller_amd import graph, synth
    if graph_kind == "hub":
        adj = _hub_graph(n, 5 * n, n // 2, seed=n)
    else:
        adj = synth.erdos_renyi_graph(n, 4 * n, seed=n)
    a_hat = graph.first_order_gcn(adj)
    if kind == "gaussian":
        x = synth.gaussian_features(n, f, seed=f)
    else:
        # (a row's differing columns fit a wave's list: ~14 of them at every width)
        x = synth.twitch_like_features(n, f, seed=f, density=0.006 if f >= 2000 else (0.02 if f >= 500 else 0.1))
        x[n - 1, f - 1] = 2.5              # the last value of the matrix and the first differ from the reference row
        x[0, 0] = -1.5
    w = synth.gcn_weights(f, h, c, seed=h)
    rng = np.random.RandomState(f + h)
    inner = np.arange(1, n - 1)
    probes = np.concatenate([[0, n - 1], rng.choice(inner, 10, replace=False)]).astype(np.int32)
    near = np.unique(np.concatenate([a_hat.indices[a_hat.indptr[v]:a_hat.indptr[v + 1]][:4] for v in probes]))      # in reach of a probe
    near = near[(near > 0) & (near < n - 1)][:24]
    far = np.setdiff1d(inner, near)
    obs = np.concatenate([[n - 1, 0], near, rng.choice(far, 46 - len(near), replace=False)]).astype(np.int32)
    ref64 = _oracle_matrix(a_hat, x, w, probes.astype(np.int64), obs.astype(np.int64), DELTA, torch.float64)
    assert ref64.max() > 0
    return types.SimpleNamespace(a_hat=a_hat, hg=graph.HipGraph(a_hat), x=x, w=w, n=n, f=f, h=h, c=c, probes=probes, obs=obs,
                                 ref64=ref64, scale=ref64.max())


def _weights(ds, off=0):
    return [V.View(ds.w[k], off=off) for k in ("W1", "b1", "W2", "b2")]


def _baseline(ds, ldx, off, w_off=0):
    w1, b1, w2, b2 = _weights(ds, w_off)
    return V.RawBaseline(ds.hg, V.View(ds.x, ldx, off), ds.f, w1, b1, ds.h, w2, b2, ds.c)


def _rows(ds, ldx, off, mode, route=None, w_off=0, ldo=None, off_o=0, **kn):
    """One baseline on X as a window, one lt_influence_rows call; the route asserted, the output's pads checked."""
    with knobs(**kn):
        base = _baseline(ds, ldx, off, w_off)
        try:
            if mode == "delta":
                base.enable_fp64()
                if route is not None:
                    assert base.fp64_route() == route
            out = V.View.output(len(ds.probes), len(ds.obs), ld=ldo, off=off_o)
            got = base.rows(ds.probes, ds.obs, DELTA, mode, out)
            assert out.pads_untouched(), out.touched_pads()[:8]
        finally:
            base.destroy()
    return got.astype(np.float64)


_controls = {}


def _control(ds_key, mode, route, **kn):
    """The same call as the engine makes it: X contiguous and aligned (a width that is no multiple of 4 cannot be both: padded
    to the next one, aligned)."""
    key = (ds_key, mode, tuple(sorted(kn.items())))
    if key not in _controls:
        ds = _dataset(*ds_key)
        _controls[key] = _rows(ds, ds.f if ds.f % 4 == 0 else _up4(ds.f), 0, mode, route, **kn)
    return _controls[key]


def _check_delta(ds, got, control, exact):
    assert np.isfinite(got).all()
    if exact:
        assert np.array_equal(got, control), np.abs(got - control).max() / ds.scale
    print(f"|got - control| / max = {np.abs(got - control).max() / ds.scale:.2e}, |got - fp64| / max = {np.abs(got - ds.ref64).max() / ds.scale:.2e}")
    assert np.abs(got - control).max() <= 1e-6 * ds.scale
    assert np.abs(got - ds.ref64).max() <= 1e-5 * ds.scale
    assert np.all(got[ds.ref64 == 0] == 0)


# ---- C. lt_gcn2_forward ------------------------------------------------------------------------------------------------
def test_gcn2_forward_strided_features_and_logits(gpu):
    from linkteller_amd import _lib, graph, synth
    from oracle import linkteller_oracle as O
    n, f, h, c = 300, 70, 24, 3
    a_hat = graph.first_order_gcn(synth.powerlaw_graph(n, 1500, seed=7))
    hg = graph.HipGraph(a_hat)
    x = synth.gaussian_features(n, f, seed=1)
    w = synth.gcn_weights(f, h, c, seed=2)

    def run(x_view, out, w_off=0):
        ws = [V.View(w[k], off=w_off) for k in ("W1", "b1", "W2", "b2")]
        _lib.check(V.gcn2_forward(hg, x_view, f, ws[0], ws[1], h, ws[2], ws[3], c, out), "lt_gcn2_forward")
        torch.cuda.synchronize()
        assert out.pads_untouched(), out.touched_pads()[:8]
        return out.body()

    control = run(V.View(x), V.View.output(n, c))
    ref = O.gcn_forward(torch.from_numpy(x).double(), O.to_torch_sparse(a_hat).double(),
                        {k: torch.from_numpy(v).double() for k, v in w.items()}).numpy()
    assert np.abs(control - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6          # (the bound of test_forward_logits)
    got = run(V.View(x, f + 3, 1), V.View.output(n, c, ld=c + 2, off=1))
    assert np.array_equal(got, control)
    assert np.array_equal(run(V.View(x, f + 3, 1), V.View.output(n, c, ld=c + 2, off=1), w_off=1), control)
    # a leading dimension smaller than the row is refused (LT_ERR_INVALID) before anything is enqueued
    bad = V.View.output(n, c)
    bad.ld = c - 1
    ws = [V.View(w[k]) for k in ("W1", "b1", "W2", "b2")]
    assert V.gcn2_forward(hg, V.View(x), f, ws[0], ws[1], h, ws[2], ws[3], c, bad) == -1
    torch.cuda.synchronize()
    assert np.all(bad.buf.cpu().numpy() == -7.0)


# ---- D. the 2-layer baseline, mode `delta`, per fp64 route --------------------------------------------------------------
GAUSS = ("gaussian", 700, 300, 64)
F64_CORES = dict(feature_delta=0, i8_split=0, aggregate_first=0)
I8_SPLIT = dict(feature_delta=0, i8_split=1, aggregate_first=0)


@pytest.mark.parametrize("f,ldx,off", [(300, 301, 1), (300, 304, 0), (301, 301, 0), (300, 303, 3)])
def test_delta_on_the_f64_matrix_cores(gpu, f, ldx, off):
    """k_gemm_f64acc reads X through alignment-4 vector types and picks vector or scalar loads by K alone: the control's bits."""
    key = ("gaussian", 700, f, 64)
    ds = _dataset(*key)
    got = _rows(ds, ldx, off, "delta", 0, **F64_CORES)
    _check_delta(ds, got, _control(key, "delta", 0, **F64_CORES), exact=True)


I8_CASES = [(300, 304, 0, 4), (302, 302, 0, 2), (300, 302, 2, 2), (301, 301, 0, 1), (300, 301, 1, 1), (300, 304, 1, 1)]


@pytest.mark.parametrize("f,ldx,off,av", I8_CASES, ids=lambda v: str(v))
def test_delta_on_the_int8_split(gpu, f, ldx, off, av):
    """lt_launch_gemm_i8split picks AV = 4 / 2 / 1 floats per load from ldx and the base pointer (AV = 2 and 1 never ran under
    the suite, and they serve every dense X with an odd F).  The width of a load changes no digit: the control's bits."""
    key = ("gaussian", 700, f, 64)
    ds = _dataset(*key)
    ptr_mod = (4 * off) % 16
    assert av == (4 if ldx % 4 == 0 and ptr_mod == 0 else (2 if ldx % 2 == 0 and ptr_mod % 8 == 0 else 1))
    got = _rows(ds, ldx, off, "delta", 0, **I8_SPLIT)
    _check_delta(ds, got, _control(key, "delta", 0, **I8_SPLIT), exact=True)
    f64 = _control(key, "delta", 0, **F64_CORES)
    assert np.abs(got - f64).max() <= 1e-6 * ds.scale          # ("i8_split": agrees to < 1e-6 of the largest score)


FEATURE_ROWS = [(700, 702, 2, 2), (701, 701, 0, 1), (700, 703, 0, 1), (700, 700, 1, 1)]      # (F, ldx, off, VEC)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("f,ldx,off,vec", FEATURE_ROWS, ids=lambda v: str(v))
def test_delta_on_the_feature_difference_rows(gpu, f, ldx, off, vec, flags):
    """k_s1d_feature_rows: VEC = 2 needs ldx and F even and 8-byte aligned rows (every F of the suite was even: VEC = 1 never
    ran).  A trip's loads run past the end of a row -- with ldx > F into the NaN pad -- and the last rows' window is shifted
    left: masked by j < F and j >= j0, which nothing checked over a pad.  VEC changes the order of a row's list: fp64
    summation order, bound (b)."""
    key = ("indicator", 900, f, 102)
    ds = _dataset(*key)
    assert vec == (2 if ldx % 2 == 0 and f % 2 == 0 and (4 * off) % 8 == 0 else 1)
    kn = dict(feature_delta=1, feature_flags=flags)
    got = _rows(ds, ldx, off, "delta", 1, **kn)
    _check_delta(ds, got, _control(key, "delta", 1, **kn), exact=False)


def test_delta_on_the_feature_difference_rows_with_the_reference_product_first(gpu):
    key = ("indicator", 900, 700, 102)
    ds = _dataset(*key)
    kn = dict(feature_delta=1, defer_cref=0)
    got = _rows(ds, 703, 0, "delta", 1, **kn)
    _check_delta(ds, got, _control(key, "delta", 1, **kn), exact=False)


RING = ("indicator", 1300, 2300, 64)


@pytest.mark.parametrize("ldx,off,ring", [(2302, 2, True), (2301, 0, False), (2300, 1, False)])
def test_delta_on_the_ring_and_its_fall_back(gpu, ldx, off, ring):
    """fd_ring_ok gates the LDS-ring kernel on 8-byte aligned rows (ldx even, X % 8 == 0).  With the knob at 1 and a layout the
    ring cannot take, the row-per-wave kernel must serve the call: the bits of the same layout with the knob at 0."""
    ds = _dataset(*RING)
    kn = dict(feature_delta=1, feature_ring=1)
    got = _rows(ds, ldx, off, "delta", 1, **kn)
    _check_delta(ds, got, _control(RING, "delta", 1, **kn), exact=False)
    rows_kernel = _rows(ds, ldx, off, "delta", 1, feature_delta=1, feature_ring=0)
    if not ring:
        assert np.array_equal(got, rows_kernel)
    assert np.abs(got - rows_kernel).max() <= 1e-6 * ds.scale


AGG_CASES = [(33, 24, 34, 1), (64, 100, 67, 0), (64, 100, 68, 0), (64, 100, 68, 1)]


@pytest.mark.parametrize("f,h,ldx,off", AGG_CASES)
def test_delta_aggregate_first(gpu, f, h, ldx, off):
    """k_rows_tiled_xf64 gathers rows of X 16 bytes at a time when they allow it (ldx % 4 == 0 and a 16-byte aligned base), one
    float at a time otherwise; the probes' product rows read X float by float.  The same fp64 chains: the control's bits."""
    key = ("gaussian", 1300, f, h, 2, "hub")
    ds = _dataset(*key)
    got = _rows(ds, ldx, off, "delta", 2, aggregate_first=1)
    _check_delta(ds, got, _control(key, "delta", 2, aggregate_first=1), exact=True)


WEIGHT_CASES = [
    (GAUSS, 301, 1, 0, F64_CORES, True),
    (GAUSS, 301, 1, 0, I8_SPLIT, True),
    (("indicator", 900, 700, 102), 703, 0, 1, dict(feature_delta=1), False),
    (RING, 2302, 2, 1, dict(feature_delta=1, feature_ring=1), False),          # W1 4 bytes off: the ring must decline
    (RING, 2300, 0, 1, dict(feature_delta=1, feature_ring=0), False),          # the rows kernel's 16-byte loads of W1 rows
    (("gaussian", 1300, 64, 100, 2, "hub"), 67, 0, 2, dict(aggregate_first=1), True),
]


@pytest.mark.parametrize("key,ldx,off,route,kn,exact", WEIGHT_CASES, ids=lambda v: None)
def test_delta_with_every_weight_tensor_four_bytes_off(gpu, key, ldx, off, route, kn, exact):
    """W1, b1, W2, b2 are borrowed as well: each at base + 4 bytes.  The readers of W1 that load 16 bytes at a time (the
    feature-difference walk, the reference row's product) must not assume more than the 4-byte alignment of a float."""
    ds = _dataset(*key)
    got = _rows(ds, ldx, off, "delta", route, w_off=1, **kn)
    _check_delta(ds, got, _control(key, "delta", route, **kn), exact=exact)
    if kn.get("feature_ring") == 1:
        assert np.array_equal(got, _rows(ds, ldx, off, "delta", route, w_off=1, feature_delta=1, feature_ring=0))


# ---- E. the fp32 modes and lt_influence_pairs on a strided X -------------------------------------------------------------
@pytest.mark.parametrize("key", [GAUSS, ("indicator", 900, 700, 102)], ids=["gaussian", "indicator"])
def test_fp32_modes_and_pairs_on_strided_features(gpu, key):
    """FULL / SPARSE read X only through lt_launch_gemm / _splitk (the baseline product, the probes' gathered rows): the
    control's bits.  lt_influence_pairs gives what the rows call gives at the listed cells, on the same window of X."""
    ds = _dataset(*key)
    ctl = {m: _control(key, m, None) for m in ("sparse", "full")}
    assert np.array_equal(ctl["sparse"], ctl["full"])
    base = _baseline(ds, ds.f + 1, 1)
    try:
        got = {}
        for m in ("sparse", "full"):
            out = V.View.output(len(ds.probes), len(ds.obs))
            got[m] = base.rows(ds.probes, ds.obs, DELTA, m, out).astype(np.float64)
            assert np.array_equal(got[m], ctl[m]), m
            assert np.all(got[m][ds.ref64 == 0] == 0)
        base.enable_fp64()
        out = V.View.output(len(ds.probes), len(ds.obs))
        got["delta"] = base.rows(ds.probes, ds.obs, DELTA, "delta", out).astype(np.float64)
        assert np.abs(got["delta"] - ds.ref64).max() <= 1e-5 * ds.scale
        # every third cell of every probe's row as a pair list
        cols = [np.arange(i % 3, len(ds.obs), 3) for i in range(len(ds.probes))]
        ptr = np.concatenate([[0], np.cumsum([len(c_) for c_ in cols])]).astype(np.int64)
        pair_obs = np.concatenate([ds.obs[c_] for c_ in cols]).astype(np.int32)
        for m in ("delta", "sparse"):
            want = np.concatenate([got[m][i, c_] for i, c_ in enumerate(cols)])
            assert np.array_equal(base.pairs(ds.probes, ptr, pair_obs, DELTA, m).astype(np.float64), want), m
    finally:
        base.destroy()


# ---- F. ldo / ldd ---------------------------------------------------------------------------------------------------------
_shared = {}


# (graphs of this size would form the pre-activation aggregate-first, which is neither the fused record route nor the S1d routes
#  behind the item kernels: pinned off where the baseline allocates and in every call)
NO_AGG = dict(aggregate_first=0)


def _shared_baseline(graph_kind):
    """One contiguous baseline per graph for the store-stride cases (fp64 on): only the layout of the RESULT varies there."""
    if graph_kind not in _shared:
        ds = _dataset("indicator", 1200, 96, 64, 2, graph_kind)
        with knobs(**NO_AGG):
            base = _baseline(ds, ds.f, 0).enable_fp64()
            assert base.fp64_route() in (0, 1)
        _shared[graph_kind] = (ds, base)
    return _shared[graph_kind]


def _node_lists(ds, n_obs):
    rng = np.random.RandomState(n_obs)
    obs = np.concatenate([[ds.n - 1], rng.choice(ds.n - 1, n_obs - 1, replace=False)]).astype(np.int32)
    probes = np.concatenate([obs[: max(1, min(n_obs // 2, 24))], [0]]).astype(np.int32)
    return probes, obs


LDO_ROUTES = {
    #                 graph, mode, knobs
    "fused_records": ("er", "delta", {}),
    "items_stageb_rows": ("hub", "delta", dict(delta_fused=0, stageb_rows=1)),
    "items_stageb_pairs": ("hub", "delta", dict(delta_fused=0, stageb_rows=0)),
    "pair_marks_no_list": ("hub", "delta", dict(delta_fused=0, pair_marks=0, pair_list=0)),
    "sparse": ("hub", "sparse", {}),
    "full": ("hub", "full", {}),
}


@pytest.mark.parametrize("pad", [1, 3])
@pytest.mark.parametrize("n_obs", [1, 7, 64, 257])
@pytest.mark.parametrize("route", list(LDO_ROUTES))
def test_result_rows_wider_than_the_observed_list(gpu, route, n_obs, pad):
    """ldo > n_obs with the result 4 bytes off a 16-byte boundary, on every route that stores result rows: the same kernels with
    another store stride -- the control's bits, and columns n_obs .. ldo - 1 keep theirs.  (That "fused_records" -- a graph with
    incidence records, default knobs -- is the fused route is what test_host_matrix_with_padded_rows proves on the same baseline:
    its packed landing exists on that route only.)"""
    graph_kind, mode, kn = LDO_ROUTES[route]
    ds, base = _shared_baseline(graph_kind)
    probes, obs = _node_lists(ds, n_obs)
    with knobs(**NO_AGG, **kn):
        base.refresh()
        control = base.rows(probes, obs, DELTA, mode, V.View.output(len(probes), n_obs))
        base.refresh()
        out = V.View.output(len(probes), n_obs, ld=n_obs + pad, off=1)
        got = base.rows(probes, obs, DELTA, mode, out)
    assert np.array_equal(got, control)
    assert out.pads_untouched(), out.touched_pads()[:8]
    assert np.isfinite(control).all() and (control > 0).any()


@pytest.mark.parametrize("mode", ["sparse", "delta"])
@pytest.mark.parametrize("n_obs,pad", [(1, 1), (7, 3), (64, 1), (257, 3)])
def test_difference_vectors_with_a_wider_result(gpu, n_obs, pad, mode):
    """lt_influence_rows_vec indexes vec with ldo too: vec[(i * ldo + j) * C + c]."""
    ds, base = _shared_baseline("hub")
    probes, obs = _node_lists(ds, n_obs)
    npb, c = len(probes), ds.c
    ldo = n_obs + pad
    out, vec = V.View.output(npb, n_obs, ld=ldo, off=1), V.View.output(npb, n_obs * c, ld=ldo * c, off=1)
    with knobs(**NO_AGG):
        base.refresh()
        c_out, c_vec = base.rows_vec(probes, obs, DELTA, mode, V.View.output(npb, n_obs), V.View.output(npb, n_obs * c))
        base.refresh()
        g_out, g_vec = base.rows_vec(probes, obs, DELTA, mode, out, vec)
    assert np.array_equal(g_out, c_out) and np.array_equal(g_vec, c_vec)
    assert out.pads_untouched() and vec.pads_untouched(), (out.touched_pads()[:8], vec.touched_pads()[:8])
    # the norm of the vectors is the score (lt_wide_combine's arithmetic on one slice), wherever the vector is non-zero
    assert np.array_equal(c_out == 0, ~(c_vec.reshape(npb, n_obs, c) != 0).any(axis=2))


@pytest.mark.parametrize("refresh", [True, False], ids=["refreshed", "warm"])
@pytest.mark.parametrize("early", [0, 2])
@pytest.mark.parametrize("compact", [None, 2], ids=["compact_default", "compact_always"])
@pytest.mark.parametrize("n_obs", [1, 7, 64, 257])
def test_host_matrix_with_padded_rows(gpu, n_obs, compact, early, refresh):
    """lt_influence_matrix_host packs "indices into dst", i * ldd + j, and promises that "columns n_obs .. ldd - 1 are left as
    they are": ldd = n_obs + 3, ldo = n_obs + 1, a pinned destination that held a sentinel everywhere."""
    ds, base = _shared_baseline("er")
    probes, obs = _node_lists(ds, n_obs)
    npb, ldd = len(probes), n_obs + 3
    before = base.host_landing_stats()
    dst = torch.full((npb * ldd + 8,), 7.0, dtype=torch.float64).pin_memory()
    out = V.View.output(npb, n_obs, ld=n_obs + 1, off=1)
    with knobs(export_compact=compact, export_early=early, **NO_AGG):
        base.refresh()
        control = base.rows(probes, obs, DELTA, "delta", V.View.output(npb, n_obs))
        if refresh:
            base.refresh()
        got = base.matrix_host(probes, obs, DELTA, "delta", out, dst, ldd)
    torch.cuda.synchronize()
    after = base.host_landing_stats()
    assert np.array_equal(got, control) and out.pads_untouched()
    host = dst.numpy()
    mat = host[: npb * ldd].reshape(npb, ldd)
    assert np.array_equal(mat[:, :n_obs], control.astype(np.float64))
    assert np.all(mat[:, n_obs:] == 7.0) and np.all(host[npb * ldd:] == 7.0)
    assert after[3] == 0 and after[3] == before[3]            # (index words the early look saw differently: none)
    if compact == 2:
        assert after[0] + after[1] == before[0] + before[1] + 1, "the call was not packed: the case would prove nothing"


# ---- G. the 3-layer model --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gcn3_case():
    """The smallest parameter set of test_gcn3_delta_mode_against_the_fp64_oracle."""
    import scipy.sparse as sp
    from linkteller_amd import graph, synth
    from oracle import linkteller_oracle as O
    h1, h2, c, n, f = 32, 16, 2, 220, 300
    a = synth.powerlaw_graph(n, 600, seed=h1).tolil()
    for k in (5, 17, 99):
        a[k, :] = 0
        a[:, k] = 0
    a = sp.csr_matrix(a)
    a.eliminate_zeros()
    a_hat = graph.first_order_gcn(a)
    x = synth.gaussian_features(n, f, seed=3)
    rng = np.random.RandomState(h2)

    def u(shape, fan):
        s = 1.0 / np.sqrt(fan)
        return rng.uniform(-s, s, size=shape).astype(np.float32)

    P = dict(W1=u((f, h1), h1), b1=u((h1,), h1), W2=u((h1, h2), h2), b2=u((h2,), h2), W3=u((h2, c), c), b3=u((c,), c))
    probes = np.concatenate([rng.choice(n, 10, replace=False), [0, n - 1, 5]]).astype(np.int32)
    obs = np.concatenate([rng.choice(n, 40, replace=False), [0, n - 1, 99]]).astype(np.int32)
    adj_t = O.to_torch_sparse(a_hat).double()
    Pd = {k: torch.from_numpy(v).double() for k, v in P.items()}
    xt = torch.from_numpy(x).double()
    ref64 = np.zeros((len(probes), len(obs)))
    with torch.no_grad():
        for i, v in enumerate(probes):
            gm = O.get_gradient_eps_mat(xt, adj_t, Pd, int(v), DELTA, forward=O.gcn3_forward)
            ref64[i] = gm[torch.as_tensor(obs.astype(np.int64))].norm(dim=1).numpy()
    return types.SimpleNamespace(hg=graph.HipGraph(a_hat), x=x, P=P, dims=(f, h1, h2, c), probes=probes, obs=obs, ref64=ref64,
                                 scale=ref64.max())


def _gcn3_rows(cs, ldx, off, mode, ldo, off_o, gather):
    f, h1, h2, c = cs.dims
    P = cs.P
    with knobs(gcn3_product_gather=gather):
        base = V.RawBaseline3(cs.hg, V.View(cs.x, ldx, off), f, V.View(P["W1"]), V.View(P["b1"]), h1, V.View(P["W2"]), V.View(P["b2"]),
                              h2, V.View(P["W3"]), V.View(P["b3"]), c)
        try:
            if mode == "delta":
                base.enable_fp64()
            out = V.View.output(len(cs.probes), len(cs.obs), ld=ldo, off=off_o)
            got = base.rows(cs.probes, cs.obs, DELTA, mode, out)
            assert out.pads_untouched(), out.touched_pads()[:8]
        finally:
            base.destroy()
    return got.astype(np.float64)


@pytest.mark.parametrize("gather", [1, 0])
@pytest.mark.parametrize("mode", ["sparse", "delta"])
def test_gcn3_strided_features_and_result(gpu, mode, gather):
    cs = _gcn3_case()
    f, nob = cs.dims[0], len(cs.obs)
    control = _gcn3_rows(cs, f, 0, mode, nob, 0, gather)
    got = _gcn3_rows(cs, f + 1, 1, mode, nob + 3, 1, gather)
    assert np.isfinite(got).all() and np.all(got[cs.ref64 == 0] == 0)
    if mode == "sparse":
        assert np.array_equal(got, control)
    else:
        assert np.abs(got - control).max() <= 1e-6 * cs.scale
        assert np.abs(got - cs.ref64).max() <= 1e-5 * cs.scale

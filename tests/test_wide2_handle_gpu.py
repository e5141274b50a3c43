"""The one-handle route of the wide 2-layer attack (lt_baseline2w_create, 1 .. 256 classes behind up to 256 hidden units;
LT_MODE_DELTA as a rectangle, lt_influence2w_rows, and as a pair list, lt_influence2w_pairs) on the GPU.

The oracle is oracle.linkteller_oracle.influence_matrix on float64 tensors with influence = 1e-4, called on the list (probes ++
observed) with probe_range = the probes, the block [probes, observed] read out of it.  Bounds, the project's own: `delta` within
1e-5 of the largest fp64 score, exact zeros where the oracle has them; two fp32 routes of the same quantity within 2e-5 of it;
logits within 2e-5 max|ref| + 1e-6; AUC / AP within 1e-4.

Graphs (F = 32), restated from test_gcn3_wide_attack_gpu.py: an Erdos-Renyi graph with n = 300 and 1500 edges (two hops reach less
than three: 600 edges leave nine tenths of the fp64 cells at zero, 1500 leave 0.69 -- asserted to lie in [0.1, 0.9], so that the
zero check has something to show), a graph with an isolated node and self loops (n = 120), and the hub ladder of boundary_cases.py
(columns of 129 / 513 entries probed, rows of 129 / 257 / 1025 entries observed).  Node lists: a probe whose feature row is all
zero, u == v, a repeated probe, a repeated observed id.  Shapes (H, C): padded and unpadded Hp / Cp, every lane-group width."""
import argparse
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import boundary_cases as B
from conftest import GOLDEN, csr_from
from linkteller_amd import _lib

pytestmark = pytest.mark.gpu

F = 32
DELTA = 1e-4
SHAPES = ((18, 9), (16, 41), (32, 121), (256, 256), (20, 8), (12, 1))
GRAPHS = ("er", "loops", "hub")
KEYS = ("W1", "b1", "W2", "b2")
LT_ERR_INVALID, LT_ERR_UNSUPPORTED, LT_ERR_WORKSPACE = -1, -3, -4
_ids = {"ids": lambda s: "x".join(map(str, s))}


# ---- cases, built once per process ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(name):
    """(normalised adjacency as float32 CSR, float32 features, probes, observed, index of the all-zero-feature probe)."""
    from linkteller_amd import graph, synth
    if name == "hub":
        g = B.hub_ladder()
        a_hat = sp.csr_matrix(g.a).astype(np.float32)
        x = B.features("hub").copy()
        pool = B.pool_nodes("hub")
        probes = [g.v[129], g.v[513], g.w[(129, "heavy")], g.t[0], int(pool[0]), int(pool[1]), int(pool[2]), int(pool[0])]
        obs = [g.u[129], g.u[257], g.u[1025], int(pool[0]), int(pool[3]), int(pool[4]), g.u[1025], g.u[1]]
        zero = int(pool[2])
    else:
        n, m, seed = (300, 1500, 3) if name == "er" else (120, 260, 4)
        rng = np.random.RandomState(seed)
        a = sp.lil_matrix((n, n))
        while a.nnz < 2 * m:
            i, j = rng.randint(0, n, 2)
            if i != j:
                a[i, j] = a[j, i] = 1.0
        if name == "loops":
            a[5, :] = 0
            a[:, 5] = 0                              # node 5 is isolated
            for i in (0, 7, 40):
                a[i, i] = 1.0                        # self loops in the raw adjacency
        a_hat = sp.csr_matrix(graph.first_order_gcn(sp.csr_matrix(a))).astype(np.float32)
        a_hat.sort_indices()
        x = synth.gaussian_features(n, F, seed=seed + 10).copy()
        pick = rng.choice(n, 44, replace=False)
        probes = list(pick[:24]) + [int(pick[3])]                           # a repeated probe
        obs = list(pick[12:44]) + [int(pick[20]), int(pick[40])]            # overlaps the probes (u == v), repeated ids
        if name == "loops":
            probes += [5, 0, 7]
            obs += [5, 0, 40]
        zero = int(pick[1])
    x[zero] = 0.0                                     # a probe whose feature row is all zero
    probes, obs = np.asarray(probes, dtype=np.int32), np.asarray(obs, dtype=np.int32)
    assert zero in probes and set(probes) & set(obs) and len(set(probes)) < len(probes) and len(set(obs)) < len(obs)
    return a_hat, np.ascontiguousarray(x, dtype=np.float32), probes, obs, int(np.flatnonzero(probes == zero)[0])


@functools.lru_cache(maxsize=None)
def _params(shape, seed=0):
    h, c = shape
    rng = np.random.RandomState(1000 * seed + 3 * h + 7 * c)
    out = {}
    for i, (fi, fo) in enumerate(((F, h), (h, c)), start=1):
        s = 1.0 / np.sqrt(fo)                          # GraphConvolution.reset_parameters (gcn/layers.py)
        out[f"W{i}"] = rng.uniform(-s, s, (fi, fo)).astype(np.float32)
        out[f"b{i}"] = rng.uniform(-s, s, fo).astype(np.float32)
    return out


def _oracle(a_hat, x, params, probes, obs):
    from oracle import linkteller_oracle as O
    torch.set_num_threads(min(16, torch.get_num_threads()))
    nodes = np.concatenate([probes, obs]).astype(np.int64)
    P = {k: torch.from_numpy(np.asarray(v)).double() for k, v in params.items()}
    full = O.influence_matrix(torch.from_numpy(x).double(), O.to_torch_sparse(a_hat).double(), P, nodes, DELTA,
                              probe_range=range(len(probes)))
    return full[:len(probes), len(probes):]


@functools.lru_cache(maxsize=None)
def _ref64(name, shape):
    a_hat, x, probes, obs, _ = _graph(name)
    ref = _oracle(a_hat, x, _params(shape), probes, obs)
    ref.setflags(write=False)
    return ref


def _tensors(name, shape, gpu, params=None):
    from linkteller_amd import graph
    a_hat, x, *_ = _graph(name)
    p = params or _params(shape)
    return graph.HipGraph(a_hat), torch.from_numpy(x).to(gpu), [torch.from_numpy(np.asarray(p[k])).to(gpu) for k in KEYS]


def _baseline(name, shape, gpu, params=None):
    from linkteller_amd import engine
    hg, xt, dev = _tensors(name, shape, gpu, params)
    return engine.Baseline2W(hg, xt, *dev), dev


def _rows(base, probes, obs):
    return base.influence_rows(probes, obs, DELTA, "delta").cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _pairs(name):
    """A pair list over (probes, obs) of the graph: (pair_ptr, pair_obs, column into obs, row into probes) -- a probe that owns no
    pair, the repeated probe with pairs of its own, u == v, a pair listed twice; the pairs of a probe in no order."""
    _, _, probes, obs, zrow = _graph(name)
    rng = np.random.RandomState(77)
    counts = rng.randint(3, 8, len(probes))
    counts[2] = 0
    ptr, col, same = [0], [], 0
    for i, cnt in enumerate(counts):
        mine = list(rng.randint(0, len(obs), cnt))
        own = np.flatnonzero(obs == probes[i])
        if cnt:
            if len(own):
                mine[1] = int(own[0])                   # u == v
            mine[2] = mine[0]                           # the same pair twice
        same += sum(int(obs[j] == probes[i]) for j in mine)
        col += mine
        ptr.append(len(col))
    ptr, col = np.asarray(ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    row = np.repeat(np.arange(len(probes)), np.diff(ptr))
    assert same > 0 and zrow != 2 and (np.diff(ptr) == 0).sum() == 1
    return ptr, obs[col].astype(np.int32), col, row


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_delta_parity_with_the_fp64_oracle(gpu, name, shape):
    from linkteller_amd import engine
    ref = _ref64(name, shape)
    _, _, probes, obs, zrow = _graph(name)
    zeros = float((ref == 0).mean())
    if name == "er":
        assert 0.1 <= zeros <= 0.9, zeros              # a condition of the zero check below, not a measurement
    base, _ = _baseline(name, shape, gpu)
    got = _rows(base, probes, obs)
    err = np.abs(got - ref).max() / ref.max()
    print(f"wide2 handle {name} {shape}: max {ref.max():.3g} zeros {zeros:.2f} |ours - ref64| / max = {err:.2e}")
    assert ref.max() > 0 and np.isfinite(got).all()
    assert err <= 1e-5
    assert np.all(got[ref == 0] == 0) and not np.signbit(got).any()
    assert np.all(ref[zrow] == 0) and np.all(got[zrow] == 0)      # the all-zero feature row: nothing to perturb
    torch.cuda.synchronize()
    engine.node_check()


# ---- 2. against the existing routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_against_the_slice_route(gpu, name, shape):
    from linkteller_amd import engine
    _, _, probes, obs, _ = _graph(name)
    hg, xt, dev = _tensors(name, shape, gpu)
    top = _ref64(name, shape).max()
    got = _rows(engine.Baseline2W(hg, xt, *dev), probes, obs)
    sl = _rows(engine.WideBaseline(hg, xt, *dev), probes, obs)
    print(f"wide2 handle {name} {shape}: |handle - slices| / max = {np.abs(got - sl).max() / top:.2e}")
    assert np.abs(got - sl).max() <= 2e-5 * top
    assert np.array_equal(got == 0, sl == 0)
    if shape == (20, 8):
        narrow = engine.Baseline(hg, xt, *dev).enable_fp64()
        assert engine.fused_shapes(*shape) and isinstance(engine.baseline_for(hg, xt, *dev), engine.Baseline)
        assert np.abs(got - _rows(narrow, probes, obs)).max() <= 2e-5 * top


# ---- 3. chunk invariance -------------------------------------------------------------------------------------------------------
def test_chunking_subsets_and_runs_give_the_same_bits(gpu):
    shape = (16, 41)
    _, _, probes, obs, _ = _graph("er")
    base, _ = _baseline("er", shape, gpu)
    lib = _lib.lib()
    one = base.influence_rows(probes, obs, DELTA, "delta").clone()
    assert torch.equal(base.influence_rows(probes, obs, DELTA, "delta"), one)                 # two runs
    need1 = lib.lt_influence2w_workspace_bytes(base._h, 1, len(obs))
    need_all = lib.lt_influence2w_workspace_bytes(base._h, len(probes), len(obs))
    assert need_all > 8 * need1                      # the default budget takes all the probes in one chunk
    try:
        for budget in (1, 2 * need1):
            _lib.set_tuning("chunk_budget_bytes", budget)
            need = lib.lt_influence2w_workspace_bytes(base._h, len(probes), len(obs))
            assert need < 4 * need1, (budget, need, need1)                                   # chunks of 1 .. 3 probes
            assert torch.equal(base.influence_rows(probes, obs, DELTA, "delta"), one), budget
    finally:
        _lib.set_tuning("chunk_budget_bytes", None)
    sel = np.array([9, 2, 24, 2, 17])
    assert torch.equal(base.influence_rows(probes[sel], obs, DELTA, "delta"), one[torch.from_numpy(sel).to(gpu)])
    cols = np.array([30, 1, 1, 12])
    assert torch.equal(base.influence_rows(probes, obs[cols], DELTA, "delta"), one[:, torch.from_numpy(cols).to(gpu)])


# ---- 4. list = rectangle --------------------------------------------------------------------------------------------------------
def _raw_pairs(base, pt, n_p, ptr, ot, n_m, mode, out, ws, ws_bytes=None):
    from linkteller_amd import engine
    return _lib.lib().lt_influence2w_pairs(base._h, pt.data_ptr(), n_p, None if ptr is None else ptr.ctypes.data, ot.data_ptr(), n_m,
                                           DELTA, mode, out.data_ptr(), ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                                           engine._stream())


@pytest.mark.parametrize("name", ("er", "hub"))
@pytest.mark.parametrize("shape", ((16, 41), (32, 121)), **_ids)
def test_pairs_are_the_bits_of_the_rectangle(gpu, name, shape):
    from linkteller_amd import engine
    lib = _lib.lib()
    _, _, probes, obs, zrow = _graph(name)
    ptr, pobs, col, row = _pairs(name)
    n_p, n_m = len(probes), len(pobs)
    base, _ = _baseline(name, shape, gpu)
    rect = base.influence_rows(probes, obs, DELTA, "delta")
    want = rect[torch.from_numpy(row).to(gpu), torch.from_numpy(col).to(gpu)]
    ref = _ref64(name, shape)[row, col]
    # a guard region behind out[n_pairs]
    buf = torch.full((n_m + 64,), -7.0, dtype=torch.float32, device=gpu)
    got = base.influence_pairs(probes, ptr, pobs, DELTA, "delta", out=buf[:n_m])
    assert got.data_ptr() == buf.data_ptr() and torch.equal(got, want) and bool((buf[n_m:] == -7.0).all())
    assert (want > 0).any() and bool((want[torch.from_numpy(row == zrow).to(gpu)] == 0).all())
    g64 = got.cpu().numpy().astype(np.float64)
    assert np.abs(g64 - ref).max() <= 1e-5 * _ref64(name, shape).max() and np.all(g64[ref == 0] == 0)
    assert torch.equal(base.influence_pairs(probes, ptr, pobs, DELTA), want)                 # two runs, the default mode
    # the workspace is sized by the list
    for p_, m_ in ((1, 1), (n_p, n_m), (25, 4 * base.n), (300, 1_000_000), (1024, 40_000)):
        need = lib.lt_influence2w_pairs_workspace_bytes(base._h, p_, m_)
        rows1 = lib.lt_influence2w_workspace_bytes(base._h, p_, 1)
        assert 0 < need <= rows1 + 4 * m_ + 8 * (p_ + 1) + 512, (p_, m_, need, rows1)
    need_all = lib.lt_influence2w_pairs_workspace_bytes(base._h, n_p, n_m)
    try:
        _lib.set_tuning("chunk_budget_bytes", 1)             # one probe per chunk: the probe without pairs is a chunk that owns none
        assert lib.lt_influence2w_pairs_workspace_bytes(base._h, n_p, n_m) < need_all
        assert torch.equal(base.influence_pairs(probes, ptr, pobs, DELTA, "delta"), want)
        assert torch.equal(base.influence_rows(probes, obs, DELTA, "delta"), rect)
    finally:
        _lib.set_tuning("chunk_budget_bytes", None)
    # pair_ptr that is no offset array: refused on the host, nothing written
    pt, ot = torch.from_numpy(probes).to(gpu), torch.from_numpy(pobs).to(gpu)
    ws = engine._workspace(need_all, gpu)
    out = torch.full((n_m,), -7.0, dtype=torch.float32, device=gpu)
    for wrong in (np.concatenate([[1], ptr[1:]]), np.concatenate([ptr[:3], [ptr[2] - 1], ptr[4:]]),
                  np.concatenate([ptr[:-1], [ptr[-1] + 1]]), np.concatenate([ptr[:-1], [ptr[-1] - 1]])):
        wrong = np.ascontiguousarray(wrong, dtype=np.int64)
        assert _raw_pairs(base, pt, n_p, wrong, ot, n_m, _lib.MODE_DELTA, out, ws) == LT_ERR_INVALID, wrong
        assert "pair_ptr" in lib.lt_last_error().decode()
    assert _raw_pairs(base, pt, n_p, None, ot, n_m, _lib.MODE_DELTA, out, ws) == LT_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert _raw_pairs(base, pt, n_p, ptr, ot, n_m, _lib.MODE_DELTA, out, ws) == 0 and torch.equal(out, want)
    torch.cuda.synchronize()
    engine.node_check()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def _raw_create(gpu, hg, xt, shape):
    h_, c = shape
    t = [torch.zeros(s, device=gpu) for s in ((F, h_), (h_,), (h_, c), (c,))]
    h = C.c_void_p()
    rc = _lib.lib().lt_baseline2w_create(hg.handle, xt.data_ptr(), F, F, t[0].data_ptr(), t[1].data_ptr(), h_, t[2].data_ptr(),
                                         t[3].data_ptr(), c, None, C.byref(h))
    return rc, h, _lib.lib().lt_last_error().decode()


def test_refusals(gpu):
    from linkteller_amd import engine, graph
    lib = _lib.lib()
    a_hat, x, probes, obs, _ = _graph("loops")
    ptr, pobs, col, row = _pairs("loops")
    n = a_hat.shape[0]
    hg, xt = graph.HipGraph(a_hat), torch.from_numpy(x).to(gpu)
    for shape in ((257, 41), (16, 257)):
        rc, h, msg = _raw_create(gpu, hg, xt, shape)
        assert rc == LT_ERR_UNSUPPORTED and not h.value and "lt_baseline2w_create" in msg
    rc, h, _ = _raw_create(gpu, hg, xt, (16, 256))
    assert rc == 0 and h.value
    assert lib.lt_baseline2w_destroy(h) == 0

    base, _ = _baseline("loops", (16, 41), gpu)
    pt, ot, lt_ = torch.from_numpy(probes).to(gpu), torch.from_numpy(obs).to(gpu), torch.from_numpy(pobs).to(gpu)
    npb, nob, n_m = len(probes), len(obs), len(pobs)
    need = lib.lt_influence2w_workspace_bytes(base._h, npb, nob)
    need_p = lib.lt_influence2w_pairs_workspace_bytes(base._h, npb, n_m)
    ws = engine._workspace(max(need, need_p), gpu)
    out = torch.full((npb, nob), 7.0, device=gpu)
    outp = torch.full((n_m,), 7.0, device=gpu)

    def call(mode, ws_bytes=None):
        return lib.lt_influence2w_rows(base._h, pt.data_ptr(), npb, ot.data_ptr(), nob, DELTA, mode, out.data_ptr(), nob,
                                       ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, engine._stream())
    for mode in (_lib.MODE_SPARSE, _lib.MODE_FULL):
        assert call(mode) == LT_ERR_UNSUPPORTED and "LT_MODE_DELTA only" in lib.lt_last_error().decode()
        assert _raw_pairs(base, pt, npb, ptr, lt_, n_m, mode, outp, ws) == LT_ERR_UNSUPPORTED
    for mode in ("sparse", "full"):
        with pytest.raises(NotImplementedError):
            base.influence_rows(probes, obs, DELTA, mode)
        with pytest.raises(NotImplementedError):
            base.influence_pairs(probes, ptr, pobs, DELTA, mode)
    assert call(_lib.MODE_DELTA, ws_bytes=need - 256) == LT_ERR_WORKSPACE
    assert _raw_pairs(base, pt, npb, ptr, lt_, n_m, _lib.MODE_DELTA, outp, ws, ws_bytes=need_p - 256) == LT_ERR_WORKSPACE
    # empty calls: LT_OK, nothing launched
    assert lib.lt_influence2w_rows(base._h, pt.data_ptr(), 0, ot.data_ptr(), nob, DELTA, _lib.MODE_DELTA, out.data_ptr(), nob,
                                   None, 0, None) == 0
    assert lib.lt_influence2w_rows(base._h, pt.data_ptr(), npb, ot.data_ptr(), 0, DELTA, _lib.MODE_DELTA, out.data_ptr(), 0,
                                   None, 0, None) == 0
    assert _raw_pairs(base, pt, npb, np.zeros(npb + 1, dtype=np.int64), lt_, 0, _lib.MODE_DELTA, outp, ws) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((outp == 7.0).all())          # nothing was enqueued by any of them
    assert call(_lib.MODE_DELTA) == 0
    torch.cuda.synchronize()
    good = out.clone()
    assert torch.equal(good, base.influence_rows(probes, obs, DELTA, "delta"))
    good_p = base.influence_pairs(probes, ptr, pobs, DELTA).clone()
    engine.node_check()
    # ids out of range: replaced on the device (no access out of bounds: the call completes), reported afterwards
    for which, bad in (("probe", n), ("observed", n), ("probe", -1), ("observed", -1), ("probe", 2 ** 31 - 1), ("observed", 2 ** 31 - 1)):
        p2, o2, l2 = probes.copy(), obs.copy(), pobs.copy()
        (p2 if which == "probe" else o2)[2] = bad
        (p2 if which == "probe" else l2)[2] = bad
        got = base.influence_rows(torch.from_numpy(p2).to(gpu), torch.from_numpy(o2).to(gpu), DELTA, "delta")
        torch.cuda.synchronize()
        assert torch.isfinite(got).all()
        with pytest.raises(IndexError):
            engine.node_check()
        engine.node_check()
        got = base.influence_pairs(torch.from_numpy(p2).to(gpu), ptr, torch.from_numpy(l2).to(gpu), DELTA)
        torch.cuda.synchronize()
        assert torch.isfinite(got).all()
        with pytest.raises(IndexError):
            engine.node_check()
        engine.node_check()
    assert torch.equal(base.influence_rows(pt, ot, DELTA, "delta"), good)
    assert torch.equal(base.influence_pairs(pt, ptr, lt_, DELTA), good_p)
    torch.cuda.synchronize()
    engine.node_check()


# ---- 6. logits and refresh ------------------------------------------------------------------------------------------------------
def _hip():
    """The HIP runtime torch itself loaded (hipMemcpy: a write torch's version counter does not see)."""
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    lib = C.CDLL(path if os.path.exists(path) else "libamdhip64.so")
    lib.hipMemcpy.restype = C.c_int
    return lib


@pytest.mark.parametrize("shape", [(18, 9), (32, 121)], **_ids)
def test_logits_and_refresh(gpu, shape):
    from linkteller_amd import engine
    from oracle import linkteller_oracle as O
    a_hat, x, probes, obs, _ = _graph("er")
    hg, xt, dev = _tensors("er", shape, gpu)
    base = engine.Baseline2W(hg, xt, *dev)

    def ref_logits(p, feats=x):
        return O.gcn_forward(torch.from_numpy(feats).double(), O.to_torch_sparse(a_hat).double(),
                             {k: torch.from_numpy(np.asarray(v)).double() for k, v in p.items()}).numpy()

    def fresh():
        f = engine.Baseline2W(hg, xt.clone(), *[t.clone() for t in dev])
        return f.logits(), f.influence_rows(probes, obs, DELTA, "delta")
    ref = ref_logits(_params(shape))
    got = base.logits().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6      # test_gpu_parity's bound
    before = _rows(base, probes, obs)
    # an in-place update of every parameter + refresh(): logits and rows follow the new weights
    new = _params(shape, seed=1)
    with torch.no_grad():
        for t, k in zip(dev, KEYS):
            t.copy_(torch.from_numpy(new[k]))
    base.refresh()
    ref2 = ref_logits(new)
    lg, rw = base.logits(), base.influence_rows(probes, obs, DELTA, "delta").clone()
    assert np.abs(lg.cpu().numpy().astype(np.float64) - ref2).max() <= 2e-5 * np.abs(ref2).max() + 1e-6
    rows_ref = _oracle(a_hat, x, new, probes, obs)
    after = rw.cpu().numpy().astype(np.float64)
    assert np.abs(after - rows_ref).max() <= 1e-5 * rows_ref.max() and np.all(after[rows_ref == 0] == 0)
    assert np.abs(after - before).max() > 1e-3 * rows_ref.max()
    f_lg, f_rw = fresh()
    assert torch.equal(lg, f_lg) and torch.equal(rw, f_rw)
    # a feature row edited in place through torch: refresh() sees the version counter
    row = int(probes[5])
    with torch.no_grad():
        xt[row] = xt[row] * 1.5 + 0.25
    base.refresh("delta")
    lg3, rw3 = base.logits(), base.influence_rows(probes, obs, DELTA, "delta").clone()
    f_lg, f_rw = fresh()
    assert torch.equal(lg3, f_lg) and torch.equal(rw3, f_rw) and not torch.equal(rw3, rw)
    x3 = xt.cpu().numpy()
    rows_ref3 = _oracle(a_hat, x3, new, probes, obs)
    assert np.abs(rw3.cpu().numpy().astype(np.float64) - rows_ref3).max() <= 1e-5 * rows_ref3.max()
    # the same kind of edit behind torch's back (a raw copy): announced with features_changed()
    word = torch.tensor([4.0], dtype=torch.float32)
    torch.cuda.synchronize()
    assert _hip().hipMemcpy(C.c_void_p(xt.data_ptr() + 4 * (row * F + 17)), C.c_void_p(word.data_ptr()), C.c_size_t(4), 1) == 0
    version = xt._version
    assert base.features_changed() is base
    assert xt._version == version and float(xt[row, 17]) == 4.0
    lg4, rw4 = base.logits(), base.influence_rows(probes, obs, DELTA, "delta").clone()
    f_lg, f_rw = fresh()
    assert torch.equal(lg4, f_lg) and torch.equal(rw4, f_rw) and not torch.equal(rw4, rw3)
    torch.cuda.synchronize()
    engine.node_check()


# ---- 7. attacker ---------------------------------------------------------------------------------------------------------------
def test_attacker_takes_the_handle(gpu, tmp_path, monkeypatch):
    from linkteller_amd import engine, graph
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN
    from oracle import linkteller_oracle as O
    g = np.load(os.path.join(GOLDEN, "next_rows.npz"), allow_pickle=False)
    a = csr_from(g, "adj")
    x = torch.from_numpy(g["x"]).to(gpu)
    adj_t = graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(a)).to(gpu)
    w = types.SimpleNamespace(features_2=x, adj_2=adj_t, adj_ori=a, n_nodes=a.shape[0])
    torch.manual_seed(7)
    model = GCN(x.shape[1], 16, 41, 0.5).to(gpu).eval()
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("LT_INFLUENCE_MODE", raising=False)
    monkeypatch.setenv("LT_WIDE2", "handle")
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=32, sample_seed=42, influence=DELTA,
                              mode="vanilla-clean", attack_mode="efficient")
    atk = Attacker(args, model, w)
    atk.prepare_test_data()
    assert atk._walk()[0] == "gcn2"
    nodes = np.asarray(atk.test_nodes, dtype=np.int64)
    mat = atk.influence_matrix()
    assert isinstance(atk._baseline, engine.Baseline2W)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    src = [sd[f"gc{i}.{p}"] for i in (1, 2) for p in ("weight", "bias")]
    own = engine.Baseline2W(atk.adj, atk.features, *src)
    want = own.influence_rows(nodes, nodes, DELTA, "delta").cpu().numpy().astype(np.float64)
    assert mat.dtype == np.float64 and np.array_equal(mat, want) and mat.max() > 0
    assert np.array_equal(atk.influence_matrix("delta"), mat)
    # the fp64 oracle on the same model
    P = {k: t.double().cpu() for k, t in zip(KEYS, src)}
    ref = O.influence_matrix(x.double().cpu(), O.to_torch_sparse(O.first_order_gcn(a)).double(), P, nodes, DELTA)
    assert np.abs(mat - ref).max() <= 1e-5 * ref.max() and np.all(mat[ref == 0] == 0)
    # evaluate(): the metrics of the matrix's cells
    ind = {int(v): i for i, v in enumerate(nodes)}

    def cells(pairs):       # perturb v, observe u (attacker.py:236-245)
        return [mat[ind[int(v)], ind[int(u)]] for u, v in np.asarray(pairs).reshape(-1, 2)]
    m = O.attack_metrics(cells(atk.exist_edges), cells(atk.nonexist_edges))
    out = atk.evaluate()
    assert abs(out["auc"] - m["auc"]) <= 1e-4 and abs(out["ap"] - m["ap"]) <= 1e-4
    # pair_scores on a shuffled pair list: the matrix's cells, through the list
    def no_rect(*a_, **k_):
        raise AssertionError("the rectangle route was taken")
    monkeypatch.setattr(Attacker, "_pair_scores_rect", no_rect)
    rng = np.random.RandomState(0)
    pi, oi = rng.randint(0, len(nodes), 200), rng.randint(0, len(nodes), 200)
    assert np.array_equal(atk.pair_scores(nodes[pi], nodes[oi]), mat[pi, oi])
    # the naive attack writes its file through the list as well
    atk.link_prediction_attack()
    name = os.path.join("eval_twitch/ES/RU", "unbalanced_32_42.pt")
    assert atk.naive_result_filename() == name and os.path.exists(name)
    saved = torch.load(name, weights_only=False)
    assert np.array_equal(np.asarray(saved["result"]["pred"]), np.asarray(cells(atk.exist_edges) + cells(atk.nonexist_edges)))
    assert isinstance(atk._baseline, engine.Baseline2W)
    monkeypatch.undo()
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("LT_INFLUENCE_MODE", raising=False)
    # `sparse` / `full` stay the slices, with their bits
    slices = engine.WideBaseline(atk.adj, atk.features, *src)
    sp_bits = slices.influence_rows(nodes, nodes, DELTA, "sparse").cpu().numpy().astype(np.float64)
    assert np.array_equal(atk.influence_matrix("sparse"), sp_bits) and isinstance(atk._baseline, engine.WideBaseline)
    monkeypatch.setenv("LT_WIDE2", "handle")
    assert np.array_equal(atk.influence_matrix(), mat) and isinstance(atk._baseline, engine.Baseline2W)      # ... and back
    monkeypatch.setenv("LT_INFLUENCE_MODE", "sparse")
    assert np.array_equal(atk.influence_matrix(), sp_bits) and isinstance(atk._baseline, engine.WideBaseline)
    monkeypatch.delenv("LT_INFLUENCE_MODE")
    # LT_WIDE2=slices keeps the slice route in `delta` too
    monkeypatch.setenv("LT_WIDE2", "slices")
    dl_bits = slices.influence_rows(nodes, nodes, DELTA, "delta").cpu().numpy().astype(np.float64)
    assert np.array_equal(atk.influence_matrix(), dl_bits) and isinstance(atk._baseline, engine.WideBaseline)
    assert np.abs(dl_bits - mat).max() <= 2e-5 * ref.max()

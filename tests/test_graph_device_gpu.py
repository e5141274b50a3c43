"""lt_graph_create_device against lt_graph_create: the host builder is the checker.  Every table the device builder produces
(read back with lt_graph_table) equals the host builder's word for word, on graphs chosen at the sizes where either builder
changes its path; the transpose also equals a scipy restatement, so the two builders do not only agree with each other.  Then:
the refusals of the host builder with the same messages, the same bits from every consumer of a graph, and the Python routes
(`HipGraph.from_device_csr`, `from_torch_sparse` on a CUDA tensor, `LT_GRAPH_BUILD`)."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import boundary_cases as B
import train_cases as K

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def build_mode(mode):
    old = os.environ.get("LT_GRAPH_BUILD")
    os.environ["LT_GRAPH_BUILD"] = mode
    try:
        yield
    finally:
        if old is None:
            del os.environ["LT_GRAPH_BUILD"]
        else:
            os.environ["LT_GRAPH_BUILD"] = old


def device_csr(mat, dev):
    import torch
    from linkteller_amd import graph
    _, rowptr, col, val = graph.csr_arrays(mat)
    return tuple(torch.from_numpy(a).to(dev) for a in (rowptr, col, val))


def both(mat, dev):
    """(host-built, device-built) graphs of the same canonical CSR."""
    from linkteller_amd import graph
    with build_mode("host"):
        gh = graph.HipGraph(mat)
    gd = graph.HipGraph.from_device_csr(*device_csr(mat, dev))
    assert gh.built_on == "host" and gd.built_on == "device"
    return gh, gd


def assert_same_tables(gh, gd):
    from linkteller_amd import _lib
    for name in _lib.GRAPH_TABLES:
        a, b = gh.table(name), gd.table(name)
        assert a.shape == b.shape, f"{name}: {a.shape} on the host builder, {b.shape} on the device builder"
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name} differs at {np.flatnonzero(a != b)[:8]}"
    assert gh.scalars() == gd.scalars()


def assert_scipy_transpose(g, mat):
    """tptr / trow / tval / tpos against tocsc() with sorted indices; the positions from rowptr."""
    from linkteller_amd import graph
    n, rowptr, col, val = graph.csr_arrays(mat)
    a = sp.csr_matrix((val, col, rowptr), shape=(n, n))
    pos = sp.csr_matrix((np.arange(len(col), dtype=np.float64) - np.repeat(rowptr[:-1], np.diff(rowptr)), col, rowptr), shape=(n, n))
    csc, pcsc = a.tocsc(), pos.tocsc()
    csc.sort_indices()
    pcsc.sort_indices()
    assert csc.nnz == len(col)                      # (explicit zeros are kept)
    assert np.array_equal(g.table("tptr"), csc.indptr.astype(np.int32))
    assert np.array_equal(g.table("trow"), csc.indices.astype(np.int32))
    assert np.array_equal(g.table("tval").view(np.int32), csc.data.astype(np.float32).view(np.int32))
    if n <= 65534:
        assert np.array_equal(g.table("tpos")[:len(col)], pcsc.data.astype(np.int32))
        assert not g.table("tpos")[len(col):].any()
    else:
        assert g.table("tpos").size == 0


@functools.lru_cache(maxsize=None)
def er_graph():
    from linkteller_amd import graph, synth
    return graph.first_order_gcn(synth.erdos_renyi_graph(1301, 1301 * 4, seed=3))


def skewed_graph(n):
    """Out-degree 2; column 0 holds 40 000 entries (longer than one block sorts), the other columns follow n u^3 (skewed in-degrees:
    hot_frac is not the uniform value)."""
    rng = np.random.RandomState(n)
    rows = np.arange(n)
    first = np.where(rows < 40000, 0, 1 + (rng.uniform(size=n) ** 3 * (n - 1)).astype(np.int64))
    second = 1 + (rng.uniform(size=n) ** 3 * (n - 1)).astype(np.int64)
    second = np.where(second == first, (second % (n - 1)) + 1, second)
    second = np.where(second == first, (second % (n - 1)) + 1, second)
    assert (first != second).all()
    a = sp.csr_matrix((rng.uniform(0.1, 1.0, 2 * n), (np.repeat(rows, 2), np.stack([first, second], 1).ravel())), shape=(n, n))
    a.sort_indices()
    assert a.nnz == 2 * n and np.diff(a.indptr).max() == 2 and np.diff(a.tocsc().indptr).max() == 40000
    return a


def explicit_zero_graph():
    a = K.directed_graph(257, 4).tocsr()
    a.data[::3] = 0.0
    assert a.nnz == len(a.data) and (a.data == 0).sum() > 100
    return a


def graph_cases():
    return {
        "er_1301": er_graph,
        "directed_513": lambda: K.directed_graph(513, 0),
        "short_ladder": lambda: B.short_ladder().a,
        "hub_ladder": lambda: B.hub_ladder().a,
        "at_cap_4096": lambda: B.short_ladder_at(B.LT_DL_MAX_T).a,
        "past_cap_4097": lambda: B.short_ladder_at(B.LT_DL_MAX_T + 1).a,
        "one_node": lambda: sp.csr_matrix((1, 1), dtype=np.float32),
        "one_node_loop": lambda: sp.csr_matrix(np.array([[0.75]], dtype=np.float32)),
        "no_entries": lambda: sp.csr_matrix((37, 37), dtype=np.float32),
        "explicit_zeros": explicit_zero_graph,
        "n_65534": lambda: skewed_graph(65534),
        "n_65535": lambda: skewed_graph(65535),
    }


# what each case must have: (records, tpos, long rows)
EXPECT = {"er_1301": (True, True, False), "directed_513": (True, True, False), "short_ladder": (True, True, False),
          "hub_ladder": (False, True, True), "at_cap_4096": (True, True, False), "past_cap_4097": (False, True, False),
          "one_node": (True, True, False), "one_node_loop": (True, True, False), "no_entries": (True, True, False),
          "explicit_zeros": (True, True, False), "n_65534": (False, True, False), "n_65535": (False, False, False)}


@pytest.mark.parametrize("name", list(EXPECT))
def test_tables_word_for_word(gpu, name):
    mat = graph_cases()[name]()
    gh, gd = both(mat, gpu)
    assert_same_tables(gh, gd)
    assert_scipy_transpose(gd, mat)
    s = gd.scalars()
    records, tpos, long_rows = EXPECT[name]
    assert (s["has_records"], s["has_tpos"], s["p_n_long"] > 0) == (records, tpos, long_rows), s
    if name == "at_cap_4096":
        assert s["dl_max_t"] == B.LT_DL_MAX_T
    if name == "short_ladder":
        assert s["dl_max_t"] == 4050
    if name.startswith("n_6"):
        assert s["max_col_nnz"] == 40000 and 0.2 < s["hot_frac"] < 1.0
        assert s["hot_frac"] != pytest.approx(16384 / s["n"], rel=0.2)        # not the uniform value
    if records:
        meta = gd.table("dl_meta").reshape(-1, 4)
        assert gd.table("dl_rec").size == meta[-1, 0] + 2 * meta[-1, 1:].sum() + 4


def test_records_against_the_host_restatement(gpu):
    """The device builder's records equal lt_graph_records_host's, the function tests/test_records.py pins against numpy."""
    from linkteller_amd import _lib
    g = B.short_ladder()
    n, nnz, rowptr, col, val = B.csr32(g)
    meta = np.zeros((n, 4), dtype=np.int32)
    words = C.c_int64()
    h = _lib.lib()
    assert h.lt_graph_records_host(n, nnz, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, meta.ctypes.data, None, 0, C.byref(words)) == 0
    rec = np.zeros(words.value, dtype=np.int32)
    assert h.lt_graph_records_host(n, nnz, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, meta.ctypes.data, rec.ctypes.data,
                                   rec.size, C.byref(words)) == 0
    from linkteller_amd import graph
    gd = graph.HipGraph.from_device_csr(*device_csr(g.a, gpu))
    assert np.array_equal(gd.table("dl_meta").reshape(-1, 4), meta)
    assert np.array_equal(gd.table("dl_rec")[:-4], rec) and not gd.table("dl_rec")[-4:].any()


def test_refusals(gpu):
    import torch
    from linkteller_amd import _lib
    h = _lib.lib()
    out = C.c_void_p()

    def create(n, rowptr, col, val):
        rp = torch.as_tensor(np.asarray(rowptr, dtype=np.int32)).to(gpu)
        ci = torch.as_tensor(np.asarray(col, dtype=np.int32)).to(gpu)
        va = torch.as_tensor(np.asarray(val, dtype=np.float32)).to(gpu)
        rc = h.lt_graph_create_device(n, len(col), rp.data_ptr(), ci.data_ptr() if len(col) else None,
                                      va.data_ptr() if len(col) else None, None, C.byref(out))
        assert rc != 0 and out.value is None
        return rc, h.lt_last_error()

    rc, msg = create(2, [1, 1, 2], [0, 1], [1, 1])
    assert rc == -1 and b"rowptr[0]" in msg
    assert create(2, [0, 2, 1], [0], [1])[0] == -1
    rc, msg = create(2, [0, 1, 2], [0, 5], [1, 1])
    assert rc == -1 and b"column 5 out of range at row 1" in msg
    rc, msg = create(2, [0, 2, 2], [1, 0], [1, 1])
    assert rc == -1 and b"columns of row 0 are not strictly increasing" in msg
    rc, msg = create(2, [0, 2, 2], [1, 1], [1, 1])       # duplicate column
    assert rc == -1 and b"strictly increasing" in msg
    assert h.lt_graph_create_device(2, 0, None, None, None, None, C.byref(out)) == -1
    rp = torch.as_tensor(np.array([0, 1, 1, 1], dtype=np.int32)).to(gpu)
    two = torch.zeros(2, dtype=torch.int32, device=gpu)
    assert h.lt_graph_create_device(3, 2, rp.data_ptr(), two.data_ptr(), two.float().data_ptr(), None, C.byref(out)) == -1
    assert b"rowptr[n]=1 != nnz=2" in h.lt_last_error()
    # the first offending row, as a single pass reports it: a bad column in row 5 lies in front of a bad offset at row 9 ...
    n, deg = 16, 3
    rp = (np.arange(n + 1) * deg).astype(np.int32)
    ci = np.tile(np.arange(deg, dtype=np.int32), n)
    va = np.ones(n * deg, dtype=np.float32)
    rp2, ci2 = rp.copy(), ci.copy()
    rp2[10] = 2
    ci2[5 * deg + 1] = 99
    ci2[7 * deg + 2] = 0
    rc, msg = create(n, rp2, ci2, va)
    assert rc == -1 and b"column 99 out of range at row 5" in msg
    ci2[5 * deg + 1] = 1
    rc, msg = create(n, rp2, ci2, va)
    assert rc == -1 and b"columns of row 7 are not strictly increasing" in msg
    # ... and behind it when the bad offset comes first (nothing is read through row 9's offsets)
    ci2[7 * deg + 2] = 2
    ci2[12 * deg] = -4
    rc, msg = create(n, rp2, ci2, va)
    assert rc == -1 and b"rowptr not monotone at row 9" in msg
    # a bad offset late in a rowptr of 2^17 rows: refused from the host copy of rowptr, no kernel reads through it
    n, deg = 1 << 17, 8
    rp = (np.arange(n + 1, dtype=np.int64) * deg).astype(np.int32)
    ci = np.tile(np.arange(deg, dtype=np.int32), n)
    va = np.ones(n * deg, dtype=np.float32)
    for row, bad in ((n - 5, -7), (n // 2 + 3, 2 ** 31 - 1), (3 * n // 4, 11)):
        rp2 = rp.copy()
        rp2[row] = bad
        rc, msg = create(n, rp2, ci, va)
        assert rc == -1 and f"rowptr not monotone at row {row - 1}".encode() in msg
    torch.cuda.synchronize()                             # the device is healthy: no refusal dereferenced anything
    assert h.lt_graph_table(None, 0, None, 0, None) == -1
    gh, gd = both(sp.csr_matrix((va, ci, rp), shape=(n, n)), gpu)       # and a good graph builds right after
    assert_same_tables(gh, gd)


@functools.lru_cache(maxsize=None)
def model():
    from linkteller_amd import synth
    a = er_graph()
    x = synth.gaussian_features(a.shape[0], 48, seed=2)
    w = synth.gcn_weights(48, 24, 3, seed=9)
    nodes = np.random.RandomState(4).choice(a.shape[0], 40, replace=False)
    return x, w, nodes


def test_same_bits_downstream(gpu):
    """Every consumer of a graph gives the same bits on the device-built graph as on the host-built one."""
    import torch
    from linkteller_amd import engine
    x_np, w_np, nodes = model()
    results = []
    for g in both(er_graph(), gpu):
        x = torch.from_numpy(x_np).to(gpu)
        w = [torch.from_numpy(w_np[k]).to(gpu) for k in ("W1", "b1", "W2", "b2")]
        out = {}
        dense = torch.from_numpy(np.random.RandomState(6).standard_normal((g.n, 64)).astype(np.float32)).to(gpu)
        out["spmm"] = engine.spmm(g, dense).cpu().numpy()
        out["forward"] = engine.gcn2_forward(g, x, *w).cpu().numpy()
        base = engine.Baseline(g, x, *w)
        for mode in ("delta", "sparse", "full"):
            out[mode] = base.influence_rows(nodes, nodes, 1e-4, mode).cpu().numpy()
        out["host_matrix"] = base.influence_matrix_host(nodes, nodes, 1e-4, "delta")
        stats = base.host_landing_stats()                  # (post_ns is a time: not a result)
        out["landing"] = np.array([stats["early"] + stats["late"], stats["mismatch"]])
        y = torch.from_numpy(np.random.RandomState(1).randint(0, 3, g.n).astype(np.int64)).to(gpu)
        tr = engine.GCN2Trainer(g, x, y, *[t.clone() for t in w], lr=0.01, weight_decay=5e-4, dropout=0.5, seed=7)
        loss, correct = tr.run(1)
        out["loss"], out["correct"] = loss, correct
        for i, t in enumerate(tr.params):
            out[f"param{i}"] = t.cpu().numpy()
        for i, t in enumerate(tr.grads()):
            out[f"grad{i}"] = t.cpu().numpy()
        results.append(out)
    host, dev = results
    for key in host:
        assert np.array_equal(host[key], dev[key]), key
    assert host["delta"].any() and host["full"].any() and host["spmm"].any()


def test_python_routes(gpu, monkeypatch):
    import torch
    from linkteller_amd import graph
    monkeypatch.delenv("LT_GRAPH_BUILD", raising=False)
    a = er_graph()
    with build_mode("host"):
        want = graph.HipGraph(a)
    coo = a.tocoo()
    idx = torch.from_numpy(np.vstack((coo.row, coo.col)).astype(np.int64)).to(gpu)
    vals = torch.from_numpy(coo.data.astype(np.float32)).to(gpu)
    # a shuffled, uncoalesced CUDA COO tensor without duplicates builds on the device
    perm = torch.from_numpy(np.random.RandomState(0).permutation(coo.nnz)).to(gpu)
    t = torch.sparse_coo_tensor(idx[:, perm], vals[perm], a.shape)
    g = graph.as_hip_graph(t)
    assert g.built_on == "device"
    assert_same_tables(want, g)
    assert graph.as_hip_graph(t) is g                       # the cache is unchanged
    # one entry split into two duplicates: the host route sums them as the reference does
    half = vals.clone()
    half[5] = half[5] / 2
    t2 = torch.sparse_coo_tensor(torch.cat([idx, idx[:, 5:6]], 1), torch.cat([half, half[5:6]]), a.shape)
    g2 = graph.HipGraph.from_torch_sparse(t2)
    assert g2.built_on == "host"
    assert_same_tables(want, g2)
    with build_mode("host"):
        assert graph.HipGraph.from_torch_sparse(t).built_on == "host"
    with build_mode("device"):
        g3 = graph.HipGraph(a)
        assert g3.built_on == "device"
        assert_same_tables(want, g3)
        assert graph.HipGraph.from_torch_sparse(t.cpu()).built_on == "device"
    assert graph.HipGraph(a).built_on == "host" and graph.HipGraph.from_torch_sparse(t.cpu()).built_on == "host"      # auto
    with build_mode("nonsense"), pytest.raises(ValueError):
        graph.HipGraph(a)
    # the ValueErrors of csr_arrays
    with pytest.raises(ValueError, match="square"):
        graph.HipGraph.from_torch_sparse(torch.sparse_coo_tensor(idx[:, :4], vals[:4], (a.shape[0], a.shape[0] + 1)))
    # from_device_csr takes int32 / int32 / float32 CUDA tensors only
    rowptr, col, val = device_csr(a, gpu)
    for bad in ((rowptr.long(), col, val), (rowptr, col.long(), val), (rowptr, col, val.double()), (rowptr.cpu(), col, val),
                (rowptr, col.cpu(), val), (rowptr, col, val.cpu())):
        with pytest.raises((TypeError, ValueError)):
            graph.HipGraph.from_device_csr(*bad)
    with pytest.raises(ValueError):
        graph.HipGraph.from_device_csr(rowptr, col, val[:-1])

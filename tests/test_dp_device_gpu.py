"""The device route of the DP graphs on the GPU: lt_sym_csr_from_cells and lt_normalize_csr against their numpy restatements
(dp_device_restate.py, which test_dp_device_cpu.py holds against scipy and the host normalisers), at the sizes where the kernels
change course, and the route through dp.perturb_adj_device, HipGraph.from_device_pattern and Worker against the host philox route.
Every comparison is np.array_equal."""
import argparse
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import dp_device_restate as D
from conftest import csr_from, load_golden

pytestmark = pytest.mark.gpu

GUARD32 = 0x5A5A5A5A
SEED_WIDE = (5 << 32) | 1234


def _t(a, gpu, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:                                            # a pointer even for nothing
        return torch.zeros(1, dtype=torch.from_numpy(a).dtype, device=gpu)
    return torch.from_numpy(a).to(gpu)


def _sym(gpu, n, cells, coins=None, base=None, capacity=None):
    """lt_sym_csr_from_cells through the C ABI with 8 guard words behind out_col: (rowptr, col [min(nnz, capacity)], info,
    the guard words)."""
    import torch
    from linkteller_amd import _lib
    h = _lib.lib()
    cells = np.asarray(cells, dtype=np.int64)
    m = int(cells.size)
    d_cells = _t(cells, gpu, np.int64)
    d_coins = None if coins is None else _t(coins, gpu, np.uint8)
    b_nnz = 0 if base is None else int(base[0][-1])
    d_brp = None if base is None else _t(base[0], gpu, np.int32)
    d_bcol = None if base is None else _t(base[1], gpu, np.int32)
    cap = b_nnz + 2 * m if capacity is None else capacity
    need = h.lt_sym_csr_workspace_bytes(n, b_nnz, m)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    rowptr = torch.full((n + 1,), -7, dtype=torch.int32, device=gpu)
    col = torch.full((cap + 8,), GUARD32, dtype=torch.int32, device=gpu)
    info = torch.full((4,), -1, dtype=torch.int64, device=gpu)
    _lib.check(h.lt_sym_csr_from_cells(n, d_brp.data_ptr() if base is not None else None, d_bcol.data_ptr() if base is not None else None,
                                       b_nnz, d_cells.data_ptr(), d_coins.data_ptr() if d_coins is not None else None, m,
                                       rowptr.data_ptr(), col.data_ptr(), cap, info.data_ptr(), ws.data_ptr(), ws.numel(),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lt_sym_csr_from_cells")
    info = info.cpu().numpy()
    col = col.cpu().numpy()
    return rowptr.cpu().numpy(), col[:min(int(info[0]), cap)], info, col[cap:]


def _check_sym(gpu, n, cells, coins=None, base=None):
    want_rowptr, want_col, want_info = D.sym_csr_from_cells(n, cells, coins, base)
    rowptr, col, info, guard = _sym(gpu, n, cells, coins, base)
    assert info.tolist() == want_info.tolist()
    assert rowptr.dtype == np.int32 and np.array_equal(rowptr, want_rowptr)
    assert np.array_equal(col, want_col)
    assert np.all(guard == GUARD32)
    return rowptr, col


def _cells(n, m, seed, coins=False):
    """m distinct strict-lower cells of an n x n matrix as flat indices i * n + j, in a shuffled order."""
    rng = np.random.RandomState(seed)
    total = n * (n - 1) // 2
    if total <= 4 * m:
        t = rng.permutation(total)[:m].astype(np.int64)
    else:
        t = np.unique(rng.randint(0, total, size=2 * m + 64).astype(np.int64))
        assert t.size >= m
        t = rng.permutation(t)[:m]
    import dp_philox_restate as R
    flat = R.flat_index(t, n)
    return (flat, rng.randint(0, 2, size=m).astype(np.uint8)) if coins else flat


def _base(a):
    a = sp.csr_matrix(a)
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32)


# ---- lt_sym_csr_from_cells ---------------------------------------------------------------------------------------------------

def test_sym_smallest_graphs(gpu):
    _check_sym(gpu, 2, [2])                                                     # the single cell (1, 0)
    _check_sym(gpu, 2, [2], coins=[0])                                          # cleared: the empty graph
    _check_sym(gpu, 3, [3, 7])                                                  # (1, 0), (2, 1)
    _check_sym(gpu, 3, [7, 6, 3], coins=[1, 0, 1])
    path = sp.csr_matrix(np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]]))
    _check_sym(gpu, 3, [6, 3], coins=[1, 0], base=_base(path))                  # sets (2, 0), clears (1, 0)


def test_sym_without_cells(gpu):
    a = D.hub_graph(65, 3, hub=64, isolated=0, self_loop=7)
    rowptr, col = _check_sym(gpu, 65, [], base=_base(a))                         # m == 0 with a base: a copy
    assert np.array_equal(rowptr, a.indptr) and np.array_equal(col, a.indices)
    rowptr, col = _check_sym(gpu, 65, [])                                        # m == 0 without one: the empty graph
    assert not rowptr.any() and col.size == 0
    _check_sym(gpu, 65, [], coins=[])


def test_sym_set_clear_and_emptied_rows(gpu):
    """A cell that sets an existing edge, a cell that clears a non-edge, a row whose every entry is cleared, and a diagonal
    entry of the base that passes through."""
    n = 9
    pairs = [(1, 0), (4, 0), (4, 2), (4, 3), (7, 4), (8, 6)]
    i, j = np.array(pairs).T
    a = sp.coo_matrix((np.ones(len(pairs), dtype=np.int64), (i, j)), shape=(n, n)).tocsr()
    a = sp.lil_matrix(a + a.T)
    a[5, 5] = 1                                                                  # row 5: the diagonal only
    a[4, 4] = 1
    a = sp.csr_matrix(a)
    cells = np.array([4 * n + 0, 4 * n + 2, 4 * n + 3, 7 * n + 4,                 # every off-diagonal entry of row 4, cleared
                      1 * n + 0,                                                 # sets an existing edge
                      6 * n + 2,                                                 # clears a non-edge
                      8 * n + 6, 3 * n + 1], dtype=np.int64)                     # clears row 8 entirely; a new edge
    coins = np.array([0, 0, 0, 0, 1, 0, 0, 1], dtype=np.uint8)
    rowptr, col = _check_sym(gpu, n, cells, coins, _base(a))
    assert col[rowptr[4]:rowptr[5]].tolist() == [4] and rowptr[8] == rowptr[9] and col[rowptr[5]:rowptr[6]].tolist() == [5]
    assert col[rowptr[1]:rowptr[2]].tolist() == [0, 3] and rowptr[6] == rowptr[7]


@pytest.mark.parametrize("n", [257, 1025])
def test_sym_at_block_edges(gpu, n):
    """n + 1 rows one past a multiple of the 256-thread blocks; with and without a base."""
    flat, coin = _cells(n, 3 * n, seed=n, coins=True)
    _check_sym(gpu, n, flat)
    _check_sym(gpu, n, flat, coin, _base(D.hub_graph(n, n + 1, hub=n - 1, self_loop=n // 2, isolated=1)))


def test_sym_hub_row(gpu):
    """A base row of 1500 columns merged with 600 listed cells of that row (sets and clears on both sides of the diagonal)."""
    n, hub = 1800, 900
    rng = np.random.RandomState(11)
    others = np.setdiff1d(np.arange(n), [hub])
    nb = rng.permutation(others)[:1500]
    a = sp.coo_matrix((np.ones(1500, dtype=np.int64), (np.full(1500, hub), nb)), shape=(n, n)).tocsr()
    a = sp.csr_matrix(a + a.T)
    assert np.diff(a.indptr)[hub] == 1500
    touched = np.concatenate([rng.permutation(nb)[:400], np.setdiff1d(others, nb)[:200]])      # 400 edges, 200 non-edges
    i, j = np.maximum(touched, hub), np.minimum(touched, hub)
    cells = rng.permutation(i.astype(np.int64) * n + j)
    coins = rng.randint(0, 2, size=600).astype(np.uint8)
    extra, extra_coin = _cells(n, 300, seed=12, coins=True)                      # and cells elsewhere
    keep = ~np.isin(extra, cells)
    rowptr, col = _check_sym(gpu, n, np.concatenate([cells, extra[keep]]), np.concatenate([coins, extra_coin[keep]]), _base(a))
    assert rowptr[hub + 1] - rowptr[hub] > 1000


@pytest.mark.parametrize("m", [255, 256, 257, 65537])
def test_sym_at_radix_block_edges(gpu, m):
    """2 m directed entries around the 256-entry groups of the sort, and past the 4 x 256 entries of a one-round block."""
    n = 1500
    flat, coin = _cells(n, m, seed=m, coins=True)
    _check_sym(gpu, n, flat)
    _check_sym(gpu, n, flat, coin, _base(D.hub_graph(n, 5, hub=3)))


def test_sym_flat_indices_beyond_32_bits(gpu):
    n = 70000
    rng = np.random.RandomState(4)
    i = rng.randint(n - 3000, n, size=5000).astype(np.int64)                     # i * n + j > 2^32 for every cell
    j = rng.randint(0, n - 3000, size=5000).astype(np.int64)
    flat = np.unique(i * n + j)
    flat = np.concatenate([flat, [np.int64(n - 1) * n + (n - 2), np.int64(1) * n + 0]])      # the last and the first cell
    assert flat.min() == n and flat.max() > 2 ** 32 and np.sort(flat)[1] > 2 ** 32
    rowptr, col = _check_sym(gpu, n, rng.permutation(flat))
    assert col.size == 2 * flat.size


def test_sym_is_a_function_of_the_cell_set(gpu):
    n = 1025
    flat, coin = _cells(n, 4000, seed=9, coins=True)
    base = _base(D.hub_graph(n, 6, hub=512))
    order = np.argsort(flat)
    perm = np.random.RandomState(1).permutation(flat.size)
    runs = [_sym(gpu, n, flat[o], coin[o], base) for o in (order, order[::-1], perm, perm)]
    for rowptr, col, info, _ in runs[1:]:
        assert rowptr.tobytes() == runs[0][0].tobytes() and col.tobytes() == runs[0][1].tobytes() and info.tolist() == runs[0][2].tolist()
    lap = [_sym(gpu, n, flat[o]) for o in (order, order[::-1], perm)]
    assert all(r[0].tobytes() == lap[0][0].tobytes() and r[1].tobytes() == lap[0][1].tobytes() for r in lap[1:])


def test_sym_capacity_contract(gpu):
    n = 257
    flat, coin = _cells(n, 700, seed=2, coins=True)
    base = _base(D.hub_graph(n, 8, hub=100))
    want_rowptr, want_col, want_info = D.sym_csr_from_cells(n, flat, coin, base)
    nnz = int(want_info[0])
    for cap in (nnz - 1, nnz, 0):
        rowptr, col, info, guard = _sym(gpu, n, flat, coin, base, capacity=cap)
        assert info.tolist() == want_info.tolist()                               # the need is reported all the same
        assert np.all(guard == GUARD32) and np.array_equal(col, want_col[:cap]) and np.array_equal(rowptr, want_rowptr)


def test_sym_counts_bad_and_repeated_cells(gpu):
    n = 300
    flat = _cells(n, 500, seed=3)
    bad = np.concatenate([flat, [np.int64(n) * n,                                # out of range
                                 np.int64(5) * n + 9,                            # j >= i
                                 flat[17]]])                                     # a duplicate
    want = D.sym_csr_from_cells(n, bad)[2]
    rowptr, col, info, guard = _sym(gpu, n, np.random.RandomState(0).permutation(bad))
    assert want[1:].tolist() == [2, 1, 0] and info[1:].tolist() == [2, 1, 0]
    assert np.all(guard == GUARD32) and 0 <= info[0] <= 2 * bad.size
    for extra in ([-1], [np.int64(7) * n + 7], [np.iinfo(np.int64).max], [np.iinfo(np.int64).min]):
        info = _sym(gpu, n, np.concatenate([flat, np.array(extra, dtype=np.int64)]))[2]
        assert info[1:].tolist() == [1, 0, 0] and 0 <= info[0] <= 2 * flat.size + 2


# ---- lt_normalize_csr --------------------------------------------------------------------------------------------------------

def _normalize(gpu, name, rowptr, col, n, capacity=None):
    import torch
    from linkteller_amd import _lib, graph
    h = _lib.lib()
    nnz = int(rowptr[-1])
    cap = nnz + n if capacity is None else capacity
    d_rowptr, d_col = _t(rowptr, gpu, np.int32), _t(col[:nnz], gpu, np.int32)
    inv = torch.from_numpy(graph.inv_power_table(name, n)).to(gpu)
    out_rowptr = torch.full((n + 1,), -7, dtype=torch.int32, device=gpu)
    out_col = torch.full((cap + 8,), GUARD32, dtype=torch.int32, device=gpu)
    out_val = torch.full((cap + 8,), GUARD32, dtype=torch.int32, device=gpu)
    info = torch.full((4,), -1, dtype=torch.int64, device=gpu)
    _lib.check(h.lt_normalize_csr(n, d_rowptr.data_ptr(), d_col.data_ptr(), nnz, _lib.NORM_CODES[name], inv.data_ptr(),
                                  out_rowptr.data_ptr(), out_col.data_ptr(), out_val.data_ptr(), cap, info.data_ptr(),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lt_normalize_csr")
    return out_rowptr.cpu().numpy(), out_col.cpu().numpy(), out_val.cpu().numpy(), info.cpu().numpy(), cap


@pytest.fixture(scope="module")
def norm_graphs():
    golden = csr_from(load_golden("dp_adjacency.npz"), "adj")                   # n = 600
    golden = sp.csr_matrix((golden != 0).astype(np.int64))
    golden.sort_indices()
    return {"single node": sp.csr_matrix((1, 1), dtype=np.int64),
            "hub + loop + isolated": D.hub_graph(300, 1, hub=17, self_loop=40, isolated=123),
            "golden 600": golden}


@pytest.fixture(scope="module")
def host_normalised(norm_graphs):
    """csr_arrays(fetch_normalization(name)(a)) of every graph and name, computed once."""
    from linkteller_amd import graph
    return {(tag, name): graph.csr_arrays(graph.fetch_normalization(name)(a)) for tag, a in norm_graphs.items() for name in D.NORMS}


@pytest.mark.parametrize("name", D.NORMS)
@pytest.mark.parametrize("tag", ["single node", "hub + loop + isolated", "golden 600"])
def test_normalize_equals_the_host_bit_for_bit(gpu, norm_graphs, host_normalised, tag, name):
    a = norm_graphs[tag]
    n = a.shape[0]
    _, want_rowptr, want_col, want_val = host_normalised[(tag, name)]
    restated = D.normalize_csr(name, a.indptr, a.indices, n)
    assert np.array_equal(restated[0], want_rowptr) and np.array_equal(restated[2].view(np.uint32), want_val.view(np.uint32))
    for cap in (None, want_col.size):                                            # nnz + n, and exactly what is written
        rowptr, col, val, info, cap = _normalize(gpu, name, a.indptr, a.indices, n, cap)
        nnz = want_col.size
        assert info.tolist() == [nnz, 0, 0, 0]
        assert np.array_equal(rowptr, want_rowptr) and np.array_equal(col[:nnz], want_col)
        assert np.array_equal(val[:nnz].view(np.uint32), want_val.view(np.uint32))
        assert np.all(col[cap:] == GUARD32) and np.all(val[cap:] == GUARD32)    # the guard words stand
        assert np.all(col[nnz:cap] == GUARD32) and np.all(val[nnz:cap] == GUARD32)


def test_normalize_counts_malformed_rows_and_stays_in_bounds(gpu, norm_graphs):
    a = norm_graphs["hub + loop + isolated"]
    n = a.shape[0]
    col = a.indices.copy()
    r = int(np.flatnonzero(np.diff(a.indptr) >= 3)[5])
    b = a.indptr[r]
    col[b], col[b + 1] = col[b + 1], col[b]                                      # one row unsorted
    r2 = int(np.flatnonzero(np.diff(a.indptr) >= 3)[9])
    col[a.indptr[r2] + 1] = n + 5                                                # one column out of range
    r3 = int(np.flatnonzero(np.diff(a.indptr) >= 3)[12])
    col[a.indptr[r3] + 1] = col[a.indptr[r3]]                                    # one column repeated
    for name in ("FirstOrderGCN", "AugRWalk"):
        rowptr, ocol, oval, info, cap = _normalize(gpu, name, a.indptr, col, n)
        assert info[1] == 3 and info[2:].tolist() == [0, 0] and 0 <= info[0] <= cap
        assert np.all(ocol[cap:] == GUARD32) and np.all(oval[cap:] == GUARD32)
    rowptr, ocol, oval, info, cap = _normalize(gpu, "BingGeNormAdj", a.indptr, a.indices, n, capacity=a.nnz // 2)
    assert info[0] == a.nnz + n - 1 and np.all(ocol[cap:] == GUARD32) and np.all(oval[cap:] == GUARD32)


# ---- the route ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def adj600():
    from linkteller_amd import synth
    return sp.csr_matrix(synth.erdos_renyi_graph(600, 3000, seed=3))


def _host_philox(adj, perturb, eps, seed):
    from linkteller_amd import dp
    m = sp.csr_matrix(dp.perturb_adj(adj, perturb, eps, seed, rng="philox"))
    m.eliminate_zeros()                                                          # EdgeRand keeps a cleared non-edge as a zero
    m.sort_indices()
    return m


@pytest.mark.parametrize("eps", [5.0, 1.0])
@pytest.mark.parametrize("perturb", ["continuous", "discrete"])
def test_perturb_adj_device_equals_the_host_philox_route(gpu, adj600, perturb, eps, capsys):
    import torch
    from linkteller_amd import dp
    want = _host_philox(adj600, perturb, eps, 42)
    host_out = capsys.readouterr().out
    rowptr, col = dp.perturb_adj_device(adj600, perturb, eps, 42)
    assert capsys.readouterr().out == host_out                                   # the same prints
    assert rowptr.is_cuda and col.is_cuda and rowptr.dtype == torch.int32 and col.dtype == torch.int32
    assert np.array_equal(rowptr.cpu().numpy(), want.indptr) and np.array_equal(col.cpu().numpy(), want.indices)
    # a (rowptr, col) pair that already lies on the device
    brp, bcol, _ = dp._device_csr(adj600)
    rowptr2, col2 = dp.perturb_adj_device((brp, bcol), perturb, eps, 42)
    assert torch.equal(rowptr, rowptr2) and torch.equal(col, col2)
    other = dp.perturb_adj_device(adj600, perturb, eps, 43)
    assert other[1].numel() != col.numel() or not torch.equal(other[1], col)


def test_perturb_adj_device_refusals(gpu, adj600):
    from linkteller_amd import dp
    with pytest.raises(NotImplementedError, match="gaussian"):
        dp.perturb_adj_device(adj600, "continuous", 5.0, 42, noise_type="gaussian")
    with pytest.raises(TypeError, match="int32 CUDA"):
        dp.perturb_adj_device((adj600.indptr, adj600.indices), "continuous", 5.0, 42)


@pytest.mark.parametrize("norm", ["FirstOrderGCN", "AugNormAdj"])
def test_from_device_pattern_builds_the_host_routes_graph(gpu, adj600, norm):
    from linkteller_amd import _lib, dp, graph
    noisy = _host_philox(adj600, "continuous", 5.0, 42)
    want = graph.HipGraph(graph.fetch_normalization(norm)(noisy))
    got = graph.HipGraph.from_device_pattern(*dp.perturb_adj_device(adj600, "continuous", 5.0, 42), norm)
    assert got.built_on == "device" and (got.n, got.nnz) == (want.n, want.nnz)
    for name in _lib.GRAPH_TABLES:
        a, b = want.table(name), got.table(name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    with pytest.raises(NotImplementedError):
        graph.HipGraph.from_device_pattern(*dp.perturb_adj_device(adj600, "continuous", 5.0, 42), "SymNorm")


def test_torch_sparse_from_device_csr_equals_the_host_tensor(gpu, adj600):
    import torch
    from linkteller_amd import graph
    m = graph.first_order_gcn(adj600)
    want = graph.sparse_mx_to_torch_sparse_tensor(m).cuda()
    n, rowptr, col, val = graph.csr_arrays(m)
    got = graph.torch_sparse_from_device_csr(*(torch.from_numpy(x).to(gpu) for x in (rowptr, col, val)))
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape and got.is_coalesced() == want.is_coalesced()
    assert got._indices().dtype == torch.int64 and torch.equal(got._indices(), want._indices()) and torch.equal(got._values(), want._values())


def _musae(tmp_path):
    from test_cli_worker_dp import _write_musae
    from linkteller_amd import synth
    a1, a2 = synth.erdos_renyi_graph(80, 400, seed=1), synth.erdos_renyi_graph(60, 300, seed=2)
    _write_musae(str(tmp_path), "ES", a1, 50, 1)
    _write_musae(str(tmp_path), "RU", a2, 50, 2)
    return a1, a2


def _workers(tmp_path, perturb, norm):
    from linkteller_amd.worker import Worker
    out = []
    for build in ("host", "device"):
        args = argparse.Namespace(norm=norm, perturb_type=perturb, epsilon=5.0, noise_seed=SEED_WIDE, noise_type="laplace", delta=1e-5,
                                  noise_rng="philox", dp_build=build)
        out.append(Worker(args, dataset="twitch/ES/RU", mode="vanilla", data_root=str(tmp_path)))
    return out


@pytest.mark.parametrize("perturb,norm", [("continuous", "FirstOrderGCN"), ("discrete", "FirstOrderGCN"), ("discrete", "AugRWalk")])
def test_worker_dp_build_device_serves_the_host_routes_tensors(gpu, tmp_path, perturb, norm):
    import torch
    a1, a2 = _musae(tmp_path)
    host, dev = _workers(tmp_path, perturb, norm)
    assert (dev.adj_ori != a2).nnz == 0 and torch.equal(host.features_2, dev.features_2) and torch.equal(host.labels_1, dev.labels_1)
    for name in ("adj_1", "adj_2"):
        h, d = getattr(host, name), getattr(dev, name)
        assert d.is_cuda and d.is_sparse and d.dtype == torch.float32 and d.shape == h.shape
        hi, hv = h._indices().cpu().numpy(), h._values().cpu().numpy()
        keep = hv != 0                                                           # EdgeRand's cleared non-edges: explicit zeros
        assert (perturb == "discrete") or keep.all()
        assert np.array_equal(d._indices().cpu().numpy(), hi[:, keep])
        assert np.array_equal(d._values().cpu().numpy().view(np.uint32), hv[keep].view(np.uint32))


def test_influence_matrix_is_identical_on_the_two_lapgraph_workers(gpu, tmp_path):
    import torch
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN
    _musae(tmp_path)
    host, dev = _workers(tmp_path, "continuous", "FirstOrderGCN")
    torch.manual_seed(3)
    model = GCN(host.n_features, 32, 2, 0.5).to(gpu).eval()
    got = []
    for w in (host, dev):
        args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=24, sample_seed=42, influence=1e-4,
                                  mode="vanilla", attack_mode="efficient")
        atk = Attacker(args, model, w)
        atk.prepare_test_data()
        got.append((np.asarray(atk.test_nodes), atk.influence_matrix()))
    assert np.array_equal(got[0][0], got[1][0])
    assert got[0][1].shape == (24, 24) and got[0][1].any() and got[0][1].tobytes() == got[1][1].tobytes()

"""The Philox edge-DP route on the GPU against its numpy restatement (dp_philox_restate.py): the selection of
lt_lapgraph_philox (cells and threshold key, bit for bit), its boundaries, its independence of key_hint, the tie rule, the
streaming pass at a capacity below its hits and at rows whose cell index passes 2^33, lt_edgerand_philox, and the route through
dp.perturb_adj and Worker.  Every expectation comes from the restatement; nothing here is compared with the numpy route's
graphs (a given seed gives another graph there)."""
import argparse
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import dp_philox_restate as R
from conftest import csr_from, load_golden

pytestmark = pytest.mark.gpu

N = 257
CELLS = N * (N - 1) // 2
SEED_WIDE = (5 << 32) | 1234
GUARD = 0x5A5A5A5A5A5A5A5A


def _sym(i, j, n):
    """Symmetric 0/1 float32 CSR with the pairs (i, j)."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    m = sp.csr_matrix((np.ones(i.size, dtype=np.float32), (i, j)), shape=(n, n))
    return sp.csr_matrix(m + m.T)


@pytest.fixture(scope="module")
def er257():
    from linkteller_amd import synth
    return sp.csr_matrix(synth.erdos_renyi_graph(N, 600, seed=3))


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _expect(adj, seed, factor, n_keep):
    n = adj.shape[0]
    keys = R.cell_keys(n, seed, adj, factor)
    t, thr, above, taken, tied = R.select(keys, n_keep)
    return R.flat_index(t, n), thr, above, taken, tied, keys


def _check_selection(adj, seed, factor, n_keep, key_hint=0.0):
    from linkteller_amd import dp
    cells, info = dp.lapgraph_philox_select(adj, seed, factor, n_keep, key_hint=key_hint)
    want, thr, above, taken, tied, _ = _expect(adj, seed, factor, n_keep)
    assert cells.dtype == np.int64 and np.array_equal(cells, want)
    assert int(info[0]) == _bits(thr)
    assert (int(info[3]), int(info[4]), int(info[5])) == (above, taken, tied) and info[3] + info[4] == n_keep
    assert info[1] >= n_keep and info[2] >= 1 and info[7] == 0
    return cells, info


# ---- selection ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [5.0, 1.0])
@pytest.mark.parametrize("seed", [42, SEED_WIDE])
def test_selection_equals_the_restatement(gpu, er257, seed, eps):
    eps1 = eps * 0.01
    factor = np.exp(eps - eps1)
    n_keep = 600 + int(R.edge_count_draw(seed, eps1))
    # the case must not be passable by ignoring the adjacency: edges dropped, edges kept only through the factor, non-edges kept
    want, _, _, _, _, keys = _expect(er257, seed, factor, n_keep)
    edge = R.edge_mask(N, er257, 0, CELLS)
    picked = np.zeros(CELLS, dtype=bool)
    picked[R.select(keys, n_keep)[0]] = True
    plain = np.zeros(CELLS, dtype=bool)
    plain[R.select(R.cell_keys(N, seed, er257, 1.0), n_keep)[0]] = True
    dropped, through_factor, non_edges = int((edge & ~picked).sum()), int((edge & picked & ~plain).sum()), int((~edge & picked).sum())
    print(f"seed {seed} eps {eps}: n_keep {n_keep}, edges dropped {dropped}, kept through the factor {through_factor}, non-edges kept {non_edges}")
    assert dropped > 0 and through_factor > 0 and non_edges > 0
    _check_selection(er257, seed, factor, n_keep)


def _star(n, centre):
    others = np.array([v for v in range(n) if v != centre])
    return _sym(np.full(others.size, centre), others, n)


@pytest.mark.parametrize("case", ["n2_empty", "n2_edge", "n3", "keep_one", "keep_all", "empty", "full_row_last", "full_row_first"])
def test_selection_boundaries(gpu, case):
    from linkteller_amd import synth
    factor = float(np.exp(4.95))
    adj, n_keep = {
        "n2_empty": lambda: (sp.csr_matrix((2, 2), dtype=np.float32), 1),
        "n2_edge": lambda: (_sym([1], [0], 2), 1),
        "n3": lambda: (_sym([2], [0], 3), 2),
        "keep_one": lambda: (sp.csr_matrix(synth.erdos_renyi_graph(40, 90, seed=1)), 1),
        "keep_all": lambda: (sp.csr_matrix(synth.erdos_renyi_graph(40, 90, seed=1)), 780),
        "empty": lambda: (sp.csr_matrix((40, 40), dtype=np.float32), 25),
        "full_row_last": lambda: (_star(40, 39), 30),          # row 39 holds every column below it
        "full_row_first": lambda: (_star(40, 0), 30),          # every row's first entry
    }[case]()
    cells, _ = _check_selection(adj, 42, factor, n_keep)
    assert cells.size == n_keep and np.all(np.diff(cells) > 0)
    if case == "keep_all":
        i, j = np.tril_indices(40, -1)
        assert np.array_equal(cells, np.sort(i * 40 + j))


def test_key_hint_does_not_change_the_result(gpu, er257):
    factor = np.exp(4.95)
    n_keep = 600 + int(R.edge_count_draw(42, 0.05))
    base, info0 = _check_selection(er257, 42, factor, n_keep, key_hint=0.0)
    far, info_far = _check_selection(er257, 42, factor, n_keep, key_hint=2.0 ** 60)        # no candidate on the first pass
    low, info_low = _check_selection(er257, 42, factor, n_keep, key_hint=2.0 ** -10)       # every cell a candidate: overflow
    assert np.array_equal(base, far) and np.array_equal(base, low)
    assert info0[0] == info_far[0] == info_low[0]
    print("passes", int(info0[2]), int(info_far[2]), int(info_low[2]), "candidates", int(info0[1]), int(info_far[1]), int(info_low[1]))
    assert info_far[2] > 1 and info_low[2] > 1


def test_tie_rule(gpu):
    """700 of the 780 cells of n = 40 are edges with key 0 (edge_factor = 0): the 380 first cells of the order are the 80
    non-edge cells and the 300 edge cells of smallest t."""
    n, total = 40, 780
    t_edge = np.sort(np.random.RandomState(5).permutation(total)[:700])
    i, j = R.cell_ij(t_edge)
    adj = _sym(i, j, n)
    cells, info = _check_selection(adj, 42, 0.0, 380)
    non_edge = np.setdiff1d(np.arange(total), t_edge)
    want_t = np.sort(np.concatenate([non_edge, t_edge[:300]]))
    assert np.array_equal(cells, R.flat_index(want_t, n))
    assert int(info[0]) == 0 and int(info[3]) == 80 and int(info[4]) == 300 and int(info[5]) == 700


# ---- the streaming pass ---------------------------------------------------------------------------------------------------

def _scan(adj, rows, seed, factor, key_min, capacity):
    """lt_philox_cells_scan with a guard word behind each output buffer: (cells, key bits, count) of the written entries."""
    import torch
    from linkteller_amd import _lib, dp
    n = adj.shape[0]
    rowptr, col, _ = dp._device_csr(adj)
    dev = rowptr.device
    cell = torch.full((capacity + 1,), GUARD, dtype=torch.int64, device=dev)
    key = torch.full((capacity + 1,), GUARD, dtype=torch.int64, device=dev)
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().lt_philox_cells_scan(n, rows[0], rows[1], rowptr.data_ptr(), col.data_ptr(), seed, float(factor), float(key_min),
                                               cell.data_ptr(), key.data_ptr(), capacity, count.data_ptr(),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lt_philox_cells_scan")
    torch.cuda.synchronize()
    found = int(count.item())
    cell, key = cell.cpu().numpy(), key.cpu().numpy()
    assert cell[capacity] == GUARD and key[capacity] == GUARD, "written past the capacity"
    m = min(found, capacity)
    assert np.all(cell[m:] == GUARD) and np.all(key[m:] == GUARD)
    order = np.argsort(cell[:m])
    return cell[:m][order], key[:m][order], found


def _scan_expect(adj, rows, seed, factor, key_min):
    n = adj.shape[0]
    keys = R.cell_keys(n, seed, adj, factor, rows=rows)
    hit = np.flatnonzero(keys >= key_min)
    return R.flat_index(hit + R.tri(rows[0]), n), keys[hit].view(np.int64)


def test_scan_capacity_contract(gpu, er257):
    factor, key_min = float(np.exp(4.95)), 4.0
    want_cell, want_key = _scan_expect(er257, (0, N), 42, factor, key_min)
    assert want_cell.size > 3000
    cell, key, found = _scan(er257, (0, N), 42, factor, key_min, capacity=want_cell.size + 10)
    assert found == want_cell.size and np.array_equal(cell, want_cell) and np.array_equal(key, want_key)
    cell, key, found = _scan(er257, (0, N), 42, factor, key_min, capacity=100)          # fewer slots than hits
    assert found == want_cell.size and cell.size == 100 and np.unique(cell).size == 100
    pos = np.searchsorted(want_cell, cell)
    assert np.array_equal(want_cell[pos], cell) and np.array_equal(want_key[pos], key)
    cell, key, found = _scan(er257, (0, N), 42, factor, key_min, capacity=0)
    assert found == want_cell.size and cell.size == 0
    # a row range: rows [100, 180) of the same stream; an empty range
    part_cell, part_key = _scan_expect(er257, (100, 180), 42, factor, key_min)
    cell, key, found = _scan(er257, (100, 180), 42, factor, key_min, capacity=part_cell.size)
    assert found == part_cell.size and np.array_equal(cell, part_cell) and np.array_equal(key, part_key)
    assert _scan(er257, (57, 57), 42, factor, key_min, capacity=4)[2] == 0
    assert _scan(er257, (0, 1), 42, factor, key_min, capacity=4)[2] == 0


def test_scan_high_rows(gpu):
    """Rows [131070, 131073) of n = 131 073: the cell index passes 2^33 inside row 131072, from where on the block counter's
    high word is in use (q = t >> 1 >= 2^32); the rows in front of it still have a zero high word."""
    n, rows, key_min, factor = 131073, (131070, 131073), 2.0 ** 11, 2.0 ** 13
    assert R.tri(131072) < 2 ** 33 < R.tri(rows[1]) and ((R.tri(rows[1]) - 1) >> 1) >> 32 == 1 and (R.tri(rows[0]) >> 1) >> 32 == 0
    adj = _sym([131070, 131071, 131072, 131072], [5, 131070, 0, 70000], n)
    want_cell, want_key = _scan_expect(adj, rows, SEED_WIDE, factor, key_min)
    edge_cells = np.array([131070 * n + 5, 131071 * n + 131070, 131072 * n, 131072 * n + 70000])
    print("hits", want_cell.size, "of them edges", int(np.isin(want_cell, edge_cells).sum()))
    assert 40 <= want_cell.size <= 200 and np.isin(want_cell, edge_cells).any()
    assert (want_cell // n == 131072).any() and (R.cell_t(want_cell // n, want_cell % n) >= 2 ** 33).any()      # hits past 2^33
    cell, key, found = _scan(adj, rows, SEED_WIDE, factor, key_min, capacity=want_cell.size + 8)
    assert found == want_cell.size and np.array_equal(cell, want_cell) and np.array_equal(key, want_key)


# ---- EdgeRand -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [4.0, 7.0])
def test_edgerand_equals_the_restatement(gpu, eps):
    from linkteller_amd import dp
    s = 2 / (np.exp(eps) + 1)
    thr = dp.edgerand_threshold(s)
    t, coin = R.edgerand_cells(N, 42, s)
    want = R.flat_index(t, N)
    cell, got_coin, found = dp.edgerand_philox_cells(N, 42, thr)
    assert found == want.size and np.array_equal(cell, want) and np.array_equal(got_coin, coin)
    lo, hi = dp.edgerand_philox_cells(N, 42, thr, rows=(0, 100)), dp.edgerand_philox_cells(N, 42, thr, rows=(100, N))
    assert lo[2] + hi[2] == want.size
    assert np.array_equal(np.concatenate([lo[0], hi[0]]), want) and np.array_equal(np.concatenate([lo[1], hi[1]]), coin)


def test_edgerand_capacity_contract(gpu):
    import torch
    from linkteller_amd import _lib, dp
    s = 2 / (np.exp(4.0) + 1)
    t, coin = R.edgerand_cells(N, SEED_WIDE, s)
    want = R.flat_index(t, N)
    cap = 64
    cell = torch.full((cap + 1,), GUARD, dtype=torch.int64, device=gpu)
    flag = torch.full((cap + 8,), 0xA5, dtype=torch.uint8, device=gpu)
    count = torch.full((1,), -7, dtype=torch.int64, device=gpu)
    _lib.check(_lib.lib().lt_edgerand_philox(N, 0, N, SEED_WIDE, dp.edgerand_threshold(s), cell.data_ptr(), flag.data_ptr(), cap,
                                             count.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lt_edgerand_philox")
    torch.cuda.synchronize()
    assert int(count.item()) == want.size > cap
    cell, flag = cell.cpu().numpy(), flag.cpu().numpy()
    assert cell[cap] == GUARD and np.all(flag[cap:] == 0xA5)
    pos = np.searchsorted(want, cell[:cap])
    assert np.unique(cell[:cap]).size == cap and np.array_equal(want[pos], cell[:cap]) and np.array_equal(coin[pos], flag[:cap])


# ---- through Python ---------------------------------------------------------------------------------------------------------

def _check_graph(m, n):
    m = sp.csr_matrix(m)
    m.eliminate_zeros()
    assert m.shape == (n, n) and (m != m.T).nnz == 0 and m.diagonal().sum() == 0 and set(np.unique(m.data)) <= {1}
    return m


@pytest.mark.parametrize("eps", [5.0, 1.0])
def test_perturb_adj_continuous_philox(gpu, er257, eps):
    from linkteller_amd import dp
    a = dp.perturb_adj(er257, "continuous", eps, 42, rng="philox")
    b = dp.perturb_adj_continuous(er257, eps, 42, rng="philox")
    m = _check_graph(a, N)
    assert (sp.csr_matrix(a) != sp.csr_matrix(b)).nnz == 0
    n_keep = 600 + int(R.edge_count_draw(42, eps * 0.01))
    want = _expect(er257, 42, np.exp(eps - eps * 0.01), n_keep)[0]
    assert m.nnz == 2 * n_keep
    low = sp.tril(m, -1).tocoo()
    assert np.array_equal(np.sort(low.row.astype(np.int64) * N + low.col), want)
    assert (sp.csr_matrix(dp.perturb_adj(er257, "continuous", eps, 43, rng="philox")) != sp.csr_matrix(a)).nnz > 0


@pytest.mark.parametrize("eps", [4.0, 7.0])
def test_perturb_adj_discrete_philox(gpu, er257, eps):
    from linkteller_amd import dp
    a = dp.perturb_adj(er257, "discrete", eps, 42, rng="philox")
    b = dp.perturb_adj_discrete(er257, eps, 42, rng="philox")
    m = _check_graph(a, N)
    assert (_check_graph(b, N) != m).nnz == 0
    t, coin = R.edgerand_cells(N, 42, 2 / (np.exp(eps) + 1))
    pairs = R.edge_mask(N, er257, 0, CELLS)
    pairs[t[coin == 1]] = True
    pairs[t[coin == 0]] = False
    assert m.nnz == 2 * int(pairs.sum())
    low = sp.tril(m, -1).tocoo()
    assert np.array_equal(np.sort(low.row.astype(np.int64) * N + low.col), R.flat_index(np.flatnonzero(pairs), N))


def test_numpy_route_unchanged_on_the_gpu(gpu):
    from linkteller_amd import dp
    g = load_golden("dp_adjacency.npz")
    a = csr_from(g, "adj")
    for perturb, eps in (("continuous", 5.0), ("discrete", 4.0)):
        res = sp.csr_matrix(dp.perturb_adj(sp.csr_matrix(a), perturb, eps, 42, rng="numpy"))
        res.sort_indices()
        tag = f"{perturb}.eps{eps:g}"
        assert np.array_equal(res.indptr, g[f"{tag}.indptr"]) and np.array_equal(res.indices, g[f"{tag}.indices"]), tag
        assert np.array_equal(np.asarray(res.data, dtype=np.float64), g[f"{tag}.data"]), tag


@pytest.mark.parametrize("perturb", ["continuous", "discrete"])
def test_worker_serves_a_philox_graph(gpu, tmp_path, perturb):
    from linkteller_amd import synth
    from linkteller_amd.worker import Worker
    a1, a2 = synth.erdos_renyi_graph(40, 90, seed=1), synth.erdos_renyi_graph(30, 60, seed=2)
    synth.write_musae_dataset(str(tmp_path), "ES", a1, 50, 1)
    synth.write_musae_dataset(str(tmp_path), "RU", a2, 50, 2)
    # (seed 42 draws an edge-count noise of -78 at eps 5: more than these graphs' 90 and 60 edges)
    args = argparse.Namespace(norm="FirstOrderGCN", perturb_type=perturb, epsilon=5.0, noise_seed=SEED_WIDE, noise_type="laplace",
                              delta=1e-5, noise_rng="philox")
    clean = Worker(args, dataset="twitch/ES/RU", mode="vanilla-clean", data_root=str(tmp_path))
    served = Worker(args, dataset="twitch/ES/RU", mode="vanilla", data_root=str(tmp_path))
    assert (served.adj_ori != a2).nnz == 0                       # pairs still come from the clean graph
    d0, d1 = clean.adj_2.to_dense().cpu().numpy(), served.adj_2.to_dense().cpu().numpy()
    assert d1.shape == (30, 30) and not np.allclose(d0, d1)

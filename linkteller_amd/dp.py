"""Edge-DP graph perturbation that precedes the hot path in the DP evaluation:
EdgeRand (``--perturb-type discrete``, reference worker.py:213-278) and LapGraph
(``--perturb-type continuous``, reference worker.py:281-335).

The random draws are host numpy, consuming numpy's legacy global stream in the reference's draw order so a
given ``--noise-seed`` yields the reference's graph (pinned by tests/golden/dp_adjacency.npz); LapGraph's
O(N^2) add + top-k select run on the GPU when one is visible (``lt_lapgraph_select``, csrc/lt_dp.hip).

``rng="philox"`` is the second, opt-in noise source: the counter-based cell stream of include/linkteller_hip.h
("edge-DP noise from a counter-based stream"), evaluated per cell on the device (``lt_lapgraph_philox``,
``lt_edgerand_philox``).  No N x N matrix exists anywhere, so it serves graphs the numpy route cannot hold; a given seed
gives a different graph than numpy's stream does.  It needs a GPU.

``perturb_adj_device`` is that route with the graph kept on the device: the cells the two generators write become a symmetric
CSR there (``lt_sym_csr_from_cells``, csrc/lt_dp_graph.hip) and nothing of O(E) visits the host.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


def get_noise(noise_type, size, seed, eps=10, delta=1e-5, sensitivity=2):
    """Seeded Laplace / Gaussian noise, reference utils/load.py:27-39."""
    np.random.seed(seed)
    if noise_type == "laplace":
        return np.random.laplace(0, sensitivity / eps, size)
    if noise_type == "gaussian":
        return np.random.normal(0, np.sqrt(2 * np.log(1.25 / delta)) * sensitivity / eps, size)
    raise NotImplementedError("noise {} not implemented!".format(noise_type))


def _symmetric_from_upper(rows, cols, n):
    """0/1 matrix with the (i < j) pairs and their mirror (role of worker.py:178-203)."""
    keep = rows < cols
    m = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int64), (rows[keep], cols[keep])), shape=(n, n))
    return m + m.T


def _check_rng(rng):
    if rng not in ("numpy", "philox"):
        raise ValueError(f"rng = {rng!r}: 'numpy' or 'philox'")


def perturb_adj_discrete(adj, epsilon, noise_seed, rng="numpy"):
    """EdgeRand: every cell is re-drawn with probability s = 2/(e^eps+1); re-drawn cells of the upper
    triangle become 1 or 0 with probability 1/2.  Draw order: one N x N binomial, then one binomial
    per selected cell in row-major order (worker.py:222-233).

    rng="philox": the same distribution per unordered pair from the device's cell stream (stream 2); no N x N draw."""
    _check_rng(rng)
    s = 2 / (np.exp(epsilon) + 1)
    print(f"s = {s:.4f}")
    n = adj.shape[0]
    if rng == "philox":
        return _edgerand_philox(adj, s, noise_seed)
    np.random.seed(noise_seed)
    rows, cols = np.nonzero(np.random.binomial(1, s, (n, n)))
    coin = np.random.binomial(1, 1 / 2, rows.shape[0])
    add = _symmetric_from_upper(rows[coin == 1], cols[coin == 1], n)
    sub = _symmetric_from_upper(rows[coin == 0], cols[coin == 0], n)
    noisy = adj + add - sub
    noisy.data[noisy.data == -1] = 0          # removed a non-edge: stays absent (explicit zero, as in the reference)
    noisy.data[noisy.data == 2] = 1           # added an existing edge
    return noisy


def _lapgraph_inputs(adj, epsilon, noise_seed, noise_type, delta):
    """The two seeded draws of worker.py:291-304 in the reference's order: the N x N cell noise, then the edge-count noise."""
    n = adj.shape[0]
    n_edges = len(adj.data) // 2
    eps_1 = epsilon * 0.01
    eps_2 = epsilon - eps_1
    noise = get_noise(noise_type, (n, n), noise_seed, eps=eps_2, delta=delta, sensitivity=1)
    n_keep = n_edges + int(get_noise(noise_type, 1, noise_seed, eps=eps_1, delta=delta, sensitivity=1)[0])
    print(f"edge number from {n_edges} to {n_keep}")
    return n, noise, n_keep


def perturb_adj_continuous(adj, epsilon, noise_seed, noise_type="laplace", delta=1e-5, backend="auto", rng="numpy"):
    """LapGraph: Laplace(1/eps2) noise on the strict lower triangle, keep the top-(E + noise) cells,
    symmetrise (worker.py:281-335).  eps is split 1 % / 99 % between the edge count and the cells.
    The reference selects the top cells with a 50-way split + argpartition; the selected *set* is the
    plain top-k (ties only among exact zeros, which are never reached).

    backend: "hip" -- the noise (numpy's stream, drawn here) is uploaded and the add + top-k select run on the GPU
    (lt_lapgraph_select); "host" -- numpy argpartition, as the reference; "auto" -- "hip" when a HIP device is visible.
    Both give the same cells (tests/golden/dp_adjacency.npz).

    rng="philox": cell noise and edge count come from the device's cell stream (streams 0 and 1) instead of numpy's; only
    the CSR is uploaded and the selection runs in O(kept edges) memory (lt_lapgraph_philox).  Laplace only; needs a GPU;
    ``backend`` does not apply."""
    _check_rng(rng)
    if rng == "philox":
        if noise_type != "laplace":
            raise NotImplementedError(f"noise {noise_type} is not implemented for rng='philox' (laplace only)")
        return _lapgraph_philox(adj, epsilon, noise_seed)
    if backend == "auto":
        import torch
        backend = "hip" if torch.cuda.is_available() else "host"
    n, noise, n_keep = _lapgraph_inputs(adj, epsilon, noise_seed, noise_type, delta)
    if backend == "hip":
        top = _lapgraph_select_hip(adj, noise, n_keep)
    elif backend == "host":
        noise *= np.tri(n, n, k=-1, dtype=bool)
        cells = np.asarray(sp.tril(adj, k=-1) + noise).ravel()
        top = np.argpartition(cells, -n_keep)[-n_keep:]
    else:
        raise ValueError(f"backend = {backend!r}")
    mat = sp.csr_matrix((np.ones(n_keep, dtype=np.int32), (top // n, top % n)), shape=(n, n))
    return mat + mat.T


def _lapgraph_select_hip(adj, noise, n_keep):
    """Flat indices of the n_keep largest cells of tril(adj, -1) + noise, selected on the device."""
    import ctypes as C
    import torch
    from . import _lib
    _lib.require_gpu()
    n = adj.shape[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    low = sp.csr_matrix(adj)
    low.sort_indices()
    rowptr = torch.from_numpy(low.indptr.astype(np.int32)).to(dev)
    col = torch.from_numpy(low.indices.astype(np.int32)).to(dev)
    cells = torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64)).to(dev)
    out = torch.empty(n_keep, dtype=torch.int64, device=dev)
    work = torch.zeros(4096, dtype=torch.uint8, device=dev)
    thr = C.c_double(0.0)
    _lib.check(_lib.lib().lt_lapgraph_select(n, rowptr.data_ptr(), col.data_ptr(), cells.data_ptr(), int(n_keep), out.data_ptr(),
                                             work.data_ptr(), work.numel(), C.byref(thr),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lt_lapgraph_select")
    return out.cpu().numpy()


def perturb_adj(adj, perturb_type, epsilon, noise_seed, noise_type="laplace", delta=1e-5, backend="auto", rng="numpy"):
    """Dispatch of worker.py:206-210."""
    if perturb_type == "discrete":
        return perturb_adj_discrete(adj, epsilon, noise_seed, rng=rng)
    return perturb_adj_continuous(adj, epsilon, noise_seed, noise_type, delta, backend=backend, rng=rng)


# ---- rng="philox": the cell stream of include/linkteller_hip.h ------------------------------------------------------------

def _philox4x32_10(counter, key):
    """One Philox4x32-10 block in Python integers (the host needs a single block: the edge-count draw)."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
    return c0, c1, c2, c3


def _seed64(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def philox_edge_count_draw(seed, eps_1):
    """LapGraph's edge-count noise: the inverse-CDF Laplace(1 / eps_1) draw of cell 0 of stream 1."""
    seed = _seed64(seed)
    a, b = _philox4x32_10((0, 0, 1, 0), (seed & 0xFFFFFFFF, seed >> 32))[:2]
    k = (a << 20) | (b >> 12)
    u = np.float64(2 * k + 1) * np.float64(2.0 ** -53)
    return float(np.log(2.0 * u) / eps_1 if k < (1 << 51) else -np.log(2.0 * (1.0 - u)) / eps_1)


def edgerand_threshold(s):
    """floor(s 2^52): a cell is re-drawn iff its 52-bit integer is below it."""
    return int(np.floor(np.float64(s) * np.float64(2.0 ** 52)))


def _device_csr(adj):
    """(rowptr, col) int32 on the current device: sorted, unique, no explicit zeros; col holds one spare element so that an
    empty graph still has a pointer to give."""
    import torch
    low = sp.csr_matrix(adj, copy=True)
    low.sum_duplicates()
    low.eliminate_zeros()
    low.sort_indices()
    dev = torch.device("cuda", torch.cuda.current_device())
    rowptr = torch.from_numpy(low.indptr.astype(np.int32)).to(dev)
    col = torch.from_numpy(np.append(low.indices.astype(np.int32), np.int32(0))).to(dev)
    return rowptr, col, int(low.nnz)


def _lapgraph_philox_cells(rowptr, col, nnz, seed, edge_factor, n_keep, key_hint=0.0):
    """``lt_lapgraph_philox`` on a device CSR: (the selected cells, an unordered int64 CUDA tensor [n_keep]; info, host int64 [8])."""
    import ctypes as C
    import torch
    from . import _lib
    n = rowptr.numel() - 1
    need = C.c_size_t(0)
    _lib.check(_lib.lib().lt_lapgraph_philox_workspace(n, nnz, int(n_keep), C.byref(need)), "lt_lapgraph_philox_workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=rowptr.device)
    out = torch.empty(int(n_keep), dtype=torch.int64, device=rowptr.device)
    info = np.zeros(8, dtype=np.int64)
    _lib.check(_lib.lib().lt_lapgraph_philox(n, rowptr.data_ptr(), col.data_ptr(), _seed64(seed), float(edge_factor), int(n_keep),
                                             float(key_hint), out.data_ptr(), info.ctypes.data, ws.data_ptr(), ws.numel(),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lt_lapgraph_philox")
    return out, info


def lapgraph_philox_select(adj, seed, edge_factor, n_keep, key_hint=0.0):
    """The first ``n_keep`` cells of the stream's order (key descending, then cell ascending) on the device: (flat indices
    i * n + j sorted ascending, info) with ``info`` the int64 [8] of lt_lapgraph_philox."""
    from . import _lib
    _lib.require_gpu()
    out, info = _lapgraph_philox_cells(*_device_csr(adj), seed, edge_factor, n_keep, key_hint)
    return np.sort(out.cpu().numpy()), info


def _lapgraph_philox_n_keep(n, n_edges, epsilon, noise_seed):
    """(n_keep, eps_2): the noisy edge count of the 1 % / 99 % split, printed and checked as on the numpy route."""
    eps_1 = epsilon * 0.01
    total = n * (n - 1) // 2
    n_keep = n_edges + int(philox_edge_count_draw(noise_seed, eps_1))
    print(f"edge number from {n_edges} to {n_keep}")
    if not 1 <= n_keep <= total:
        raise ValueError(f"LapGraph: the noisy edge count {n_keep} is outside [1, {total}]")
    return n_keep, epsilon - eps_1


def _lapgraph_philox(adj, epsilon, noise_seed):
    from . import _lib
    _lib.require_gpu()
    n = adj.shape[0]
    n_keep, eps_2 = _lapgraph_philox_n_keep(n, len(adj.data) // 2, epsilon, noise_seed)
    top, _ = lapgraph_philox_select(adj, noise_seed, np.exp(eps_2), n_keep)
    mat = sp.csr_matrix((np.ones(n_keep, dtype=np.int32), (top // n, top % n)), shape=(n, n))
    return mat + mat.T


def _edgerand_philox_cells_device(n, seed, s_threshold, rows=None, capacity=None):
    """``lt_edgerand_philox`` over rows [rows[0], rows[1]) (default: all): (cells int64, coins uint8 -- CUDA tensors in the
    device's order, cut to what was written --, the count the device found).  Without ``rows`` a capacity that proves too small
    is raised to the count and the call repeated."""
    import ctypes as C
    import torch
    from . import _lib
    r0, r1 = (0, n) if rows is None else rows
    dev = torch.device("cuda", torch.cuda.current_device())
    if capacity is None:
        cells_in = r1 * (r1 - 1) // 2 - r0 * (r0 - 1) // 2 if r0 else r1 * (r1 - 1) // 2
        expect = cells_in * (s_threshold / 2.0 ** 52)
        capacity = int(expect + 8 * np.sqrt(expect) + 1024)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    while True:
        cell = torch.empty(max(capacity, 1), dtype=torch.int64, device=dev)
        coin = torch.empty(max(capacity, 1), dtype=torch.uint8, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().lt_edgerand_philox(n, r0, r1, _seed64(seed), int(s_threshold), cell.data_ptr(), coin.data_ptr(),
                                                 int(capacity), count.data_ptr(), stream), "lt_edgerand_philox")
        found = int(count.item())
        if found <= capacity or rows is not None or capacity == 0:
            break
        capacity = found                      # the 8 sigma of slack did not do: the count is known now
    m = min(found, capacity)
    return cell[:m], coin[:m], found


def edgerand_philox_cells(n, seed, s_threshold, rows=None, capacity=None):
    """The re-drawn cells of rows [rows[0], rows[1]) (default: all) and their coins, sorted by cell: (flat indices i * n + j,
    coins uint8, count).  ``count`` is what the device found; with a ``capacity`` below it only ``capacity`` cells come back."""
    from . import _lib
    _lib.require_gpu()
    cell, coin, found = _edgerand_philox_cells_device(n, seed, s_threshold, rows, capacity)
    cell, coin = cell.cpu().numpy(), coin.cpu().numpy()
    order = np.argsort(cell, kind="stable")
    return cell[order], coin[order], found


def _edgerand_philox_guard(n, s, bytes_per_cell):
    """EdgeRand's output grows with s n^2 / 2: refuse what the device cannot hold (``bytes_per_cell`` per re-drawn cell)."""
    import torch
    expect = int(s * (n * (n - 1) // 2))
    held = bytes_per_cell * (expect + 8 * int(np.sqrt(expect)) + 1024)
    free = torch.cuda.mem_get_info()[0]
    if held > 0.8 * free:
        raise MemoryError(f"EdgeRand with rng='philox' expects {expect} re-drawn cells ({held} bytes on the device, "
                          f"{free} free): the perturbed graph cannot be held; raise epsilon")


def _edgerand_philox(adj, s, noise_seed):
    from . import _lib
    _lib.require_gpu()
    n = adj.shape[0]
    _edgerand_philox_guard(n, s, 9)                                # int64 cell + uint8 coin on the device
    cell, coin, _ = edgerand_philox_cells(n, noise_seed, edgerand_threshold(s))
    i, j = cell // n, cell % n                                     # j < i
    add = _symmetric_from_upper(j[coin == 1], i[coin == 1], n)
    sub = _symmetric_from_upper(j[coin == 0], i[coin == 0], n)
    noisy = adj + add - sub
    noisy.data[noisy.data == -1] = 0          # removed a non-edge: stays absent (explicit zero, as on the numpy route)
    noisy.data[noisy.data == 2] = 1           # added an existing edge
    return noisy


# ---- the philox route with the graph kept on the device ------------------------------------------------------

def sym_csr_from_cells(n, cells, coins=None, base=None):
    """``lt_sym_csr_from_cells``: the listed lower-triangle cells (int64 CUDA tensor of flat indices i * n + j, j < i; ``coins``
    uint8 or None = every cell sets) merged with ``base`` (a ``(rowptr, col, nnz)`` triple of int32 CUDA tensors, or None) into a
    symmetric CSR.  Returns (rowptr int32 [n + 1], col int32 [base nnz + 2 m, which always suffices], info int64 [4] on the
    device): the caller reads ``info`` (nnz, bad cells, repeated cells) and cuts ``col``."""
    import ctypes as C
    import torch
    from . import _lib
    _lib.require_gpu()
    m = int(cells.numel())
    dev = cells.device
    b_rowptr, b_col, b_nnz = base if base is not None else (None, None, 0)
    capacity = b_nnz + 2 * m
    need = _lib.lib().lt_sym_csr_workspace_bytes(n, b_nnz, m)
    if need == 0:
        raise ValueError(f"lt_sym_csr_from_cells: n = {n}, {b_nnz} base entries and {m} cells are outside what int32 row pointers hold")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().lt_sym_csr_from_cells(
            n, b_rowptr.data_ptr() if base is not None else None, b_col.data_ptr() if base is not None else None, b_nnz,
            cells.data_ptr(), coins.data_ptr() if coins is not None else None, m, rowptr.data_ptr(), col.data_ptr(), capacity,
            info.data_ptr(), ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lt_sym_csr_from_cells")
    return rowptr, col, info


def _checked_sym_csr(n, cells, coins, base):
    """(rowptr, col) cut to the result's nnz; the generators' cells are distinct strict-lower cells, anything else is a bug."""
    rowptr, col, info = sym_csr_from_cells(n, cells, coins, base)
    nnz, bad, repeated, _ = info.tolist()                                # the one read-back of this stage: 32 bytes
    if bad or repeated:
        raise RuntimeError(f"lt_sym_csr_from_cells: {bad} cells outside the strict lower triangle, {repeated} repeated cells")
    return rowptr, col[:nnz]


def _as_device_csr(adj):
    """(rowptr, col, nnz) on the device from a scipy matrix (``_device_csr``) or from a (rowptr, col) pair of int32 CUDA tensors
    (canonical: columns sorted and unique per row; ``col`` may carry spare elements behind rowptr[n] entries)."""
    import torch
    if isinstance(adj, (tuple, list)):
        rowptr, col = adj
        for name, t in (("rowptr", rowptr), ("col", col)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1:
                raise TypeError(f"perturb_adj_device: {name} must be a 1-D int32 CUDA tensor")
        if rowptr.numel() < 1 or rowptr.device != col.device:
            raise ValueError("perturb_adj_device: rowptr is empty or lies on another device than col")
        nnz = int(rowptr[-1].item())
        if not 0 <= nnz <= col.numel():
            raise ValueError(f"perturb_adj_device: rowptr[n] = {nnz} with {col.numel()} columns")
        rowptr, col = rowptr.contiguous(), col.contiguous()
        if col.numel() == nnz:                                           # the kernels want a pointer even for an empty graph
            col = torch.cat([col, col.new_zeros(1)])
        return rowptr, col, nnz
    return _device_csr(adj)


def perturb_adj_device(adj, perturb_type, epsilon, noise_seed, noise_type="laplace", delta=1e-5):
    """``perturb_adj(..., rng="philox")`` with the result left on the device: (rowptr, col) int32 CUDA tensors of the perturbed
    0/1 graph, columns strictly increasing, no explicit zeros (the host EdgeRand route keeps a cleared non-edge as an explicit
    zero; it is the same graph).  ``adj``: a scipy matrix, or a (rowptr, col) pair of int32 CUDA tensors.  Draws, prints and
    refusals are the philox route's: Laplace only, a GPU is needed, EdgeRand refuses a graph the device cannot hold."""
    import torch
    from . import _lib
    if perturb_type != "discrete" and noise_type != "laplace":
        raise NotImplementedError(f"noise {noise_type} is not implemented for rng='philox' (laplace only)")
    _lib.require_gpu()
    rowptr, col, nnz = _as_device_csr(adj)
    n = rowptr.numel() - 1
    with torch.cuda.device(rowptr.device):
        if perturb_type == "discrete":
            s = 2 / (np.exp(epsilon) + 1)
            print(f"s = {s:.4f}")
            # per re-drawn cell: int64 cell + uint8 coin, then two directed entries of four sort words, a merged column and a flag
            _edgerand_philox_guard(n, s, 9 + 2 * 24)
            cell, coin, _ = _edgerand_philox_cells_device(n, noise_seed, edgerand_threshold(s))
            return _checked_sym_csr(n, cell, coin, (rowptr, col, nnz))
        # (the host route counts the entries of the matrix it is given)
        n_keep, eps_2 = _lapgraph_philox_n_keep(n, len(adj.data) // 2 if sp.issparse(adj) else nnz // 2, epsilon, noise_seed)
        out, _ = _lapgraph_philox_cells(rowptr, col, nnz, noise_seed, np.exp(eps_2), n_keep)
        return _checked_sym_csr(n, out, None, None)

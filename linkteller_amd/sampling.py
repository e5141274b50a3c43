"""Node / node-pair sampling for the attack (reference attacker.py:33-48, utils/load.py:304-381).

Host-side integer work by default (the device routes are at the end of the file).  The node draw must reproduce numpy's *legacy global* stream
(``np.random.seed(sample_seed)`` then ``np.random.choice(..., replace=False)``, attacker.py:45 and
utils/load.py:379), so it stays on ``np.random``; the O(n_test^2) pair enumeration is vectorised
but returns the pairs in the reference's order (i < j over the sampled nodes, row-major).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


def degree_bounds(dataset: str):
    """(lo, hi) thresholds of utils/load.py:354-372."""
    if dataset.startswith("twitch"):
        return (5 if "PTBR" not in dataset else 10), 10
    if dataset in ("flickr", "ppi") or dataset.startswith("deezer"):
        return 15, 30
    if dataset in "cora":        # the reference tests substring membership: ( 'cora' ) is a str
        return 3, 4
    if dataset in "citeseer":
        return 3, 3
    if dataset in "pubmed":
        return 10, 10
    raise NotImplementedError(f"lo and hi for dataset = {dataset} not set!")


def edge_sets_among_nodes(adj: sp.csr_matrix, nodes: np.ndarray):
    """All pairs (nodes[i], nodes[j]), i < j, split by structural presence of nodes[j] in row
    nodes[i] of ``adj`` (utils/load.py:304-326).  Returns two int64 arrays of shape [k, 2]."""
    nodes = np.asarray(nodes, dtype=np.int64)
    k = nodes.shape[0]
    pattern = sp.csr_matrix((np.ones(adj.indices.shape[0], dtype=np.int8), adj.indices, adj.indptr),
                            shape=adj.shape)
    sub = pattern[nodes][:, nodes].toarray() != 0
    iu, ju = np.triu_indices(k, k=1)
    present = sub[iu, ju]
    pairs = np.stack([nodes[iu], nodes[ju]], axis=1)
    return pairs[present], pairs[~present]


def draw_subgraph_nodes(dataset, sample_type, adj, n_samples):
    """The node draw of utils/load.py:338-379: ``n_samples`` distinct nodes from all nodes (``unbalanced``) or from the low- /
    high-degree ones, off numpy's legacy global stream.  ``adj``: a scipy CSR matrix."""
    n_nodes = adj.shape[0]
    if sample_type == "unbalanced":
        candidates = np.arange(n_nodes)
    else:
        deg = np.diff(adj.indptr)
        lo, hi = degree_bounds(dataset)
        if sample_type == "unbalanced-lo":
            candidates = np.where(deg <= lo)[0]
        elif sample_type == "unbalanced-hi":
            candidates = np.where(deg >= hi)[0]
        else:
            raise NotImplementedError(f"sample_type = {sample_type} not implemented!")
    print("#indice =", len(candidates))
    return np.random.choice(candidates, n_samples, replace=False)


def construct_edge_sets_from_random_subgraph(dataset, sample_type, adj, n_samples):
    """Same signature/return shape as utils/load.py:338-381: ((edges, non_edges), nodes)."""
    adj = sp.csr_matrix(adj)
    nodes = draw_subgraph_nodes(dataset, sample_type, adj, n_samples)
    edges, non_edges = edge_sets_among_nodes(adj, nodes)
    print("#nodes =", len(nodes))
    print("#edges_set =", len(edges))
    print("#nonedge_set =", len(non_edges))
    return (edges, non_edges), nodes


def construct_balanced_edge_sets(dataset, sample_type, adj, n_samples):
    """``balanced-full`` (reference utils/load.py:219-249): every u < v edge of the graph, plus as many
    random pairs that are adjacent in neither direction.  The non-edge draws are two scalar
    ``np.random.choice(n_nodes)`` calls per candidate, in the reference's order (u == v and repeated
    pairs can occur, as they do there).  Returns ((edges, non_edges), all nodes)."""
    adj = sp.csr_matrix(adj)
    n_nodes = adj.shape[0]
    indptr, indices = adj.indptr, adj.indices
    rows = np.repeat(np.arange(n_nodes, dtype=np.int64), np.diff(indptr))
    upper = indices > rows
    edges = np.stack([rows[upper], indices[upper].astype(np.int64)], axis=1)
    nbr_sets = [set(indices[indptr[u]: indptr[u + 1]].tolist()) for u in range(n_nodes)]
    non_edges = np.empty((edges.shape[0], 2), dtype=np.int64)
    k = 0
    while k < edges.shape[0]:
        u = np.random.choice(n_nodes)
        v = np.random.choice(n_nodes)
        if v not in nbr_sets[u] and u not in nbr_sets[v]:
            non_edges[k] = (u, v)
            k += 1
    print(f"sampling done! len(edge_set) = {len(edges)}, len(nonedge_set) = {len(non_edges)}")
    return (edges, non_edges), list(range(n_nodes))


# ---- the pairs on the device (include/linkteller_hip.h, "the attack's node pairs") --------------------

def device_pattern_csr(adj):
    """(rowptr, col, nnz) int32 CUDA tensors of the STRUCTURAL pattern, columns sorted and unique per row.  A scipy matrix keeps
    its stored zeros (``dp._device_csr`` drops them): the labels read presence, as ``edge_sets_among_nodes`` does.  A
    (rowptr, col) pair of int32 CUDA tensors is checked as ``dp._as_device_csr`` checks it.  ``col`` holds one spare element so
    that an empty graph still has a pointer to give."""
    import torch
    from . import _lib, dp
    if isinstance(adj, (tuple, list)):
        return dp._as_device_csr(adj[:2])
    _lib.require_gpu()
    a = sp.csr_matrix(adj)
    pat = sp.csr_matrix((np.ones(a.indices.shape[0], dtype=np.int8), a.indices.copy(), a.indptr.copy()), shape=a.shape)
    pat.sum_duplicates()                  # (a stored zero stays: only eliminate_zeros() would drop it)
    pat.sort_indices()
    dev = torch.device("cuda", torch.cuda.current_device())
    rowptr = torch.from_numpy(pat.indptr.astype(np.int32)).to(dev)
    col = torch.from_numpy(np.append(pat.indices.astype(np.int32), np.int32(0))).to(dev)
    return rowptr, col, int(pat.nnz)


def _stream():
    import ctypes as C
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def square_labels_device(csr, nodes, lds, index=True):
    """``lt_sample_square_labels``: all pairs (nodes[i], nodes[j]), i < j over the POSITIONS of the sample, in the row-major order
    of ``edge_sets_among_nodes``.  ``csr``: what ``device_pattern_csr`` returns; ``nodes``: int32 CUDA tensor or a host list (range
    and repeats are checked on the device either way).  Returns ``(index, labels, info)``: ``index`` int64 [T] (``j * lds + i``,
    the cell "perturb nodes[j], observe nodes[i]" of score rows of stride ``lds``; None with ``index=False``), ``labels`` uint8 [T]
    (1 iff nodes[j] is stored in row nodes[i]) and ``info`` int64 [4] -- all on the device: ``info[0]`` is the number of edges,
    ``info[1]`` / ``info[2]`` count out-of-range / repeated nodes (``check_square_info`` raises on them).  Enqueues on the current
    stream and does not synchronise."""
    import torch
    from . import _lib
    _lib.require_gpu()
    rowptr, col, nnz = csr
    dev = rowptr.device
    n = int(rowptr.numel()) - 1
    if not (isinstance(nodes, torch.Tensor) and nodes.is_cuda and nodes.dtype == torch.int32):
        nodes = torch.as_tensor(np.asarray(nodes, dtype=np.int64).reshape(-1).astype(np.int32)).to(dev)
    nodes = nodes.contiguous()
    k, lds = int(nodes.numel()), int(lds)
    if k < 2:
        raise ValueError("square_labels_device: fewer than two sampled nodes")
    if lds < k:
        raise ValueError(f"square_labels_device: row stride {lds} smaller than the {k} sampled nodes")
    total = k * (k - 1) // 2
    labels = torch.empty(total, dtype=torch.uint8, device=dev)
    idx = torch.empty(total, dtype=torch.int64, device=dev) if index else None
    info = torch.empty(4, dtype=torch.int64, device=dev)
    ws = torch.empty(max(_lib.lib().lt_sample_square_workspace_bytes(n, k), 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().lt_sample_square_labels(n, rowptr.data_ptr(), col.data_ptr(), nnz, nodes.data_ptr(), k, lds,
                                                      labels.data_ptr(), idx.data_ptr() if index else None, info.data_ptr(),
                                                      ws.data_ptr(), ws.numel(), _stream()), "lt_sample_square_labels")
    return idx, labels, info


def check_square_info(info):
    """The host's look at ``square_labels_device``'s info (one copy of 4 words, one wait): the number of edges; ``IndexError`` for
    nodes outside the graph, ``ValueError`` for repeated nodes."""
    n_edges, outside, repeated, _ = [int(v) for v in info.tolist()]
    if outside:
        raise IndexError(f"square_labels_device: {outside} sampled nodes outside the graph")
    if repeated:
        raise ValueError(f"square_labels_device: {repeated} sampled nodes repeat an earlier one")
    return n_edges


def upper_edge_count(csr):
    """E = the stored entries with col > row (``lt_upper_edge_count``; one copy of a word, one wait)."""
    import torch
    from . import _lib
    _lib.require_gpu()
    rowptr, col, nnz = csr
    count = torch.empty(1, dtype=torch.int64, device=rowptr.device)
    with torch.cuda.device(rowptr.device):
        _lib.check(_lib.lib().lt_upper_edge_count(int(rowptr.numel()) - 1, rowptr.data_ptr(), col.data_ptr(), nnz, count.data_ptr(),
                                                  _stream()), "lt_upper_edge_count")
    return int(count.item())


def balanced_pairs_philox(csr, seed, *, max_draws=0, round_draws=0, n_edges=None):
    """``lt_sample_balanced_philox``: the ``balanced-full`` pair lists on the device -> ``(u, v, E, info)``.  ``u``, ``v``: int32
    CUDA tensors of 2 E entries; [0, E) are the edges (every stored entry with col > row, in ``construct_balanced_edge_sets``'
    order), [E, 2 E) the first E accepted draws of Philox stream 3 (include/linkteller_hip.h): pairs adjacent in neither
    direction, u == v and repeats possible as in the reference -- a DIFFERENT sample than numpy's stream gives for the seed.
    ``info``: host int64 [8] (E, draws consumed, rounds, accepted draws with u == v).  ``n_edges``: E when the caller knows it
    (else counted by ``upper_edge_count``).  Synchronises.  A graph too dense to yield E non-edges within ``max_draws``
    (0 = 64 E + 4096) raises ``LinkTellerHipError``; the reference's loop would not end there."""
    import torch
    from . import _lib, dp
    _lib.require_gpu()
    rowptr, col, nnz = csr
    dev = rowptr.device
    n = int(rowptr.numel()) - 1
    n_e = upper_edge_count(csr) if n_edges is None else int(n_edges)
    need = _lib.lib().lt_sample_balanced_workspace_bytes(n, n_e, int(round_draws))
    if need == 0:
        raise ValueError(f"balanced_pairs_philox: E = {n_e} or round_draws = {round_draws} outside what the library serves")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    u = torch.empty(max(2 * n_e, 1), dtype=torch.int32, device=dev)
    v = torch.empty(max(2 * n_e, 1), dtype=torch.int32, device=dev)
    info = np.zeros(8, dtype=np.int64)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().lt_sample_balanced_philox(n, rowptr.data_ptr(), col.data_ptr(), nnz, n_e, dp._seed64(seed),
                                                        int(max_draws), int(round_draws), u.data_ptr(), v.data_ptr(),
                                                        info.ctypes.data, ws.data_ptr(), ws.numel(), _stream()),
                   "lt_sample_balanced_philox")
    return u[:2 * n_e], v[:2 * n_e], n_e, info

"""numpy restatement of the edge-DP cell stream (include/linkteller_hip.h, "edge-DP noise from a counter-based stream";
csrc/lt_dp.hip), built on train_restate.philox4x32_10.  Shared by test_dp_philox_cpu.py and test_dp_philox_gpu.py.

A cell is a strict-lower-triangle pair (i, j), j < i, with the linear index t = i (i - 1) / 2 + j.  Cells 2q and 2q + 1 share
the Philox block with counter (q lo, q hi, stream, 0) and key (seed lo, seed hi); cell t takes the words a = w[2 (t & 1)] and
b = w[2 (t & 1) + 1], k = (a << 20) | (b >> 12), u = (2k + 1) 2^-53, coin = b & 1."""
import numpy as np

import train_restate as T

STREAM_LAPGRAPH, STREAM_EDGE_COUNT, STREAM_EDGERAND = 0, 1, 2
_LO = np.uint64(0xFFFFFFFF)


def tri(i):
    """Cells in front of row i."""
    i = int(i)
    return i * (i - 1) // 2


def cell_t(i, j):
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    return i * (i - 1) // 2 + j


def cell_ij(t):
    """(i, j) of the linear cell indices t (int64 arrays)."""
    t = np.asarray(t, dtype=np.int64)
    i = np.floor((1.0 + np.sqrt(1.0 + 8.0 * t.astype(np.float64))) / 2.0).astype(np.int64)
    i = np.where(i * (i - 1) // 2 > t, i - 1, i)
    i = np.where(i * (i + 1) // 2 <= t, i + 1, i)
    j = t - i * (i - 1) // 2
    assert np.all((j >= 0) & (j < i))
    return i, j


def cell_words(t, seed, stream):
    """(k, u, coin) of the cells t: the 52-bit integer (uint64), the uniform (float64), the coin bit (uint8)."""
    t = np.asarray(t, dtype=np.uint64).reshape(-1)
    q = t >> np.uint64(1)
    ctr = np.stack([q & _LO, q >> np.uint64(32), np.full_like(q, stream), np.zeros_like(q)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), (q.size, 2))
    w = T.philox4x32_10(ctr, key).astype(np.uint64)
    sel = ((t & np.uint64(1)) * np.uint64(2)).astype(np.int64)
    rows = np.arange(q.size)
    a, b = w[rows, sel], w[rows, sel + 1]
    k = (a << np.uint64(20)) | (b >> np.uint64(12))
    u = (np.uint64(2) * k + np.uint64(1)).astype(np.float64) * np.float64(2.0 ** -53)
    return k, u, (b & np.uint64(1)).astype(np.uint8)


def rank_factor(k, u):
    """g: 2u below one half, else 1 / (2 (1 - u)) -- exp(eps2 * Laplace(1 / eps2)) of the inverse-CDF draw of u."""
    low = k < np.uint64(1 << 51)
    return np.where(low, 2.0 * u, 1.0 / (2.0 * (1.0 - np.where(low, 0.5, u))))


def laplace_unit(k, u):
    """The inverse-CDF Laplace(0, 1) draw of u, by np.log."""
    low = k < np.uint64(1 << 51)
    return np.where(low, np.log(2.0 * np.where(low, u, 0.25)), -np.log(2.0 * (1.0 - np.where(low, 0.5, u))))


def edge_mask(n, adj, t0, t1):
    """bool [t1 - t0]: the cells of [t0, t1) that are entries (i, j), j < i, of the scipy matrix adj."""
    coo = adj.tocoo()
    keep = (coo.col < coo.row) & (coo.data != 0)
    t = cell_t(coo.row[keep], coo.col[keep])
    t = t[(t >= t0) & (t < t1)]
    mask = np.zeros(t1 - t0, dtype=bool)
    mask[t - t0] = True
    return mask


def cell_keys(n, seed, adj, edge_factor, rows=None):
    """float64 keys of the cells of rows [rows[0], rows[1]) (default: all rows), in t order: g * edge_factor on the edge cells
    of adj, g elsewhere."""
    r0, r1 = (0, n) if rows is None else rows
    t0, t1 = tri(r0), tri(r1)
    k, u, _ = cell_words(np.arange(t0, t1, dtype=np.uint64), seed, STREAM_LAPGRAPH)
    g = rank_factor(k, u)
    return np.where(edge_mask(n, adj, t0, t1), g * np.float64(edge_factor), g)


def select(keys, n_keep):
    """The first n_keep cells of the total order (key descending, then t ascending) over keys[t]: (t of the selected cells
    ascending, the threshold key, cells above it, tied cells taken, tied cells in total)."""
    keys = np.asarray(keys, dtype=np.float64)
    order = np.argsort(-keys, kind="stable")[:n_keep]          # stable: equal keys stay in t order
    thr = keys[order[-1]]
    above, tied = int((keys > thr).sum()), int((keys == thr).sum())
    return np.sort(order).astype(np.int64), thr, above, n_keep - above, tied


def edgerand_threshold(s):
    return int(np.floor(np.float64(s) * np.float64(2.0 ** 52)))


def edgerand_cells(n, seed, s, rows=None):
    """(t of the re-drawn cells ascending, their coins): k < floor(s 2^52) on stream 2."""
    r0, r1 = (0, n) if rows is None else rows
    t = np.arange(tri(r0), tri(r1), dtype=np.uint64)
    k, _, coin = cell_words(t, seed, STREAM_EDGERAND)
    hit = k < np.uint64(edgerand_threshold(s))
    return t[hit].astype(np.int64), coin[hit]


def edge_count_draw(seed, eps1):
    """LapGraph's edge-count noise: the Laplace(1 / eps1) draw of cell 0 of stream 1."""
    k, u, _ = cell_words(np.array([0], dtype=np.uint64), seed, STREAM_EDGE_COUNT)
    return float(laplace_unit(k, u)[0] / eps1)


def flat_index(t, n):
    """i * n + j of the cells t."""
    i, j = cell_ij(t)
    return i * n + j

"""numpy restatements of the sampling contracts of include/linkteller_hip.h ("the attack's node pairs"): the label triangle of a
node sample (lt_sample_square_labels), the grouped pair layout (lt_group_pairs) and the balanced pair lists with their Philox
stream 3 (lt_sample_balanced_philox).  Shared by test_sample_cpu.py and test_sample_gpu.py; nothing here imports the library."""
import numpy as np
import scipy.sparse as sp

from train_restate import philox4x32_10


def pattern(adj):
    """The structural pattern: every stored entry (stored zeros included) as 1, columns sorted and unique per row."""
    a = sp.csr_matrix(adj)
    p = sp.csr_matrix((np.ones(a.indices.shape[0], dtype=np.int8), a.indices.copy(), a.indptr.copy()), shape=a.shape)
    p.sum_duplicates()
    p.sort_indices()
    p.data[:] = 1
    return p


def triangle(k):
    """(iu, ju): the positions of slot p = i (2 k - i - 1) / 2 + (j - i - 1), i < j -- np.triu_indices' order."""
    iu, ju = np.triu_indices(k, k=1)
    p = iu * (2 * k - iu - 1) // 2 + (ju - iu - 1)
    assert np.array_equal(p, np.arange(k * (k - 1) // 2))
    return iu, ju


def square_labels(adj, nodes, lds):
    """(index int64 [T], labels uint8 [T], number set) by per-pair membership tests, written out pair by pair."""
    p = pattern(adj)
    nodes = np.asarray(nodes, dtype=np.int64)
    k = nodes.size
    rows = [set(p.indices[p.indptr[u]:p.indptr[u + 1]].tolist()) for u in range(p.shape[0])]
    iu, ju = triangle(k)
    labels = np.array([1 if int(nodes[j]) in rows[int(nodes[i])] else 0 for i, j in zip(iu, ju)], dtype=np.uint8)
    index = ju.astype(np.int64) * int(lds) + iu.astype(np.int64)
    return index, labels, int(labels.sum())


def group_pairs(probe, observed):
    """(nodes, ptr, obs, order) by one pass over the pairs with a list per probe: no sort routine shared with the code under test."""
    probe = np.asarray(probe, dtype=np.int64).reshape(-1)
    observed = np.asarray(observed, dtype=np.int64).reshape(-1)
    groups = {}
    for idx, p in enumerate(probe.tolist()):
        groups.setdefault(p, []).append(idx)
    nodes = sorted(groups)
    order = np.array([i for p in nodes for i in groups[p]], dtype=np.int64)
    ptr = np.zeros(len(nodes) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(groups[p]) for p in nodes])
    return np.array(nodes, dtype=np.int32), ptr, observed[order].astype(np.int32), order


def upper_edges(adj):
    """[E, 2] int64: the stored entries with col > row, rows ascending, columns ascending within a row."""
    p = pattern(adj)
    rows = np.repeat(np.arange(p.shape[0], dtype=np.int64), np.diff(p.indptr))
    up = p.indices > rows
    return np.stack([rows[up], p.indices[up].astype(np.int64)], axis=1)


def draws(n, seed, t0, count):
    """(u, v) int64 [count] of the draws t0 .. t0 + count - 1 of stream 3."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    t = np.arange(t0, t0 + count, dtype=np.uint64)
    ctr = np.stack([t & np.uint64(0xFFFFFFFF), t >> np.uint64(32), np.full_like(t, 3), np.zeros_like(t)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), (count, 2))
    w = philox4x32_10(ctr, key).astype(np.uint64)
    u = (w[:, 0] * np.uint64(n)) >> np.uint64(32)
    v = (w[:, 1] * np.uint64(n)) >> np.uint64(32)
    return u.astype(np.int64), v.astype(np.int64)


def default_max_draws(n_edges):
    return 64 * n_edges + 4096


def balanced_pairs(adj, seed, max_draws=0):
    """dict(ok, edges [E, 2], non_edges [accepted, 2] (E of them when ok), draws, self_pairs, accepted): draw by draw, the
    reference's loop with the stream swapped in -- accepted iff v is not stored in row u and u is not stored in row v."""
    p = pattern(adj)
    n = p.shape[0]
    edges = upper_edges(p)
    n_edges = edges.shape[0]
    cap = int(max_draws) if max_draws else default_max_draws(n_edges)
    rows = [set(p.indices[p.indptr[u]:p.indptr[u + 1]].tolist()) for u in range(n)]
    out, t, last, self_pairs = [], 0, 0, 0
    while len(out) < n_edges and t < cap:
        cnt = min(4096, cap - t)
        us, vs = draws(n, seed, t, cnt)
        for x in range(cnt):
            u, v = int(us[x]), int(vs[x])
            if v not in rows[u] and u not in rows[v]:
                out.append((u, v))
                self_pairs += u == v
                last = t + x + 1
                if len(out) == n_edges:
                    break
        t += cnt
    ok = len(out) == n_edges
    return dict(ok=ok, edges=edges, non_edges=np.array(out, dtype=np.int64).reshape(-1, 2), draws=last if ok else t,
                self_pairs=int(self_pairs), accepted=len(out))

"""numpy restatements of lt_sym_csr_from_cells and lt_normalize_csr (include/linkteller_hip.h, "a DP graph stays on the device";
csrc/lt_dp_graph.hip).  Shared by test_dp_device_cpu.py, which holds them against scipy and the host normalisers, and
test_dp_device_gpu.py, which holds the kernels against them."""
import numpy as np
import scipy.sparse as sp

NORMS = ("FirstOrderGCN", "BingGeNormAdj", "NormAdj", "AugRWalk", "RWalk", "AugNormAdj")
AUG = ("BingGeNormAdj", "AugRWalk", "AugNormAdj")            # A + I before the degrees
PLUS_ONE = ("FirstOrderGCN", "BingGeNormAdj")                # + I after the scaling
WALK = ("RWalk", "AugRWalk")                                 # D^-1 A: one factor, infinities kept


def _csr_from_keys(keys, n):
    """(rowptr int32, col int32) of the sorted, unique flat indices r * n + c."""
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(keys // n, minlength=n))
    return rowptr.astype(np.int32), (keys % n).astype(np.int32)


def pattern_keys(rowptr, col, n):
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    return rows * n + np.asarray(col[:rowptr[-1]], dtype=np.int64)


def sym_csr_from_cells(n, cells, coins=None, base=None):
    """Row r = {c in base row r : {r, c} not listed with coin 0} u {c : {r, c} listed with coin 1}; (rowptr, col, info [4]).
    base: (rowptr, col) or None.  info = [nnz, cells that are no strict-lower cell, listed cells that repeat one, 0]; the graph is
    formed from the valid cells (the device leaves it unspecified when info[1] or info[2] is non-zero)."""
    cells = np.asarray(cells, dtype=np.int64)
    coins = np.ones(cells.size, dtype=np.uint8) if coins is None else np.asarray(coins, dtype=np.uint8)
    ok = (cells >= 0) & (cells < n * n)
    i, j = np.where(ok, cells // n, 0), np.where(ok, cells % n, 0)
    ok &= j < i
    i, j, coin = i[ok], j[ok], coins[ok] != 0
    repeated = int(i.size - np.unique(i * n + j).size)
    both = lambda sel: np.concatenate([i[sel] * n + j[sel], j[sel] * n + i[sel]])
    have = np.zeros(0, dtype=np.int64) if base is None else pattern_keys(base[0], base[1], n)
    kept = have[~np.isin(have, both(~coin))]
    keys = np.union1d(kept, both(coin))
    rowptr, col = _csr_from_keys(keys, n)
    return rowptr, col, np.array([keys.size, int((~ok).sum()), repeated, 0], dtype=np.int64)


def inv_pow_table(name, n):
    """np.power(arange(n + 2), p): p = -1/2 with the infinity zeroed, p = -1 with it kept for the random-walk forms."""
    with np.errstate(divide="ignore"):
        d = np.power(np.arange(n + 2, dtype=np.float64), -1.0 if name in WALK else -0.5)
    if name not in WALK:
        d[np.isinf(d)] = 0.0
    return d


def normalize_csr(name, rowptr, col, n, inv_pow=None):
    """The header's recipe on the unit pattern (rowptr, col): (rowptr int32, col int32, val float32)."""
    aug, plus1, walk = name in AUG, name in PLUS_ONE, name in WALK
    inv_pow = inv_pow_table(name, n) if inv_pow is None else inv_pow
    have = pattern_keys(rowptr, col, n)
    keys = np.union1d(have, np.arange(n, dtype=np.int64) * (n + 1)) if (aug or plus1) else have
    r, c = keys // n, keys % n
    d = inv_pow[np.diff(rowptr).astype(np.int64) + (1 if aug else 0)]
    a = np.isin(keys, have).astype(np.float64) + np.where(aug & (r == c), 1.0, 0.0)
    with np.errstate(invalid="ignore"):
        v = d[r] * a
        if not walk:
            v = v * d[c]
    if plus1:
        v = np.where(r == c, v + 1.0, v)
    out_rowptr, out_col = _csr_from_keys(keys, n)
    return out_rowptr, out_col, v.astype(np.float32)


def unit_matrix(rowptr, col, n, dtype=np.int64):
    """The scipy 0/1 matrix of a pattern."""
    nnz = int(rowptr[-1])
    return sp.csr_matrix((np.ones(nnz, dtype=dtype), np.asarray(col[:nnz]), np.asarray(rowptr)), shape=(n, n))


def hub_graph(n, seed, hub=None, self_loop=None, isolated=None, e_per_node=4):
    """A symmetric 0/1 int64 CSR with a hub row (joined to every node but the isolated one), optionally a self-loop and an
    isolated node."""
    rng = np.random.RandomState(seed)
    i = rng.randint(0, n, e_per_node * n)
    j = rng.randint(0, n, e_per_node * n)
    keep = i != j
    i, j = i[keep], j[keep]
    if hub is not None:
        others = np.setdiff1d(np.arange(n), [hub])
        i, j = np.concatenate([i, np.full(others.size, hub)]), np.concatenate([j, others])
    m = sp.coo_matrix((np.ones(i.size, dtype=np.int64), (i, j)), shape=(n, n)).tocsr()
    m = ((m + m.T) > 0).astype(np.int64).tolil()
    if isolated is not None:
        m[isolated, :] = 0
        m[:, isolated] = 0
    if self_loop is not None:
        m[self_loop, self_loop] = 1
    m = sp.csr_matrix(m)
    m.eliminate_zeros()
    m.sort_indices()
    return m

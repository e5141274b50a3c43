"""lt_pairs_present / engine.pairs_present against scipy's ``pattern[u, v]`` on the structural pattern of a graph."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu


def _pattern(adj):
    a = sp.csr_matrix(adj)
    p = sp.csr_matrix((np.ones(a.indices.shape[0], dtype=np.int8), a.indices.copy(), a.indptr.copy()), shape=a.shape)
    p.sum_duplicates()
    p.sort_indices()
    return p


def _graphs():
    from linkteller_amd import synth
    er = sp.lil_matrix(synth.erdos_renyi_graph(1301, 6000, seed=5))
    er[17, :] = 0          # empty rows (and their columns: the pattern stays symmetric)
    er[:, 17] = 0
    er[1300, :] = 0
    er[:, 1300] = 0
    er = sp.csr_matrix(er)
    er.eliminate_zeros()
    hub = synth.powerlaw_graph(900, 7000, seed=6)
    return {"er": er, "hub": hub}


@pytest.mark.parametrize("name", ["er", "hub"])
def test_pairs_present_equals_scipy(gpu, name):
    from linkteller_amd import engine, sampling
    adj = _graphs()[name]
    pat = _pattern(adj)
    n = pat.shape[0]
    csr = sampling.device_pattern_csr(adj)
    rng = np.random.RandomState(11)
    u = [rng.randint(n, size=20000)]
    v = [rng.randint(n, size=20000)]
    coo = pat.tocoo()
    u.append(coo.row), v.append(coo.col)                             # every stored entry
    lens = np.diff(pat.indptr)
    rows = np.flatnonzero(lens > 0)
    first, last = pat.indices[pat.indptr[rows]], pat.indices[pat.indptr[rows + 1] - 1]
    for cols in (first, last, first - 1, last + 1):                  # the ends of every row and the columns just outside them
        ok = (cols >= 0) & (cols < n)
        u.append(rows[ok]), v.append(cols[ok])
    empty = np.flatnonzero(lens == 0)
    if name == "er":
        assert {17, 1300} <= set(empty.tolist())
    u.append(np.repeat(empty, 3)), v.append(rng.randint(n, size=3 * len(empty)))      # empty rows
    u.append(np.arange(n)), v.append(np.arange(n))                   # u == v
    u.append(np.full(50, rows[0])), v.append(np.full(50, first[0]))  # one pair many times
    u, v = np.concatenate(u).astype(np.int64), np.concatenate(v).astype(np.int64)
    want = np.asarray(pat[u, v]).reshape(-1) != 0
    assert want.any() and not want.all()
    for dtype in (torch.int64, torch.int32):
        got = engine.pairs_present(csr, torch.from_numpy(u).to(gpu).to(dtype), torch.from_numpy(v).to(gpu).to(dtype))
        assert got.dtype == torch.uint8 and got.shape == (len(u),)
        assert np.array_equal(got.cpu().numpy() != 0, want)
        assert set(np.unique(got.cpu().numpy()).tolist()) <= {0, 1}
    none = engine.pairs_present(csr, torch.empty(0, dtype=torch.int64, device=gpu), torch.empty(0, dtype=torch.int64, device=gpu))
    assert none.numel() == 0


def test_pairs_present_bad_ids(gpu):
    from linkteller_amd import engine, sampling
    adj = _graphs()["hub"]
    n = adj.shape[0]
    csr = sampling.device_pattern_csr(adj)
    good = torch.arange(10, device=gpu)
    for bad in (-1, n, n + 7, 2 ** 40, -2 ** 40):
        for where in (0, 9):
            ids = good.clone()
            ids[where] = bad
            with pytest.raises(IndexError, match="1 pairs"):
                engine.pairs_present(csr, ids, good)
            with pytest.raises(IndexError, match="1 pairs"):
                engine.pairs_present(csr, good, ids)
    # the node-id flag of the probe primitives is untouched, and the next call is served
    engine.node_check()
    assert engine.pairs_present(csr, good, good).shape == (10,)
    with pytest.raises(ValueError):
        engine.pairs_present(csr, good, good[:5])

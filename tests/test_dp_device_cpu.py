"""The device route of the DP graphs without a GPU: the two entry points' declaration / binding / export, the argument checks that
precede any device call, the workspace query, the numpy restatements (dp_device_restate.py) against scipy and the host normalisers
-- they are what test_dp_device_gpu.py holds the kernels against -- and the command line."""
import argparse
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import dp_device_restate as D
import dp_philox_restate as R
from conftest import REPO

NEW = ("lt_sym_csr_workspace_bytes", "lt_sym_csr_from_cells", "lt_normalize_csr")


@pytest.fixture(scope="module")
def lt():
    from linkteller_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


# ---- ABI ------------------------------------------------------------------------------------------------------------------

def test_symbols_exported_declared_and_bound(lt):
    src = open(os.path.join(REPO, "include", "linkteller_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(", code))
    h = lt.lib()
    for name in NEW:
        assert name in declared and name in lt.SIGNATURES and hasattr(h, name), name
    assert h.lt_abi_version() == 5
    for name, code_ in lt.NORM_CODES.items():                 # the enum's values are the binding's
        c_name = {"FirstOrderGCN": "FIRST_ORDER_GCN", "BingGeNormAdj": "BINGGE", "NormAdj": "NORM_ADJ", "AugRWalk": "AUG_RWALK",
                  "RWalk": "RWALK", "AugNormAdj": "AUG_NORM_ADJ"}[name]
        assert re.search(rf"\bLT_NORM_{c_name} = {code_}\b", code), name
    for word in ("inv_pow[s_r]", "np.power", "listed with coin 0", "base_nnz + 2 m"):        # the contract's text
        assert word in src, word


def test_argument_checks_make_no_device_call(lt):
    """Host memory stands in for the device pointers: every call below returns before anything is enqueued or dereferenced
    (this process has no GPU to enqueue on)."""
    h = lt.lib()
    buf = np.zeros(1 << 16, dtype=np.int64)
    p = buf.ctypes.data
    need = h.lt_sym_csr_workspace_bytes(8, 20, 5)
    assert 0 < need <= buf.nbytes

    def sym(n=8, brp=p, bcol=p, bnnz=20, cells=p, coins=p, m=5, orp=p, ocol=p, cap=30, info=p, ws=p, ws_bytes=buf.nbytes):
        return h.lt_sym_csr_from_cells(n, brp, bcol, bnnz, cells, coins, m, orp, ocol, cap, info, ws, ws_bytes, None)

    for kw in (dict(cells=None), dict(orp=None), dict(ocol=None), dict(info=None), dict(ws=None)):
        assert sym(**kw) == -1 and b"NULL" in h.lt_last_error(), kw
    assert sym(brp=None) == -1 and b"both rowptr and col" in h.lt_last_error()
    assert sym(bcol=None) == -1 and b"both rowptr and col" in h.lt_last_error()
    assert sym(brp=None, bcol=None) == -1 and b"without a base" in h.lt_last_error()      # base_nnz = 20 with no base
    assert sym(n=1) == -1 and b"n=1 < 2" in h.lt_last_error()
    assert sym(n=0) == -1 and sym(n=-4) == -1
    assert sym(m=-1) == -1 and b"negative size" in h.lt_last_error()
    assert sym(bnnz=-1) == -1 and b"negative size" in h.lt_last_error()
    assert sym(cap=-1) == -1 and b"capacity" in h.lt_last_error()
    assert sym(bnnz=2 ** 31 - 1 - 10, m=5) == -1 and b"int32 row pointers" in h.lt_last_error()      # base_nnz + 2 m = 2^31 - 1
    assert sym(bnnz=0, m=2 ** 30) == -1 and b"int32 row pointers" in h.lt_last_error()
    assert sym(m=2 ** 62) == -1
    assert sym(ws_bytes=need - 1) == -1 and b"workspace" in h.lt_last_error()
    assert sym(ws_bytes=0) == -1
    assert sym(ws=p + 4) == -1 and b"aligned" in h.lt_last_error()

    def norm(n=8, rp=p, col=p, nnz=20, code=0, inv=p, orp=p, ocol=p, oval=p, cap=28, info=p):
        return h.lt_normalize_csr(n, rp, col, nnz, code, inv, orp, ocol, oval, cap, info, None)

    for kw in (dict(rp=None), dict(col=None), dict(inv=None), dict(orp=None), dict(ocol=None), dict(oval=None), dict(info=None)):
        assert norm(**kw) == -1 and b"NULL" in h.lt_last_error(), kw
    assert norm(n=0) == -1 and b"n=0 < 1" in h.lt_last_error()
    assert norm(nnz=-1) == -1 and b"nnz=-1" in h.lt_last_error()
    assert norm(nnz=2 ** 31) == -1
    assert norm(code=6) == -1 and b"unknown norm 6" in h.lt_last_error()
    assert norm(code=-1) == -1 and b"unknown norm" in h.lt_last_error()
    assert norm(cap=-1) == -1 and b"capacity" in h.lt_last_error()


def test_workspace_query_is_zero_for_bad_arguments_and_linear(lt):
    q = lt.lib().lt_sym_csr_workspace_bytes
    assert q(1, 0, 0) == 0 and q(0, 0, 0) == 0 and q(8, -1, 0) == 0 and q(8, 0, -1) == 0
    assert q(8, 2 ** 31 - 1, 0) == 0 and q(8, 2 ** 31 - 11, 5) == 0 and q(8, 0, 2 ** 30) == 0
    assert q(2, 0, 0) > 0 and q(8, 2 ** 31 - 12, 5) > 0
    # per base entry: the merged column and its flag; per cell: two directed entries of four sort words + those two
    for n in (1 << 10, 1 << 20):
        b0 = q(n, 0, 0)
        assert b0 <= 4 * (n + 1) + 4096                                    # O(n) words: the list's row extents
        for base_nnz, m in ((1 << 20, 0), (0, 1 << 20), (1 << 22, 1 << 21), (1 << 26, 1 << 25)):
            got = q(n, base_nnz, m)
            assert b0 <= got <= b0 + 8 * base_nnz + 48 * m + 4 * 256 * 4096 + (8 * base_nnz + 16 * m) // 1024 + 4096, (n, base_nnz, m, got)
        assert q(n, 1 << 21, 1 << 20) - q(n, 1 << 20, 1 << 20) <= 9 * (1 << 20)                # linear, not more, in the base
    assert q(1 << 30, 1000, 1000) - q(1 << 10, 1000, 1000) <= 4 * (1 << 30)                   # n costs n + 1 words, nothing else


# ---- the restatements against the host ------------------------------------------------------------------------------------------

def _norm_graphs():
    return {"hub+loop+isolated": D.hub_graph(300, 1, hub=17, self_loop=40, isolated=123),
            "loop on the hub": D.hub_graph(130, 2, hub=0, self_loop=0, isolated=129),
            "no loop": D.hub_graph(65, 3, hub=64, isolated=0),
            "single node": sp.csr_matrix((1, 1), dtype=np.int64),
            "single node with a loop": sp.csr_matrix(np.ones((1, 1), dtype=np.int64))}


@pytest.mark.parametrize("name", D.NORMS)
def test_restated_normaliser_equals_the_host_bit_for_bit(name):
    from linkteller_amd import graph
    for tag, a in _norm_graphs().items():
        n = a.shape[0]
        want_n, want_rowptr, want_col, want_val = graph.csr_arrays(graph.fetch_normalization(name)(a))
        rowptr, col, val = D.normalize_csr(name, a.indptr, a.indices, n)
        assert want_n == n and np.array_equal(rowptr, want_rowptr) and np.array_equal(col, want_col), (name, tag)
        assert val.dtype == np.float32 and np.array_equal(val.view(np.uint32), want_val.view(np.uint32)), (name, tag)
        assert np.array_equal(D.inv_pow_table(name, n).view(np.uint64), graph.inv_power_table(name, n).view(np.uint64))
        # d_info[0] of the contract
        diag = int((a.diagonal() != 0).sum())
        assert col.size == a.nnz + (n - diag if name in D.AUG + D.PLUS_ONE else 0)


def test_normalize_device_refuses_unknown_names():
    from linkteller_amd import graph
    with pytest.raises(NotImplementedError, match="not implemented"):
        graph.normalize_device("SymNorm", None, None)
    with pytest.raises(NotImplementedError, match="not implemented"):
        graph.fetch_normalization("SymNorm")
    with pytest.raises(NotImplementedError):
        graph.inv_power_table("SymNorm", 4)


@pytest.mark.parametrize("eps", [5.0, 1.0])
def test_restated_sym_csr_equals_lapgraph_symmetrisation(eps):
    """mat + mat.T of dp._lapgraph_philox, on the cells the stream selects."""
    from linkteller_amd import synth
    n, seed = 257, 42
    adj = sp.csr_matrix(synth.erdos_renyi_graph(n, 600, seed=3))
    n_keep = 600 + int(R.edge_count_draw(seed, eps * 0.01))
    t = R.select(R.cell_keys(n, seed, adj, np.exp(eps - eps * 0.01)), n_keep)[0]
    top = R.flat_index(t, n)
    mat = sp.csr_matrix((np.ones(n_keep, dtype=np.int32), (top // n, top % n)), shape=(n, n))
    want = sp.csr_matrix(mat + mat.T)
    want.sort_indices()
    for cells in (top, top[::-1], np.random.RandomState(0).permutation(top)):
        rowptr, col, info = D.sym_csr_from_cells(n, cells)
        assert np.array_equal(rowptr, want.indptr) and np.array_equal(col, want.indices)
        assert info.tolist() == [2 * n_keep, 0, 0, 0]


@pytest.mark.parametrize("eps", [4.0, 1.0])
def test_restated_sym_csr_equals_edgerand_arithmetic(eps):
    """adj + add - sub with the two fix-ups of dp._edgerand_philox, explicit zeros eliminated."""
    from linkteller_amd import dp, synth
    n, seed = 257, 42
    adj = sp.csr_matrix(synth.erdos_renyi_graph(n, 600, seed=3))
    t, coin = R.edgerand_cells(n, seed, 2 / (np.exp(eps) + 1))
    cell = R.flat_index(t, n)
    i, j = cell // n, cell % n
    add = dp._symmetric_from_upper(j[coin == 1], i[coin == 1], n)
    sub = dp._symmetric_from_upper(j[coin == 0], i[coin == 0], n)
    noisy = sp.csr_matrix(adj + add - sub)
    assert (noisy.data == -1).any() and (noisy.data == 2).any()           # a cleared non-edge and a set edge both occur
    noisy.data[noisy.data == -1] = 0
    noisy.data[noisy.data == 2] = 1
    noisy.eliminate_zeros()
    noisy.sort_indices()
    base = sp.csr_matrix(adj)
    base.sort_indices()
    rowptr, col, info = D.sym_csr_from_cells(n, cell, coin, (base.indptr, base.indices))
    assert np.array_equal(rowptr, noisy.indptr) and np.array_equal(col, noisy.indices)
    assert info.tolist() == [noisy.nnz, 0, 0, 0] and set(np.unique(noisy.data)) == {1}
    cleared_edges = int(np.isin(cell[coin == 0], R.flat_index(np.flatnonzero(R.edge_mask(n, adj, 0, n * (n - 1) // 2)), n)).sum())
    assert cleared_edges > 0                                               # 1 - 1: the pair leaves the graph


def test_restated_sym_csr_counts_bad_and_repeated_cells():
    n = 5
    cells = np.array([1 * n + 0, 3 * n + 2, 3 * n + 2, n * n, 2 * n + 2, 1 * n + 3, -1], dtype=np.int64)
    rowptr, col, info = D.sym_csr_from_cells(n, cells)
    assert info.tolist() == [4, 4, 1, 0]
    assert rowptr.tolist() == [0, 1, 2, 3, 4, 4] and col.tolist() == [1, 0, 3, 2]


# ---- command line and Worker ------------------------------------------------------------------------------------------------

def test_cli_dp_build(monkeypatch):
    from linkteller_amd import main as lt_main, worker
    assert lt_main.get_arguments([]).dp_build == "host"
    assert lt_main.get_arguments(["--dp-build", "device"]).dp_build == "device"
    with pytest.raises(SystemExit):
        lt_main.get_arguments(["--dp-build", "gpu"])

    def no_worker(*a, **k):
        raise AssertionError("a Worker was built")
    monkeypatch.setattr(worker, "Worker", no_worker)
    common = ["--test", "--dataset", "twitch/ES/RU", "--dp-build", "device"]
    for extra in (["--mode", "vanilla"],                                           # numpy noise
                  ["--mode", "vanilla", "--noise-rng", "numpy"],
                  ["--mode", "vanilla-clean", "--noise-rng", "philox"],
                  ["--noise-rng", "philox"]):                                       # the default mode is vanilla-clean
        with pytest.raises(NotImplementedError, match="--dp-build device needs"):
            lt_main.main(common + extra)
    lt_main.check_dp_build(lt_main.get_arguments(["--mode", "vanilla", "--noise-rng", "philox", "--dp-build", "device"]))
    lt_main.check_dp_build(lt_main.get_arguments(["--mode", "vanilla-clean"]))
    lt_main.check_dp_build(argparse.Namespace(mode="vanilla"))                     # a Namespace without the flag: host


def test_worker_reads_dp_build_and_tolerates_its_absence(tmp_path, monkeypatch):
    """Without dp_build (or with 'host') the Worker takes dp.perturb_adj; with 'device' it takes dp.perturb_adj_device."""
    import torch
    from linkteller_amd import dp, graph, synth
    from linkteller_amd.worker import Worker
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    synth.write_musae_dataset(str(tmp_path), "ES", synth.erdos_renyi_graph(40, 90, seed=1), 50, 1)
    synth.write_musae_dataset(str(tmp_path), "RU", synth.erdos_renyi_graph(30, 60, seed=2), 50, 2)
    seen = []

    class Stop(Exception):
        pass

    def host(adj, *a, **k):
        seen.append("host")
        return adj

    def device(adj, *a, **k):
        seen.append("device")
        raise Stop
    monkeypatch.setattr(dp, "perturb_adj", host)
    monkeypatch.setattr(dp, "perturb_adj_device", device)
    base = dict(norm="FirstOrderGCN", perturb_type="continuous", epsilon=5.0, noise_seed=42, noise_type="laplace", delta=1e-5)
    for extra in (dict(), dict(dp_build="host"), dict(dp_build="host", noise_rng="philox")):
        Worker(argparse.Namespace(**base, **extra), dataset="twitch/ES/RU", mode="vanilla", data_root=str(tmp_path))
        assert seen[-2:] == ["host", "host"]
    with pytest.raises(Stop):
        Worker(argparse.Namespace(**base, dp_build="device", noise_rng="philox"), dataset="twitch/ES/RU", mode="vanilla",
               data_root=str(tmp_path))
    assert seen[-1] == "device"
    with pytest.raises(NotImplementedError, match="philox"):
        Worker(argparse.Namespace(**base, dp_build="device"), dataset="twitch/ES/RU", mode="vanilla", data_root=str(tmp_path))
    n_seen = len(seen)
    Worker(argparse.Namespace(**base, dp_build="device", noise_rng="philox"), dataset="twitch/ES/RU", mode="vanilla-clean",
           data_root=str(tmp_path))                                                # a clean graph has nothing to build
    assert len(seen) == n_seen

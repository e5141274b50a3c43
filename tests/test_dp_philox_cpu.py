"""The Philox edge-DP route without a GPU: the command line and the Python surface, the three entry points' export / binding
and the argument checks that precede any device call, and the statistics of the stream's numpy restatement
(dp_philox_restate.py) that the GPU tests compare the kernels with."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import dp_philox_restate as R
from conftest import REPO

NEW = ("lt_philox_cells_scan", "lt_lapgraph_philox_workspace", "lt_lapgraph_philox", "lt_edgerand_philox")
N, SEED = 257, 42
CELLS = N * (N - 1) // 2          # 32 896


@pytest.fixture(scope="module")
def lt():
    from linkteller_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


@pytest.fixture(scope="module")
def stream0():
    """(k, u) of every cell of n = 257, seed 42, stream 0."""
    k, u, _ = R.cell_words(np.arange(CELLS, dtype=np.uint64), SEED, R.STREAM_LAPGRAPH)
    return k, u


def _er(n, e, seed):
    from linkteller_amd import synth
    return sp.csr_matrix(synth.erdos_renyi_graph(n, e, seed=seed))


# ---- command line and surface ----------------------------------------------------------------------------------------------

def test_cli_noise_rng():
    from linkteller_amd import main as lt_main
    assert lt_main.get_arguments([]).noise_rng == "numpy"
    assert lt_main.get_arguments(["--noise-rng", "philox"]).noise_rng == "philox"
    assert lt_main.get_arguments(["--noise-rng", "numpy"]).noise_rng == "numpy"
    with pytest.raises(SystemExit):
        lt_main.get_arguments(["--noise-rng", "mt19937"])


def test_philox_needs_a_gpu_and_refuses_gaussian(lt):
    import torch
    from linkteller_amd import dp
    adj = _er(40, 90, 1)
    for perturb in ("continuous", "discrete"):
        if not torch.cuda.is_available():
            with pytest.raises(lt.LinkTellerHipError, match="no HIP device"):
                dp.perturb_adj(adj, perturb, 5.0, 42, rng="philox")
    with pytest.raises(NotImplementedError, match="gaussian"):
        dp.perturb_adj(adj, "continuous", 5.0, 42, noise_type="gaussian", rng="philox")
    with pytest.raises(NotImplementedError):
        dp.perturb_adj_continuous(adj, 5.0, 42, noise_type="gaussian", rng="philox")
    with pytest.raises(ValueError, match="rng"):
        dp.perturb_adj(adj, "continuous", 5.0, 42, rng="torch")
    with pytest.raises(ValueError, match="rng"):
        dp.perturb_adj_discrete(adj, 5.0, 42, rng="torch")


def test_worker_reads_noise_rng_and_tolerates_its_absence(tmp_path, monkeypatch):
    """Worker.prepare_data hands args.noise_rng to dp.perturb_adj, and 'numpy' when the Namespace has no such attribute."""
    import torch
    from linkteller_amd import dp, synth
    from linkteller_amd.worker import Worker
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    synth.write_musae_dataset(str(tmp_path), "ES", synth.erdos_renyi_graph(40, 90, seed=1), 50, 1)
    synth.write_musae_dataset(str(tmp_path), "RU", synth.erdos_renyi_graph(30, 60, seed=2), 50, 2)
    seen = []

    def fake(adj, *a, rng="numpy", **k):
        seen.append(rng)
        return adj
    monkeypatch.setattr(dp, "perturb_adj", fake)
    for extra, want in ((dict(), "numpy"), (dict(noise_rng="philox"), "philox")):
        args = argparse.Namespace(norm="FirstOrderGCN", perturb_type="continuous", epsilon=5.0, noise_seed=42,
                                  noise_type="laplace", delta=1e-5, **extra)
        Worker(args, dataset="twitch/ES/RU", mode="vanilla", data_root=str(tmp_path))
        assert seen[-2:] == [want, want]


def test_host_draws_equal_the_restatement():
    from linkteller_amd import dp
    for seed in (42, (5 << 32) | 1234, 0, 2 ** 64 - 1):
        for eps1 in (0.05, 0.01):
            assert dp.philox_edge_count_draw(seed, eps1) == R.edge_count_draw(seed, eps1)
    for eps in (4.0, 7.0, 0.1):
        s = 2 / (np.exp(eps) + 1)
        assert dp.edgerand_threshold(s) == R.edgerand_threshold(s) and 0 < dp.edgerand_threshold(s) < 2 ** 52


# ---- ABI ------------------------------------------------------------------------------------------------------------------

def test_symbols_exported_declared_and_bound(lt):
    src = open(os.path.join(REPO, "include", "linkteller_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(", code))
    h = lt.lib()
    for name in NEW:
        assert name in declared and name in lt.SIGNATURES and hasattr(h, name), name
    assert h.lt_abi_version() == 5
    for word in ("t = i (i - 1) / 2 + j", "(2 k + 1) 2^-53", "s_threshold", "key descending"):      # the stream's definition
        assert word in src, word


def test_argument_checks_make_no_device_call(lt):
    """Host memory stands in for the device pointers: every call below returns before anything is enqueued or dereferenced
    (this process has no GPU to enqueue on)."""
    h = lt.lib()
    buf = np.zeros(1 << 16, dtype=np.int64)
    p = buf.ctypes.data
    info = np.zeros(8, dtype=np.int64)

    def scan(n=8, r0=0, r1=8, rowptr=p, col=p, factor=2.0, key_min=1.0, cell=p, key=p, cap=16, count=p):
        return h.lt_philox_cells_scan(n, r0, r1, rowptr, col, 42, factor, key_min, cell, key, cap, count, None)

    for kw in (dict(rowptr=None), dict(col=None), dict(cell=None), dict(key=None), dict(count=None)):
        assert scan(**kw) == -1 and b"NULL" in h.lt_last_error(), kw
    assert scan(n=1, r1=1) == -1 and b"n < 2" in h.lt_last_error()
    assert scan(r0=5, r1=4) == -1 and b"row_begin" in h.lt_last_error()
    assert scan(r0=-1) == -1 and scan(r1=9) == -1
    assert scan(cap=-1) == -1 and b"capacity" in h.lt_last_error()
    assert scan(factor=-1.0) == -1 and scan(factor=float("inf")) == -1 and scan(key_min=-1.0) == -1
    assert scan(key_min=float("nan")) == -1 and b"key_min" in h.lt_last_error()

    def erand(n=8, r0=0, r1=8, thr=1 << 40, cell=p, coin=p, cap=16, count=p):
        return h.lt_edgerand_philox(n, r0, r1, 42, thr, cell, coin, cap, count, None)

    for kw in (dict(cell=None), dict(coin=None), dict(count=None)):
        assert erand(**kw) == -1 and b"NULL" in h.lt_last_error(), kw
    assert erand(n=1, r1=1) == -1 and erand(n=0, r1=0) == -1
    assert erand(r0=5, r1=4) == -1 and b"row_begin" in h.lt_last_error()
    assert erand(r1=9) == -1 and erand(cap=-2) == -1
    assert erand(thr=(1 << 52) + 1) == -1 and b"2^52" in h.lt_last_error()

    need = C.c_size_t(0)
    assert h.lt_lapgraph_philox_workspace(8, 20, 5, C.byref(need)) == 0 and 0 < need.value <= buf.nbytes
    need8 = need.value

    def lap(n=8, rowptr=p, col=p, factor=2.0, keep=5, out=p, inf=info.ctypes.data, ws=p, ws_bytes=buf.nbytes):
        return h.lt_lapgraph_philox(n, rowptr, col, 42, factor, keep, 0.0, out, inf, ws, ws_bytes, None)

    for kw in (dict(rowptr=None), dict(col=None), dict(out=None), dict(inf=None), dict(ws=None)):
        assert lap(**kw) == -1 and b"NULL" in h.lt_last_error(), kw
    assert lap(n=1, keep=1) == -1 and b"n < 2" in h.lt_last_error()
    assert lap(keep=0) == -1 and b"outside" in h.lt_last_error()
    assert lap(keep=29) == -1 and b"[1, 28]" in h.lt_last_error()
    assert lap(keep=-3) == -1
    assert lap(factor=-0.5) == -1 and b"edge_factor" in h.lt_last_error()
    assert lap(ws_bytes=need8 - 1) == -1 and b"workspace" in h.lt_last_error()
    assert lap(ws=p + 4) == -1 and b"aligned" in h.lt_last_error()
    assert lap(ws_bytes=0) == -1


def test_workspace_is_linear_and_not_quadratic(lt):
    h = lt.lib()

    def q(n, nnz, keep):
        b = C.c_size_t(7)
        rc = h.lt_lapgraph_philox_workspace(n, nnz, keep, C.byref(b))
        return rc, b.value

    assert q(1, 0, 1) == (-1, 0) and q(8, -1, 1) == (-1, 0) and q(8, 10, 0) == (-1, 0) and q(8, 10, 29) == (-1, 0)
    assert h.lt_lapgraph_philox_workspace(8, 10, 1, None) == -1
    assert q(2, 0, 1)[0] == 0 and q(8, 10, 28)[0] == 0
    keep, nnz = 40000, 80000
    n = 1 << 10
    while n < (1 << 30):                      # at most 16 bytes per node when n doubles at fixed n_keep and nnz
        (r0, b0), (r1, b1) = q(n, nnz, keep), q(2 * n, nnz, keep)
        assert r0 == 0 and r1 == 0 and b1 - b0 <= 16 * n, (n, b0, b1)
        n *= 2
    # linear in n_keep, and the R-MAT size (2 M nodes, 33.5 M kept edges) asks for gigabytes, not for n^2
    b_small, b_big = q(1 << 21, 1 << 26, 1 << 20)[1], q(1 << 21, 1 << 26, 1 << 25)[1]
    assert b_big <= 32 * b_small + 4096 and b_big < 4 << 30


# ---- the restatement's statistics -------------------------------------------------------------------------------------------

def test_uniforms_are_exact_and_open(stream0):
    k, u = stream0
    assert k.max() < (1 << 52) and np.all((u > 0) & (u < 1))
    assert np.array_equal((u * 2.0 ** 53).astype(np.uint64), 2 * k + 1)            # (2k + 1) 2^-53 is exact


def test_laplace_moments_within_5_sigma(stream0):
    """Laplace(0, 1): variance 2, fourth moment 24, so the sample mean has sigma sqrt(2 / M) and the sample variance
    sqrt((24 - 4) / M).  Measured: mean 0.0072, variance 1.9849."""
    lap = R.laplace_unit(*stream0)
    print("mean", lap.mean(), "variance", lap.var())
    assert abs(lap.mean()) <= 5 * np.sqrt(2 / CELLS)
    assert abs(lap.var() - 2) <= 5 * np.sqrt(20 / CELLS)


@pytest.mark.parametrize("eps", [5.0, 1.0])
def test_key_order_is_the_order_of_adjacency_plus_noise(stream0, eps):
    adj = _er(N, 600, 3)
    eps2 = eps - eps * 0.01
    n_keep = 600 + int(R.edge_count_draw(SEED, eps * 0.01))
    assert 1 <= n_keep <= CELLS
    keys = R.cell_keys(N, SEED, adj, np.exp(eps2))
    picked = np.zeros(CELLS, dtype=bool)
    picked[R.select(keys, n_keep)[0]] = True
    value = R.edge_mask(N, adj, 0, CELLS).astype(np.float64) + R.laplace_unit(*stream0) / eps2
    assert picked.sum() == n_keep and value[picked].min() > value[~picked].max()   # no selected / unselected pair inverted
    assert np.array_equal(np.sort(np.argsort(-value, kind="stable")[:n_keep]), np.flatnonzero(picked))


@pytest.mark.parametrize("eps", [4.0, 7.0])
def test_edgerand_counts_within_5_sigma(eps):
    s = 2 / (np.exp(eps) + 1)
    t, coin = R.edgerand_cells(N, SEED, s)
    m = t.size
    print("re-drawn", m, "of", CELLS, "expected", CELLS * s, "ones", int(coin.sum()))
    assert abs(m - CELLS * s) <= 5 * np.sqrt(CELLS * s * (1 - s))
    assert abs(int(coin.sum()) - CELLS * s / 2) <= 5 * np.sqrt(CELLS * (s / 2) * (1 - s / 2))
    assert np.all(np.diff(t) > 0) and set(np.unique(coin)) <= {0, 1}
    lo, hi = R.edgerand_cells(N, SEED, s, rows=(0, 100)), R.edgerand_cells(N, SEED, s, rows=(100, N))
    assert np.array_equal(np.concatenate([lo[0], hi[0]]), t) and np.array_equal(np.concatenate([lo[1], hi[1]]), coin)


def test_streams_differ_and_cells_invert():
    t = np.arange(CELLS, dtype=np.uint64)
    k0, k2 = R.cell_words(t, SEED, 0)[0], R.cell_words(t, SEED, 2)[0]
    assert (k0 == k2).sum() == 0
    assert (R.cell_words(t, SEED + 1, 0)[0] == k0).sum() == 0
    i, j = R.cell_ij(t.astype(np.int64))
    assert np.array_equal(R.cell_t(i, j), t.astype(np.int64)) and i.max() == N - 1
    big = np.array([R.tri(131072) - 1, R.tri(131072), R.tri(131073) - 1, R.tri(2 ** 31 - 1) - 1], dtype=np.int64)
    bi, bj = R.cell_ij(big)
    assert bi.tolist() == [131071, 131072, 131072, 2 ** 31 - 2] and bj.tolist() == [131070, 0, 131071, 2 ** 31 - 3]

"""lt_influence3_pairs on the device: the scores of a LIST of (probe, observed) pairs for the 3-layer model.

What is pinned here:
  * the same BITS as the rectangle: ``Baseline3.influence_pairs`` equals ``influence_rows(probes, pool)`` read at the listed cells
    for the same mode -- narrow handles in `delta`, `sparse` and `full`, wide handles in `delta` -- under forced probe chunking
    (one probe per chunk: chunks that own no pair; a few probes per chunk) and from run to run;
  * `delta` within 1e-5 of the largest score of the fp64 oracle (oracle.linkteller_oracle.influence_matrix with gcn3_forward,
    the block test_gcn3_wide_attack_gpu._ref64 computes once per process) -- the bound of every `delta` test of this suite -- with
    exact zeros where the oracle has them;
  * the workspace bound the header states, the refusals, a weight update, and the attacker's list consumers end to end.

The pair list of a graph is built from the graph's own ``probes`` / ``obs`` lists (test_gcn3_wide_attack_gpu._graph), so the
oracle block covers it: probes that own 0, 1, 3 and 40 pairs, the repeated probe, u == v, a pair listed twice, the probe whose
feature row is all zero, and one probe that observes EVERY node of ``obs`` (on `hub`: every hub row)."""
import argparse
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, csr_from
from linkteller_amd import _lib
from test_gcn3_wide_attack_gpu import KEYS, _graph, _params, _ref64, _wide3
from test_pairs_gpu import _from_rect

pytestmark = pytest.mark.gpu

DELTA = 1e-4
NARROW = ((16, 12, 2), (20, 12, 3), (256, 64, 8))          # the three CP instantiations, the widest hidden layers
WIDE = ((16, 12, 9), (32, 16, 121), (256, 64, 256))        # distinct lt_lpr_for(Cp); the largest class layer
BOTH = (20, 12, 8)                                         # the narrow and the wide kernels on the same 8-class model
GRAPHS = ("er", "loops", "hub")
CASES = [(s, False) for s in NARROW + (BOTH,)] + [(s, True) for s in WIDE + (BOTH,)]
LT_ERR_INVALID, LT_ERR_UNSUPPORTED, LT_ERR_INDEX = -1, -3, -6
LIST_SEED = 5


def _case_id(c):
    return "x".join(map(str, c[0])) + ("w" if c[1] else "")


@functools.lru_cache(maxsize=None)
def _pairs(name):
    """(pair_ptr [P + 1], pair_obs [M] node ids, col [M]: pair k observes obs[col[k]], row [M]: its probe's place in probes)."""
    _, _, probes, obs, zrow = _graph(name)
    rng = np.random.RandomState(LIST_SEED)
    n_p, n_o = len(probes), len(obs)
    counts = rng.choice([0, 0, 1, 3, 10], n_p)
    counts[:4] = (0, 1, 3, 40)                              # the first four probes: no pair, one, three, forty
    rep = [i for i in range(n_p) if (probes[:i] == probes[i]).any()][0]
    counts[rep] = max(counts[rep], 3)                       # the repeated probe owns pairs at both of its places
    first = int(np.flatnonzero(probes == probes[rep])[0])
    if first > 3:
        counts[first] = max(counts[first], 3)
    if zrow > 3:
        counts[zrow] = max(counts[zrow], 3)                 # the all-zero feature row
    ptr, col = [0], []
    same = 0
    for i in range(n_p):
        cnt = int(counts[i])
        mine = list(rng.randint(0, n_o, cnt))
        if cnt == 40:
            mine = [k % n_o for k in range(cnt)]            # every node of obs is observed by this probe
        own = np.flatnonzero(obs == probes[i])
        if cnt >= 3 and cnt != 40:
            if len(own):
                mine[1] = int(own[0])                       # u == v
            mine[2] = mine[0]                               # the same pair twice
        same += sum(int(obs[j] == probes[i]) for j in mine)
        col += mine
        ptr.append(len(col))
    ptr, col = np.asarray(ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    row = np.repeat(np.arange(n_p), np.diff(ptr))
    own_counts = set(np.diff(ptr).tolist())
    assert {0, 1, 3, 40} <= own_counts and same > 0 and set(col.tolist()) == set(range(n_o))
    assert counts[zrow] > 0 and counts[rep] > 0
    return ptr, obs[col].astype(np.int32), col, row


def _ref_cells(name, shape):
    ptr, pobs, col, row = _pairs(name)
    return _ref64(name, shape)[row, col]


def _baseline(name, shape, wide, gpu):
    from linkteller_amd import engine, graph
    a_hat, x, *_ = _graph(name)
    p = _params(shape)
    dev = [torch.from_numpy(np.asarray(p[k])).to(gpu) for k in KEYS]
    make = _wide3 if wide else engine.Baseline3
    base = make(graph.HipGraph(a_hat), torch.from_numpy(x).to(gpu), *dev)
    assert base.wide == wide
    return base, dev


def _rect_cells(base, name, mode):
    _, _, probes, obs, _ = _graph(name)
    ptr, pobs, col, row = _pairs(name)
    pool = np.unique(obs)
    rect = base.influence_rows(probes, pool, DELTA, mode).cpu().numpy()
    return _from_rect(rect, ptr, pobs, pool)


# ---- 1. the bits of the rectangle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_pairs_are_the_bits_of_the_rectangle(gpu, name, case):
    shape, wide = case
    _, _, probes, obs, _ = _graph(name)
    ptr, pobs, col, row = _pairs(name)
    base, _ = _baseline(name, shape, wide, gpu)
    lib = _lib.lib()
    modes = ("delta",) if wide else ("delta", "sparse")
    want = {}
    for mode in modes:
        got = base.influence_pairs(probes, ptr, pobs, DELTA, mode)
        assert got.shape == (len(pobs),) and got.dtype == torch.float32
        want[mode] = got.cpu().numpy()
        assert np.array_equal(want[mode], _rect_cells(base, name, mode)), (mode, np.abs(want[mode] - _rect_cells(base, name, mode)).max())
        assert np.array_equal(base.influence_pairs(probes, ptr, pobs, DELTA, mode).cpu().numpy(), want[mode])      # two runs
        assert (want[mode] > 0).any()
    if not wide:
        assert np.array_equal(base.influence_pairs(probes, ptr, pobs, DELTA, "full").cpu().numpy(), want["sparse"])
        assert np.array_equal(_rect_cells(base, name, "full"), want["sparse"])
    # forced chunking: one probe per chunk (the probes without pairs make chunks that own none), then a few probes per chunk
    n_p, n_m = len(probes), len(pobs)
    need1 = lib.lt_influence3_pairs_workspace_bytes(base._h, 1, 1)
    need_all = lib.lt_influence3_pairs_workspace_bytes(base._h, n_p, n_m)
    try:
        _lib.set_tuning("chunk_budget_bytes", 1)
        need_one = lib.lt_influence3_pairs_workspace_bytes(base._h, n_p, n_m)
        assert need_one < need_all
        for mode in modes:
            assert np.array_equal(base.influence_pairs(probes, ptr, pobs, DELTA, mode).cpu().numpy(), want[mode]), mode
            assert np.array_equal(_rect_cells(base, name, mode), want[mode]), mode
        _lib.set_tuning("chunk_budget_bytes", 2 * need1)
        need_few = lib.lt_influence3_pairs_workspace_bytes(base._h, n_p, n_m)
        assert need_one < need_few < need_all, (need_one, need_few, need_all)       # more than one probe per chunk, not all of them
        for mode in modes:
            assert np.array_equal(base.influence_pairs(probes, ptr, pobs, DELTA, mode).cpu().numpy(), want[mode]), mode
    finally:
        _lib.set_tuning("chunk_budget_bytes", None)
    from linkteller_amd import engine
    torch.cuda.synchronize()
    engine.node_check()


# ---- 2. the fp64 oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_delta_pairs_against_the_fp64_oracle(gpu, name, case):
    shape, wide = case
    _, _, probes, obs, zrow = _graph(name)
    ptr, pobs, col, row = _pairs(name)
    ref = _ref_cells(name, shape)
    zeros = float((ref == 0).mean())
    if name == "er":
        assert 0.1 <= zeros <= 0.9, zeros              # a condition of the zero check below, not a measurement
    base, _ = _baseline(name, shape, wide, gpu)
    got = base.influence_pairs(probes, ptr, pobs, DELTA, "delta").cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max() / ref.max()
    print(f"gcn3 pairs {name} {_case_id(case)}: {len(ref)} pairs, max {ref.max():.3g} zeros {zeros:.2f} |ours - ref64| / max = {err:.2e}")
    assert ref.max() > 0 and np.isfinite(got).all()
    assert err <= 1e-5
    assert np.all(got[ref == 0] == 0) and not np.signbit(got).any()
    assert (row == zrow).any() and np.all(ref[row == zrow] == 0) and np.all(got[row == zrow] == 0)


# ---- 3. the workspace -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_workspace_is_sized_by_the_list(gpu, wide):
    """lt_influence3_pairs_workspace_bytes(b, P, M) <= lt_influence3_workspace_bytes(b, P, 1) + 4 M + 8 (P + 1) + 512 (the
    header's bound: the checked pair_obs, the offsets' device copy, two 256-byte roundings), whatever nodes the list names: a
    call with exactly that many bytes serves a list of one distinct node and a list of all of them."""
    from linkteller_amd import engine
    lib = _lib.lib()
    base, _ = _baseline("er", (16, 12, 9) if wide else (20, 12, 3), wide, gpu)
    n = base.n
    for n_p, n_m in ((1, 1), (25, 137), (25, 4 * n), (300, 1_000_000), (1024, 40_000)):
        need = lib.lt_influence3_pairs_workspace_bytes(base._h, n_p, n_m)
        rows1 = lib.lt_influence3_workspace_bytes(base._h, n_p, 1)
        assert 0 < need <= rows1 + 4 * n_m + 8 * (n_p + 1) + 512, (n_p, n_m, need, rows1)
        assert need >= 4 * n_m + 8 * (n_p + 1)
    # ... nothing of the size of n_probe x (nodes observed): all n nodes observed by every probe's list, 25 probes
    n_p, n_m = 25, 4 * n
    assert lib.lt_influence3_pairs_workspace_bytes(base._h, n_p, n_m) < lib.lt_influence3_workspace_bytes(base._h, n_p, 1) + 4 * n_p * n
    base.enable_fp64()
    probes = torch.arange(n_p, dtype=torch.int32, device=gpu)
    ptr = np.arange(n_p + 1, dtype=np.int64) * (n_m // n_p)
    need = lib.lt_influence3_pairs_workspace_bytes(base._h, n_p, n_m)
    ws = engine._workspace(need, gpu)
    outs = []
    for pobs in (torch.full((n_m,), 7, dtype=torch.int32, device=gpu),
                 (torch.arange(n_m, dtype=torch.int32, device=gpu) * 7) % n):
        out = torch.empty(n_m, dtype=torch.float32, device=gpu)
        assert lib.lt_influence3_pairs(base._h, probes.data_ptr(), n_p, ptr.ctypes.data, pobs.data_ptr(), n_m, DELTA, _lib.MODE_DELTA,
                                       out.data_ptr(), ws.data_ptr(), need, engine._stream()) == 0
        rect = base.influence_rows(probes, torch.arange(n, dtype=torch.int32, device=gpu), DELTA, "delta")
        rows = torch.repeat_interleave(torch.arange(n_p, device=gpu), n_m // n_p)
        assert torch.equal(out, rect[rows, pobs.long()])
        outs.append(out)
    assert lib.lt_influence3_pairs(base._h, probes.data_ptr(), n_p, ptr.ctypes.data, pobs.data_ptr(), n_m, DELTA, _lib.MODE_DELTA,
                                   out.data_ptr(), ws.data_ptr(), need - 256, engine._stream()) == -4          # LT_ERR_WORKSPACE
    torch.cuda.synchronize()
    engine.node_check()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_calls(gpu):
    from linkteller_amd import engine
    lib = _lib.lib()
    _, _, probes, obs, _ = _graph("er")
    ptr, pobs, col, row = _pairs("er")
    base, _ = _baseline("er", (20, 12, 3), False, gpu)
    wide, _ = _baseline("er", (16, 12, 9), True, gpu)
    n, n_p, n_m = base.n, len(probes), len(pobs)
    pt, ot = torch.from_numpy(probes).to(gpu), torch.from_numpy(pobs).to(gpu)
    out = torch.full((n_m,), -7.0, dtype=torch.float32, device=gpu)
    ws = engine._workspace(max(lib.lt_influence3_pairs_workspace_bytes(b._h, n_p, n_m) for b in (base, wide)), gpu)

    def raw(b, mode, ptr_=ptr, n_probe=n_p, n_pairs=n_m):
        return lib.lt_influence3_pairs(b._h, pt.data_ptr(), n_probe, None if ptr_ is None else ptr_.ctypes.data, ot.data_ptr(), n_pairs,
                                       DELTA, mode, out.data_ptr(), ws.data_ptr(), ws.numel(), engine._stream())
    # `delta` before lt_baseline3_enable_fp64
    assert raw(base, _lib.MODE_DELTA) == LT_ERR_INVALID and "lt_baseline3_enable_fp64" in lib.lt_last_error().decode()
    assert raw(wide, _lib.MODE_DELTA) == LT_ERR_INVALID and "lt_baseline3_enable_fp64" in lib.lt_last_error().decode()
    # a wide handle outside `delta`
    for mode in (_lib.MODE_SPARSE, _lib.MODE_FULL):
        assert raw(wide, mode) == LT_ERR_UNSUPPORTED and "wide handle" in lib.lt_last_error().decode()
    for mode in ("sparse", "full"):
        with pytest.raises(NotImplementedError):
            wide.influence_pairs(probes, ptr, pobs, DELTA, mode)
    wide.enable_fp64()
    assert raw(wide, _lib.MODE_SPARSE) == LT_ERR_UNSUPPORTED             # ... with the fp64 baseline too
    # empty calls: LT_OK, nothing launched
    zeros = np.zeros(n_p + 1, dtype=np.int64)
    assert raw(base, _lib.MODE_SPARSE, ptr_=zeros, n_pairs=0) == 0
    assert raw(base, _lib.MODE_SPARSE, ptr_=zeros[:1], n_probe=0, n_pairs=0) == 0
    assert lib.lt_influence3_pairs(base._h, None, 0, None, None, 0, DELTA, _lib.MODE_SPARSE, None, None, 0, None) == 0
    assert base.influence_pairs(probes, zeros, [], DELTA, "delta").numel() == 0
    assert base.influence_pairs([], [0], [], DELTA, "sparse").numel() == 0
    # pair_ptr that is no offset array (the four of test_pairs_gpu.test_pairs_refusals_and_empty_calls); NULL with pairs
    for b, mode in ((base, "delta"), (base, "sparse"), (wide, "delta")):
        for wrong in (ptr[::-1].copy(), np.concatenate([[1], ptr[1:]]), np.concatenate([ptr[:-1], [ptr[-1] + 1]]),
                      np.concatenate([ptr[:3], [ptr[2] - 1], ptr[4:]])):
            with pytest.raises(_lib.LinkTellerHipError):
                b.influence_pairs(probes, wrong, pobs, DELTA, mode, out=out)
    assert raw(base, _lib.MODE_SPARSE, ptr_=None) == LT_ERR_INVALID
    with pytest.raises(ValueError):
        base.influence_pairs(probes, ptr[:-1], pobs, DELTA)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                     # nothing was written by any of them
    engine.node_check()
    # ids out of range: clamped on the device (the call completes), reported afterwards; the flag then clears
    good = {id(b): b.influence_pairs(probes, ptr, pobs, DELTA, "delta").clone() for b in (base, wide)}
    for b in (base, wide):
        for which, bad in (("probe", n), ("observed", n + 12345), ("probe", -1), ("observed", 2 ** 31 - 1)):
            p2, o2 = probes.copy(), pobs.copy()
            (p2 if which == "probe" else o2)[2] = bad
            got = b.influence_pairs(torch.from_numpy(p2).to(gpu), ptr, torch.from_numpy(o2).to(gpu), DELTA, "delta")
            torch.cuda.synchronize()
            assert torch.isfinite(got).all()
            with pytest.raises(IndexError):
                engine.node_check()
            engine.node_check()
        assert torch.equal(b.influence_pairs(pt, ptr, ot, DELTA, "delta"), good[id(b)])
    # a flag nobody collected refuses the next call (which reports it, enqueues nothing and clears it)
    p2 = probes.copy()
    p2[0] = n
    base.influence_pairs(torch.from_numpy(p2).to(gpu), ptr, ot, DELTA, "sparse")
    torch.cuda.synchronize()
    assert raw(base, _lib.MODE_SPARSE) == LT_ERR_INDEX and "out of range" in lib.lt_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    engine.node_check()
    assert raw(base, _lib.MODE_SPARSE) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), base.influence_pairs(pt, ptr, ot, DELTA, "sparse").cpu().numpy())
    engine.node_check()


# ---- 5. the weights ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((20, 12, 3), False), ((16, 12, 9), True)], ids=_case_id)
def test_pairs_follow_a_weight_update(gpu, case):
    shape, wide = case
    _, _, probes, obs, _ = _graph("er")
    ptr, pobs, col, row = _pairs("er")
    base, dev = _baseline("er", shape, wide, gpu)
    for mode in ("delta",) if wide else ("delta", "sparse"):
        before = base.influence_pairs(probes, ptr, pobs, DELTA, mode).cpu().numpy()
        with torch.no_grad():
            dev[0].mul_(1.25)                # W1
            dev[4].add_(0.01)                # W3
        base.refresh()
        after = base.influence_pairs(probes, ptr, pobs, DELTA, mode).cpu().numpy()
        assert np.array_equal(after, _rect_cells(base, "er", mode))
        assert not np.array_equal(after, before)


# ---- 6. the attacker --------------------------------------------------------------------------------------------------------
def _world(gpu, prefix_adj, xkey):
    from linkteller_amd import graph
    g = np.load(os.path.join(GOLDEN, "next_rows.npz"), allow_pickle=False)
    a = csr_from(g, prefix_adj)
    x = torch.from_numpy(g[xkey]).to(gpu)
    adj_t = graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(a)).to(gpu)
    return g, a, types.SimpleNamespace(features_2=x, adj_2=adj_t, adj_ori=a, n_nodes=a.shape[0])


def _model(gpu, g, kind):
    from linkteller_amd.gcn import GCN3
    if kind == "gcn3":
        model = GCN3(64, 32, 16, 2, 0.5)
        model.load_state_dict({k: torch.from_numpy(g[f"gcn3.sd.{k}"]) for k in
                               ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias", "gc3.weight", "gc3.bias")})
    else:
        torch.manual_seed(7)
        model = GCN3(64, 16, 12, 41, 0.5)
    return model.to(gpu).eval()


class _Spy:
    def __init__(self, monkeypatch):
        from linkteller_amd import engine
        self.rows = self.pairs = 0
        rows, pairs = engine.Baseline3.influence_rows, engine.Baseline3.influence_pairs

        def spy_rows(base, *a, **k):
            self.rows += 1
            return rows(base, *a, **k)

        def spy_pairs(base, *a, **k):
            self.pairs += 1
            return pairs(base, *a, **k)
        monkeypatch.setattr(engine.Baseline3, "influence_rows", spy_rows)
        monkeypatch.setattr(engine.Baseline3, "influence_pairs", spy_pairs)


ATTACKS = [("gcn3", "delta"), ("gcn3", "sparse"), ("gcn3w", "delta")]


@pytest.mark.parametrize("kind,mode", ATTACKS)
def test_naive_attack_takes_the_pair_list(gpu, tmp_path, monkeypatch, kind, mode):
    from test_metrics_gpu import _against_the_file
    from linkteller_amd import engine
    from linkteller_amd.attacker import Attacker
    g, a, w = _world(gpu, "adj", "x")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("LT_INFLUENCE_MODE", raising=False)
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=32, sample_seed=42, influence=DELTA,
                              mode="vanilla-clean", attack_mode="naive", influence_mode=mode)
    atk = Attacker(args, _model(gpu, g, kind), w)
    atk.prepare_test_data()
    assert atk._walk()[0] == kind
    spy = _Spy(monkeypatch)
    name = atk.naive_result_filename()
    _against_the_file(atk, atk.link_prediction_attack, name)          # the attack, then evaluate(): the file's curves, auc, ap
    assert spy.rows == 0 and spy.pairs == 3                             # existing pairs, the others, evaluate()
    pred = np.asarray(torch.load(name, weights_only=False)["result"]["pred"])
    # the rectangle route for the same pairs: perturb v, observe u
    nodes = np.asarray(atk.test_nodes, dtype=np.int64)
    rows = atk._rows(nodes, nodes).cpu().numpy().astype(np.float64)
    assert spy.rows == 1
    ind = {int(v): i for i, v in enumerate(nodes)}
    pairs = np.concatenate([np.asarray(atk.exist_edges).reshape(-1, 2), np.asarray(atk.nonexist_edges).reshape(-1, 2)])
    want = np.array([rows[ind[int(v)], ind[int(u)]] for u, v in pairs])
    assert pred.shape == want.shape and np.array_equal(pred, want) and (pred > 0).any()
    # ... and the fallback of pair_scores itself, called directly
    nd, ptr, obs, order = engine.group_pairs(pairs[:, 1], pairs[:, 0])
    rect = atk._pair_scores_rect(nd, ptr, obs, order, np.empty(len(pairs)), chunk=7)
    assert np.array_equal(rect, pred) and spy.pairs == 3


@pytest.mark.parametrize("kind,mode", ATTACKS)
def test_balanced_full_takes_the_pair_list(gpu, tmp_path, monkeypatch, kind, mode):
    from test_metrics_gpu import _against_the_file
    from linkteller_amd.attacker import Attacker
    g, ab, w = _world(gpu, "bf.adj", "bf.x")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("LT_INFLUENCE_MODE", raising=False)
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="balanced-full", n_test=7, sample_seed=82, influence=DELTA,
                              mode="vanilla-clean", attack_mode="efficient", influence_mode=mode)
    atk = Attacker(args, _model(gpu, g, kind), w)
    atk.prepare_test_data()
    spy = _Spy(monkeypatch)
    name = atk.result_filename()
    _against_the_file(atk, atk.link_prediction_attack_efficient_balanced, name)
    assert spy.rows == 0 and spy.pairs == 2                             # the attack, evaluate()
    pred = np.asarray(torch.load(name, weights_only=False)["result"]["pred"])
    # the computation of attacker.py:250-284 through the rectangle, restated (test_pairs_gpu.test_balanced_full_pred_is_unchanged)
    ex = np.asarray(atk.exist_edges, dtype=np.int64).reshape(-1, 2)
    nex = np.asarray(atk.nonexist_edges, dtype=np.int64).reshape(-1, 2)
    n = ab.shape[0]
    starts = np.union1d(ex[:, 0], nex[:, 0])
    rows = atk._rows(starts, np.arange(n, dtype=np.int64)).cpu().numpy().astype(np.float64)
    assert spy.rows == 1
    pos = np.full(n, -1, dtype=np.int64)
    pos[starts] = np.arange(len(starts))
    s_ex, s_nex = rows[pos[ex[:, 0]], ex[:, 1]], rows[pos[nex[:, 0]], nex[:, 1]]
    want = np.concatenate([s_ex[np.argsort(ex[:, 0], kind="stable")], s_nex[np.argsort(nex[:, 0], kind="stable")]])
    assert pred.shape == want.shape and np.array_equal(pred, want) and (pred > 0).any()


@pytest.mark.parametrize("kind,mode", ATTACKS)
def test_philox_pair_lists_stay_on_the_device(gpu, monkeypatch, kind, mode):
    from linkteller_amd import engine
    from linkteller_amd.attacker import Attacker
    g, ab, w = _world(gpu, "bf.adj", "bf.x")
    monkeypatch.delenv("LT_INFLUENCE_MODE", raising=False)
    for am in ("efficient", "naive"):
        args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="balanced-full", n_test=7, sample_seed=82, influence=DELTA,
                                  mode="vanilla-clean", attack_mode=am, influence_mode=mode)
        atk = Attacker(args, _model(gpu, g, kind), w)
        atk.prepare_test_data(rng="philox")
        with monkeypatch.context() as m:
            spy = _Spy(m)
            m.setattr(Attacker, "_materialise_pairs", lambda self: pytest.fail("the host lists were built"))
            out = atk.evaluate()
            assert spy.rows == 0 and spy.pairs == 1
        assert "_exist_edges" not in atk.__dict__                        # the lists stayed on the device
        # the host-list route for the same pairs
        ex, nex = atk.exist_edges, atk.nonexist_edges
        p, o = (1, 0) if am == "naive" else (0, 1)
        labels = np.zeros(len(ex) + len(nex), dtype=np.uint8)
        labels[:len(ex)] = 1
        ref = atk._pair_curve(np.concatenate([ex[:, p], nex[:, p]]), np.concatenate([ex[:, o], nex[:, o]]), labels).summary()
        engine.node_check()
        assert out["auc"] == ref["auc"] and out["ap"] == ref["ap"]
        assert out["n_pos"] == out["n_neg"] == len(ex)

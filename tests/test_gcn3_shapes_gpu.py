"""The 3-layer attack (lt_influence3_rows_mode, lt_influence3_pairs; narrow and wide handles) at the shapes the rest of the suite
leaves out (gcn3_shape_cases.py; their conditions: test_gcn3_shapes_cpu.py):

  1. hidden widths that are no multiple of 4 and class counts on every lane-group size of the wide class layer, on two small graphs
     and on one whose feature rows have an odd stride: `delta` within 1e-5 of the largest score of the fp64 oracle
     (oracle.linkteller_oracle.influence_matrix with gcn3_forward, as test_gcn3_wide_attack_gpu._oracle calls it) on both routes of
     the probes' product rows, exact zeros, the all-zero probe; `sparse` inside the reference's own fp32 noise class
     (conftest.noise_gate) and `full` its bits; logits() against the fp64 forward;
  2. relations that need no tolerance on the padded shapes: chunking, subsets of either list, the pair list, a weight update;
  3. probe bitmaps of 516 words (three stretches of k3_list2 / k3w_rank2) and a wide chunk of 300 probes (k3w_list2's strided sum);
  4. a whole row at its layer-1 / layer-2 kinks behind padded widths and through the wide chain, and the wide chain's bits under a
     power-of-two rescaling of layer 2.

Every case builds its own handle; the oracle matrices are computed once per process and shared."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import gcn3_shape_cases as S
import test_gcn3_shapes_cpu as SC
from conftest import noise_gate
from linkteller_amd import _lib
from test_gcn3_pairs_gpu import _pairs
from test_gcn3_wide_attack_gpu import KEYS, _oracle, _wide3
from test_pairs_gpu import _from_rect

pytestmark = pytest.mark.gpu

DELTA = S.DELTA
GATE = 1e-5             # the project's bound of every `delta` test: |ours - ref64|.max() <= 1e-5 * ref64.max()


@contextlib.contextmanager
def knobs(**kw):
    try:
        for k, v in kw.items():
            _lib.set_tuning(k, v)
        yield
    finally:
        for k in kw:
            _lib.set_tuning(k, None)


# ---- handles, oracles ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hg(name):
    from linkteller_amd import graph
    a_hat = {"big": S.big_graph, "kink": lambda: (S.kink_base()["a_hat"],)}.get(name, lambda: S.small_graph(name))()[0]
    return graph.HipGraph(a_hat)


def _make(name, x, params, wide, gpu):
    from linkteller_amd import engine
    dev = [torch.from_numpy(np.ascontiguousarray(params[k])).to(gpu) for k in KEYS]
    base = (_wide3 if wide else engine.Baseline3)(_hg(name), torch.from_numpy(x).to(gpu), *dev)
    assert base.wide == wide and (base.h1, base.h2, base.c) == (params["W1"].shape[1], params["W2"].shape[1], params["W3"].shape[1])
    return base, dev


def _small(name, shape, wide, gpu):
    return _make(name, S.small_graph(name)[1], S.small_params(name, shape), wide, gpu)


def _rows(base, probes, obs, mode="delta"):
    out = torch.full((len(probes), len(obs)), float("nan"), dtype=torch.float32, device=base.x.device)
    got = base.influence_rows(probes, obs, DELTA, mode, out=out).cpu().numpy()
    assert np.isfinite(got).all()                      # (a cell nobody wrote keeps its NaN)
    return got


@functools.lru_cache(maxsize=None)
def _ref32(a_key, shape):
    """The oracle of _oracle on float32 tensors: the reference's own fp32 finite difference.  On ONE thread: the fp32 sums of the
    CPU products depend on how many threads share them (the error of loops / 129x130x6 is 4.85e-3 on sixteen threads and 3.57e-3
    on one), and the recorded ratios are in units of this error -- whatever an earlier test left the thread count at."""
    from oracle import linkteller_oracle as O
    a_hat, x, probes, obs, _ = S.big_graph() if a_key == "big" else S.small_graph(a_key)
    params = S.big_params(shape) if a_key == "big" else S.small_params(a_key, shape)
    nodes = np.concatenate([probes, obs]).astype(np.int64)
    P = {k: torch.from_numpy(np.asarray(v)).float() for k, v in params.items()}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        full = O.influence_matrix(torch.from_numpy(x).float(), O.to_torch_sparse(a_hat).float(), P, nodes, DELTA,
                                  forward=O.gcn3_forward, probe_range=range(len(probes)))
    finally:
        torch.set_num_threads(threads)
    return np.asarray(full[:len(probes), len(probes):], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _big_ref64(shape):
    a_hat, x, probes, obs, _ = S.big_graph()
    return _oracle(a_hat, x, S.big_params(shape), probes, obs)


def _check_delta(got, ref, zrow, what):
    got = got.astype(np.float64)
    err = np.abs(got - ref).max() / ref.max()
    print(f"gcn3shape {what}: max {ref.max():.3g} zeros {(ref == 0).mean():.2f} |ours - ref64| / max = {err:.2e}")
    assert ref.max() > 0 and err <= GATE, (what, err)
    assert np.all(got[ref == 0] == 0) and not np.signbit(got).any(), what
    if zrow is not None:
        assert np.all(ref[zrow] == 0) and np.all(got[zrow] == 0), what      # the all-zero feature row: nothing to perturb
    return err


def _check_sparse(base, probes, obs, ref, ref32, key):
    got = _rows(base, probes, obs, "sparse")
    e32, scale = np.abs(ref32 - ref).max(), ref.max()
    ours = np.abs(got.astype(np.float64) - ref).max()
    print(f"{key}: max {scale:.3g} |ref32 - ref64| {e32:.2e} |ours - ref64| {ours:.2e} ratio {ours / max(e32, 1e-4 * scale):.4f}")
    noise_gate(key, ours / max(e32, 1e-4 * scale))
    assert np.all(got[ref == 0] == 0) and not np.signbit(got).any()
    assert np.array_equal(_rows(base, probes, obs, "full"), got)
    return got


def _finish():
    from linkteller_amd import engine
    torch.cuda.synchronize()
    engine.node_check()


# ---- 1. the width ladder against the oracle --------------------------------------------------------------------------------------
SMALL_IDS = [f"{c[0]}-{S.case_id(c[1:])}" for c in SC.SMALL]


@pytest.mark.parametrize("name,shape,wide", SC.SMALL, ids=SMALL_IDS)
def test_delta_and_logits_on_the_width_ladder(gpu, name, shape, wide):
    from oracle import linkteller_oracle as O
    a_hat, x, probes, obs, zrow = S.small_graph(name)
    ref = SC.ref64(name, shape)
    base, _ = _small(name, shape, wide, gpu)
    # the probes' fp64 product rows read off the inner baseline's product (1), or formed again by the gathered product (0: the
    # route that clears the pad columns of Spd itself); each against the oracle, no bit claim between them
    for gather in (1, 0):
        with knobs(gcn3_product_gather=gather):
            _check_delta(_rows(base, probes, obs), ref, zrow, f"{name} {S.case_id((shape, wide))} gather={gather}")
    p = S.small_params(name, shape)
    ref_logits = O.gcn3_forward(torch.from_numpy(x).double(), O.to_torch_sparse(a_hat).double(),
                                {k: torch.from_numpy(np.asarray(v)).double() for k, v in p.items()}).numpy()
    logits = base.logits().cpu().numpy().astype(np.float64)
    assert logits.shape == ref_logits.shape == (a_hat.shape[0], shape[2])
    assert np.abs(logits - ref_logits).max() <= 2e-5 * max(1.0, np.abs(ref_logits).max())
    _finish()


SPARSE = [c for c in SC.SMALL if not c[2]]


@pytest.mark.parametrize("name,shape,wide", SPARSE, ids=[f"{c[0]}-{S.case_id(c[1:])}" for c in SPARSE])
def test_sparse_and_full_on_the_width_ladder(gpu, name, shape, wide):
    _, _, probes, obs, zrow = S.small_graph(name)
    ref = SC.ref64(name, shape)
    base, _ = _small(name, shape, wide, gpu)
    got = _check_sparse(base, probes, obs, ref, _ref32(name, shape), "gcn3shape.%s.%d.%d.%d" % ((name,) + tuple(shape)))
    assert np.all(got[zrow] == 0)
    _finish()


# ---- 2. relations that need no tolerance -----------------------------------------------------------------------------------------
def _chunked_bits(base, probes, obs, modes, want):
    """one probe per chunk, then a chunk budget of twice one probe's workspace: the bits of the default chunking"""
    lib = _lib.lib()
    need1 = lib.lt_influence3_workspace_bytes(base._h, 1, len(obs))
    need_all = lib.lt_influence3_workspace_bytes(base._h, len(probes), len(obs))
    for budget in (1, 2 * need1):
        with knobs(chunk_budget_bytes=budget):
            need = lib.lt_influence3_workspace_bytes(base._h, len(probes), len(obs))
            assert need < min(need_all, 4 * need1), (budget, need, need1, need_all)          # chunks of 1 .. 3 probes
            for mode in modes:
                assert np.array_equal(_rows(base, probes, obs, mode), want[mode]), (budget, mode)


REL = [(g,) + c for g in S.GRAPHS for c in S.RELATIONS]


@pytest.mark.parametrize("name,shape,wide", REL, ids=[f"{c[0]}-{S.case_id(c[1:])}" for c in REL])
def test_chunks_subsets_pairs_and_refresh(gpu, name, shape, wide):
    a_hat, x, probes, obs, zrow = S.small_graph(name)
    base, dev = _small(name, shape, wide, gpu)
    modes = ("delta",) if wide else ("delta", "sparse")
    want = {m: _rows(base, probes, obs, m) for m in modes}
    assert len(probes) > 8
    _chunked_bits(base, probes, obs, modes, want)
    sel, cols = np.array([9, 2, 24, 2, 17]), np.array([30, 1, 1, 12])
    for m in modes:
        assert np.array_equal(_rows(base, probes, obs, m), want[m]), m                          # two runs
        assert np.array_equal(_rows(base, probes[sel], obs, m), want[m][sel]), m
        assert np.array_equal(_rows(base, probes, obs[cols], m), want[m][:, cols]), m
    # a workspace that holds 0xFF bytes (NaN as a float) when the call starts: nothing reads a pad column, a pad lane or a table
    # entry that the call itself has not written -- the same bits
    for m in modes:
        _rows(base, probes, obs, m)                    # (the handle keeps the workspace of its last call's list lengths)
        (ws,) = base._ws.values()
        ws.fill_(0xFF)
        assert np.array_equal(_rows(base, probes, obs, m), want[m]), m
        assert next(iter(base._ws.values())) is ws
    # the pair list of test_gcn3_pairs_gpu: the rectangle over the distinct observed nodes, read at the listed cells
    ptr, pobs, col, row = _pairs(name)
    pool = np.unique(obs)
    for m in modes:
        cells = base.influence_pairs(probes, ptr, pobs, DELTA, m).cpu().numpy()
        assert cells.shape == (len(pobs),) and np.array_equal(cells, _from_rect(_rows(base, probes, pool, m), ptr, pobs, pool)), m
        assert np.array_equal(cells, want[m][row, col]), m
        with knobs(chunk_budget_bytes=1):
            assert np.array_equal(base.influence_pairs(probes, ptr, pobs, DELTA, m).cpu().numpy(), cells), m
    # a weight update in place + refresh(): other scores, still the oracle's
    with torch.no_grad():
        dev[2].mul_(1.25)
    base.refresh()
    p2 = dict(S.small_params(name, shape))
    p2["W2"] = (p2["W2"] * np.float32(1.25)).astype(np.float32)
    assert np.array_equal(dev[2].cpu().numpy(), p2["W2"])
    ref2 = _oracle(a_hat, x, p2, probes, obs)
    after = _rows(base, probes, obs)
    _check_delta(after, ref2, zrow, f"{name} {S.case_id((shape, wide))} after W2 * 1.25")
    assert np.abs(after.astype(np.float64) - want["delta"]).max() > 1e-3 * ref2.max()
    _finish()


# ---- 3. bitmaps of more than 256 words, chunks of more than 256 probes -----------------------------------------------------------
@pytest.mark.parametrize("shape,wide", S.BIG, ids=[S.case_id(c) for c in S.BIG])
def test_three_stretches_of_bitmap_words(gpu, shape, wide):
    a_hat, x, probes, obs, zrow = S.big_graph()
    assert (a_hat.shape[0] + 31) // 32 == 516
    ref = _big_ref64(shape)
    base, _ = _make("big", x, S.big_params(shape), wide, gpu)
    want = {}
    for gather in (1, 0):
        with knobs(gcn3_product_gather=gather):
            got = _rows(base, probes, obs)
            _check_delta(got, ref, zrow, f"big {S.case_id((shape, wide))} gather={gather}")
            want.setdefault("delta", got)
    if not wide:
        want["sparse"] = _check_sparse(base, probes, obs, ref, _ref32("big", shape), "gcn3shape.big.%d.%d.%d" % tuple(shape))
    # one probe per chunk: the same bits (a chunk's items start at the head of its tables; a probe's own order must not matter)
    with knobs(chunk_budget_bytes=1):
        lib = _lib.lib()
        assert lib.lt_influence3_workspace_bytes(base._h, len(probes), len(obs)) < 2 * lib.lt_influence3_workspace_bytes(base._h, 1, len(obs))
        for m, w in want.items():
            assert np.array_equal(_rows(base, probes, obs, m), w), m
    _finish()


@pytest.mark.parametrize("shape", S.ALL_PROBES, ids=lambda s: "x".join(map(str, s)))
def test_three_hundred_probes_in_one_wide_chunk(gpu, shape):
    a_hat, x, _, obs, _ = S.small_graph("er")
    n = a_hat.shape[0]
    probes = np.arange(n, dtype=np.int32)
    base, _ = _small("er", shape, True, gpu)
    base.enable_fp64()
    lib = _lib.lib()
    # the workspace grows with every probe of a chunk (n * Cp floats of dS3x alone), so the bytes of a chunk of 300 are reached
    # only by a chunk of 300: the default budget cuts nothing, a budget of 2^50 bytes could not take more
    need = {k: lib.lt_influence3_workspace_bytes(base._h, k, len(obs)) for k in (256, 299, 300)}
    with knobs(chunk_budget_bytes=1 << 50):
        assert lib.lt_influence3_workspace_bytes(base._h, 300, len(obs)) == need[300]
    assert need[256] < need[299] < need[300] and need[300] - need[256] >= 44 * n * S.round_up4(shape[2]) * 4
    ref = _oracle(a_hat, x, S.small_params("er", shape), probes, obs)
    got = _rows(base, probes, obs)
    zero = int(np.flatnonzero(~x.any(axis=1))[0])
    _check_delta(got, ref, zero, f"er {S.case_id((shape, True))} 300 probes")
    with knobs(chunk_budget_bytes=1):
        assert lib.lt_influence3_workspace_bytes(base._h, 300, len(obs)) < need[256]
        assert np.array_equal(_rows(base, probes, obs), got)
    _finish()


# ---- 4. a row at its kinks behind padded and wide layers -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kink_ref(widths, seed, variant):
    c = S.kink_base()
    return SC_oracle(c["x"], S.kink_weights(widths, seed, variant))


def SC_oracle(x, w):
    import test_value_domain_cpu as VC
    return VC.oracle("G", x, w)


_kink_cache = {}


def _kink_run(gpu, widths, seed, handle, variant, k=0, **kn):
    key = (widths, seed, handle, variant, k, tuple(sorted(kn.items())))
    if key not in _kink_cache:
        c = S.kink_base()
        with knobs(**kn):          # ("s1_f32" is read when the fp64 baseline is formed: a fresh handle under the knobs)
            base, _ = _make("kink", c["x"], S.kink_weights(widths, seed, variant, k), handle == "wide", gpu)
            _kink_cache[key] = _rows(base, c["probes"], c["obs"])
    return _kink_cache[key]


KINK = [(w, s, h, v) for w, s, hs in S.KINKS for h in hs for v in S.VARIANTS]
KINK_IDS = ["x".join(map(str, w)) + f"-seed{s}-{h}-{v}" for w, s, h, v in KINK]


@pytest.mark.parametrize("widths,seed,handle,variant", KINK, ids=KINK_IDS)
def test_row_at_its_kinks_behind_padded_and_wide_layers(gpu, widths, seed, handle, variant):
    """Every unit of row r0 crosses its kink (layer 1: `kink`, layer 2: `kink2`) under every probe that reaches the row.  The
    storage of the product rows costs at most 8.8e-7 of the largest score on these cases (test_gcn3_shapes_cpu.py), so the gate
    is the kernels'."""
    ref = _kink_ref(widths, seed, variant)
    errs = {}
    for label, kn in (("default", {}), ("s1_f32=0", dict(s1_f32=0))):
        got = _kink_run(gpu, widths, seed, handle, variant, **kn).astype(np.float64)
        assert np.all(got[ref == 0] == 0) and not np.signbit(got).any(), label
        errs[label] = np.abs(got - ref).max() / ref.max()
    print(f"gcn3shape kink {widths} seed {seed} {handle} {variant}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["default"] <= GATE and errs["s1_f32=0"] <= GATE, errs
    _finish()


RESCALE = [(w, s, v, k) for w, s, hs in S.KINKS for v in S.VARIANTS for k in S.EXACT_KS]


@pytest.mark.parametrize("widths,seed,variant,k", RESCALE, ids=["x".join(map(str, w)) + f"-{v}-k{k}" for w, s, v, k in RESCALE])
def test_wide_chain_keeps_its_bits_under_a_rescaling_of_layer_2(gpu, widths, seed, variant, k):
    """The even units of layer 2 scaled by 2^k (W2 columns and b2 up, W3 rows down): with fp64 product rows nothing in the wide
    chain is fixed point and a power of two commutes with every rounding, so a changed bit is an absolute constant or a product
    that is not fp32 behind the layer-2 kink test.  (The oracle does not move either: test_gcn3_shapes_cpu.py.)"""
    a = _kink_run(gpu, widths, seed, "wide", variant, k, s1_f32=0)
    b = _kink_run(gpu, widths, seed, "wide", variant, 0, s1_f32=0)
    assert np.array_equal(a, b), (int((a != b).sum()), float(np.abs(a.astype(np.float64) - b).max() / b.max()))
    _finish()

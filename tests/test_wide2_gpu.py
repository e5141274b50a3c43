"""The wide 2-layer attack (engine.WideBaseline = one lt_influence_rows_vec call per slice of <= 256 hidden units and <= 8 classes,
joined by lt_wide_combine) where the rest of the suite leaves it alone (wide2_cases.py; what the references can see:
test_wide2_cpu.py):

  A. lt_wide_combine against its contract restated in numpy, bit for bit, and its refusals;
  B. the difference vectors of lt_influence_rows_vec on the hub ladder under every stage-B knob: the norms and the vectors against
     lt_influence_rows, against lt_wide_combine on one slice, against each other, chunked, and in `delta` every COMPONENT against
     the plain fp64 difference;
  C. WideBaseline on the hub ladder at its slice edges against the fp64 oracle, its exact relations to the narrow model, and
     the limit of 32 hidden slices.

No tolerance of its own: `delta` is held to 1e-5 of the largest fp64 score (test_boundary_gpu.py), `sparse` to the
recorded noise gate of conftest.py, the logits to the bound of test_layers_wider_than_the_fused_kernels; everything else is bits."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

import boundary_cases as B
import wide2_cases as W
from conftest import noise_gate
from test_boundary_gpu import _baseline, _dev_inputs, _hg, _rows, _sentinel, knobs

pytestmark = pytest.mark.gpu

DELTA = W.DELTA


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- A. lt_wide_combine ---------------------------------------------------------------------------------------------------------
def _combine(dev, C, delta, ss, first, last, n_vec=None, n_pairs=None, null_entry=None):
    """The raw call: its return code (the stream is drained).  ``dev``: the slices' device tensors; ``ss``: a device tensor or None."""
    from linkteller_amd import _lib, engine
    n_vec = len(dev) if n_vec is None else n_vec
    ptrs = (ct.c_void_p * max(len(dev), n_vec, 1))()
    for s in range(len(ptrs)):
        ptrs[s] = dev[s % len(dev)].data_ptr()
    if null_entry is not None:
        ptrs[null_entry] = None
    n_pairs = dev[0].shape[0] if n_pairs is None else n_pairs
    rc = _lib.lib().lt_wide_combine(ptrs, n_vec, n_pairs, C, delta, None if ss is None else ss.data_ptr(), first, last, engine._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("n_vec,C,n_pairs", W.COMBINE_CASES, ids=lambda v: str(v))
def test_combine_bits(gpu, n_vec, C, n_pairs):
    """The four (first, last) combinations at both signs of delta: the bits of combine_restated.  A call that is not the first
    starts from the buffer's running sum."""
    v = W.combine_case(n_vec, C, n_pairs)
    dev = [torch.from_numpy(np.ascontiguousarray(v[s])).to(gpu) for s in range(n_vec)]
    rng = np.random.RandomState(n_vec + C)
    running = (rng.uniform(0, 100, n_pairs) * (rng.uniform(0, 1, n_pairs) > 0.1)).astype(np.float32)
    for delta in W.COMBINE_DELTAS:
        for first in (1, 0):
            for last in (0, 1):
                ss = torch.from_numpy(running).to(gpu) if not first else torch.full((n_pairs,), float("nan"), device=gpu)
                assert _combine(dev, C, delta, ss, first, last) == 0
                want = W.combine_restated(list(v), C, delta, running, first, last)
                got = ss.cpu().numpy()
                bad = np.flatnonzero(_bits(got) != _bits(want))
                assert bad.size == 0, (delta, first, last, bad[:5], got[bad[:5]], want[bad[:5]])


def test_combine_chain_over_one_buffer(gpu):
    """first, middle, last over classes 3 + 3 + 2 of three slices on ONE buffer that starts as NaN: after every call the buffer holds
    the restated chain -- the running sum, never a square root, until the last call -- and in the end the one chain of 8 classes."""
    v = W.combine_inputs(3, 8, 257)
    ss = torch.full((257,), float("nan"), device=gpu)
    want = None
    for k, (c0, c1) in enumerate(((0, 3), (3, 6), (6, 8))):
        part = [np.ascontiguousarray(s[:, c0:c1]) for s in v]
        assert _combine([torch.from_numpy(p).to(gpu) for p in part], c1 - c0, DELTA, ss, int(k == 0), int(k == 2)) == 0
        want = W.combine_restated(part, c1 - c0, DELTA, want, int(k == 0), int(k == 2))
        assert np.array_equal(_bits(ss.cpu().numpy()), _bits(want)), k
    assert np.array_equal(_bits(want), _bits(W.combine_restated(list(v), 8, DELTA, None, 1, 1)))


def test_combine_refusals(gpu):
    """Each refused call returns an error and leaves ss alone; n_pairs = 0 is served and launches nothing."""
    v = W.combine_inputs(2, 8, 257)
    dev = [torch.from_numpy(np.ascontiguousarray(s)).to(gpu) for s in v]
    ss = torch.full((257,), 7.0, device=gpu)
    refused = [dict(n_vec=0), dict(n_vec=W.MAX_VEC + 1), dict(C=0), dict(C=W.MAX_C + 1), dict(delta=0.0), dict(delta=float("nan")),
               dict(null_entry=1)]
    for kw in refused:
        args = dict(C=8, delta=DELTA)
        args.update(kw)
        assert _combine(dev, args.pop("C"), args.pop("delta"), ss, 1, 1, **args) < 0, kw
        assert bool((ss == 7.0).all()), kw
    assert _combine(dev, 8, DELTA, None, 1, 1) < 0
    assert _combine(dev, 8, DELTA, ss, 1, 1, n_pairs=0) == 0 and bool((ss == 7.0).all())
    assert _combine(dev, 8, DELTA, ss, 1, 1) == 0 and bool((ss != 7.0).all())          # (the same operands are served)


# ---- B. lt_influence_rows_vec on the hub ladder --------------------------------------------------------------------------------------
_vec_cache = {}


def _lists(gpu):
    probes, obs = B.node_lists("hub")
    return torch.from_numpy(probes).to(gpu), torch.from_numpy(obs).to(gpu)


def _vec(gpu, h, c, mode, **kn):
    """One fresh baseline under the knobs, one lt_influence_rows_vec call over node_lists("hub") into NaN-filled results:
    (out [n_probe, n_obs], vec [n_probe, n_obs, C]) as float32 numpy.  Cached per knob set."""
    from linkteller_amd import _lib
    key = (h, c, mode, tuple(sorted(kn.items())))
    if key not in _vec_cache:
        probes, obs = _lists(gpu)
        out = _sentinel(probes.numel(), obs.numel())
        vec = torch.full((probes.numel(), obs.numel(), c), float("nan"), dtype=torch.float32, device=gpu)
        with knobs(**kn):
            _baseline("hub", h, c).influence_rows_vec(probes, obs, DELTA, _lib.MODES[mode], out, vec)
        got = out.cpu().numpy(), vec.cpu().numpy()
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()          # (a cell nobody wrote keeps its NaN)
        _vec_cache[key] = got
    return _vec_cache[key]


def _chunks(base, npb, nob, m, budget):
    """The probe chunks of a call under "chunk_budget_bytes" = budget, from the workspace geometry: but for the checked probe
    list (4 bytes a probe of the CALL, rounded up to 256) every table of the workspace is sized by the chunk, and under the
    default budget a call of k probes is one chunk of k -- so the chunk is the one k whose tables have the same size."""
    from linkteller_amd import _lib
    need = _lib.lib().lt_influence_workspace_bytes

    def list_bytes(k):
        return (4 * k + 255) // 256 * 256

    with knobs(chunk_budget_bytes=budget):
        tables = need(base._h, npb, nob, m) - list_bytes(npb)
    fits = [k for k in range(1, npb + 1) if need(base._h, k, nob, m) - list_bytes(k) == tables]
    assert len(fits) == 1, fits
    return -(-npb // fits[0])


@pytest.mark.parametrize("mode", ["sparse", "delta"])
@pytest.mark.parametrize("h,c", B.MODEL_SHAPES)
def test_difference_vectors_on_hub_ladder(gpu, h, c, mode):
    from linkteller_amd import _lib
    m = _lib.MODES[mode]
    ref64 = B.oracle_matrix("hub", h, c, "float64")
    probes, obs = B.node_lists("hub")
    out0, vec0 = _vec(gpu, h, c, mode)
    for kn in [{}] + W.ITEM_KNOBS:
        out, vec = _vec(gpu, h, c, mode, **kn)
        # the norm form under the same knobs, on the per-pair stage B and off the fused route like every vector call
        # (test_boundary_gpu's knob tests already show that "stageb_rows" and "delta_fused" change no bit of it)
        norm = _rows("hub", h, c, mode, **dict(kn, stageb_rows=0, delta_fused=0)).astype(np.float32)
        assert np.array_equal(_bits(out), _bits(norm)), kn
        # one slice through lt_wide_combine: the tails of diff_norm, of the DELTA branch and of store_diff_vec are the same operations
        ss = torch.full((out.size,), float("nan"), device=gpu)
        assert _combine([torch.from_numpy(vec).to(gpu).view(-1, c)], c, DELTA, ss, 1, 1) == 0
        assert np.array_equal(_bits(ss.cpu().numpy().reshape(out.shape)), _bits(out)), kn
        assert np.array_equal(_bits(vec), _bits(vec0)), kn
    # the library's own probe chunks (vrow = vec + p0 * ldo * C)
    budget = 1 << 19
    n_chunks = _chunks(_baseline("hub", h, c), len(probes), len(obs), m, budget)
    assert n_chunks >= 3, n_chunks
    out_c, vec_c = _vec(gpu, h, c, mode, chunk_budget_bytes=budget)
    assert np.array_equal(_bits(vec_c), _bits(vec0)) and np.array_equal(_bits(out_c), _bits(out0))
    # +0.0 in every component exactly where the fp64 pair is untouched -- the member ladder's m = 0 cells among them
    untouched = ref64 == 0
    m_rows, m_col = B.member_cells()
    assert untouched[m_rows, m_col].sum() == 2 and (~untouched[m_rows, m_col]).sum() == len(m_rows) - 2
    assert np.all(_bits(vec0)[untouched] == 0)
    if mode == "delta":
        # (the propagated difference of a touched pair is no cancellation: it is there.  SPARSE's fp32 difference of a pair
        #  whose score is 6e-7 of the largest is below the last place of its logits)
        assert np.array_equal((vec0 != 0).any(axis=2), ~untouched)
    assert (vec0 != 0).any(axis=2).sum() > 0.25 * untouched.size
    dup = np.flatnonzero(obs == B.hub_ladder().u[B.HUB])
    assert len(dup) == 2 and np.array_equal(_bits(vec0[:, dup[0]]), _bits(vec0[:, dup[1]]))
    if mode == "delta":
        # every component: sign, order and class index -- the project's `delta` bound, applied before the norm
        ref = W.diff_vectors64("hub", h, c)
        scale = ref64.max()
        got = vec0.astype(np.float64) / float(np.float32(DELTA))
        err = np.abs(got - ref).max()
        sub = np.abs(got[m_rows, m_col] - ref[m_rows, m_col]).max()
        print(f"wide2 vec H {h} C {c}: max score {scale:.3f}; |vec / delta - ref64| per component = {err:.3e} ({err / scale:.2e} of max), "
              f"bound {W.GATE * scale:.3e}; member cells {sub:.3e} of a largest member score {ref64[m_rows, m_col].max():.3e}")
        assert err <= W.GATE * scale
        assert sub <= W.GATE * ref64[m_rows, m_col].max()
    print(f"wide2 vec H {h} C {c} {mode}: {n_chunks} chunks at {budget} bytes; {int((~untouched).sum())} touched pairs of {untouched.size}")


# ---- C. WideBaseline ------------------------------------------------------------------------------------------------------------------
def _params(w, gpu):
    return [torch.from_numpy(np.ascontiguousarray(w[k])).to(gpu) for k in ("W1", "b1", "W2", "b2")]


def _wide(gpu, w):
    from linkteller_amd import engine
    base = engine.baseline_for(_hg("hub"), _dev_inputs("hub", *B.MODEL_SHAPES[0])[0], *_params(w, gpu))
    assert isinstance(base, engine.WideBaseline)
    return base


def _wrows(base, mode, lists=None):
    probes, obs = lists or B.node_lists("hub")
    got = base.influence_rows(probes, obs, DELTA, mode, out=_sentinel(len(probes), len(obs))).cpu().numpy()
    assert np.isfinite(got).all()          # (a cell nobody wrote keeps its NaN)
    return got


@pytest.mark.parametrize("h,c", W.WIDE_SHAPES)
def test_wide_baseline_on_hub_ladder(gpu, h, c):
    ref64 = B.oracle_matrix("hub", h, c, "float64")
    e32 = np.abs(B.oracle_matrix("hub", h, c, "float32") - ref64).max()
    scale = ref64.max()
    _, obs = B.node_lists("hub")
    base = _wide(gpu, B.weights(h, c))
    assert [len(s) for s in (base.h_slices, base.c_slices)] == [len(s) for s in W.slices(h, c)]
    res = {mode: _wrows(base, mode).astype(np.float64) for mode in ("delta", "sparse", "full")}
    e_delta, e_sparse = np.abs(res["delta"] - ref64).max(), np.abs(res["sparse"] - ref64).max()
    m_rows, m_col = B.member_cells()
    sub = ref64[m_rows, m_col]
    e_member = np.abs(res["delta"][m_rows, m_col] - sub).max()
    print(f"wide2 H {h} C {c}: max score {scale:.3f}; |ref32 - ref64| = {e32:.3e}; |delta - ref64| = {e_delta:.3e} ({e_delta / scale:.2e} "
          f"of max); member cells {e_member / sub.max():.2e} of their max; |sparse - ref64| = {e_sparse:.3e} "
          f"(ratio {e_sparse / max(e32, 1e-4 * scale):.4f})")
    assert e_delta <= W.GATE * scale
    assert e_member <= W.GATE * sub.max()
    assert np.array_equal(res["sparse"], res["full"])
    noise_gate(f"wide2.hub.h{h}c{c}.sparse", e_sparse / max(e32, 1e-4 * scale))
    dup = np.flatnonzero(obs == B.hub_ladder().u[B.HUB])
    for got in res.values():
        assert np.all(got[ref64 == 0] == 0) and not np.signbit(got).any()
        assert np.array_equal(got[:, dup[0]], got[:, dup[1]])
    ref_logits = B.oracle_logits("hub", h, c)
    assert np.abs(base.logits().cpu().numpy() - ref_logits).max() <= 2e-5 * max(1.0, np.abs(ref_logits).max())


@pytest.mark.parametrize("kind", ["hidden", "classes"])
def test_wide_equals_narrow_where_a_slice_adds_nothing(gpu, kind):
    """H = 300 with W2[256:] = 0: the second hidden slice's vectors are exact zeros; C = 12 with W2[:, 8:] = 0 and b2[8:] = 0: the
    second class slice adds fma(0, 0, ss).  The bits of engine.Baseline on the narrow model -- and other bits once the block holds
    small values (the relation is not vacuous)."""
    from linkteller_amd import engine
    w, narrow = W.relation_weights(kind)
    wc, _ = W.relation_weights(kind, control=True)
    x = _dev_inputs("hub", *B.MODEL_SHAPES[0])[0]
    for mode in ("sparse", "delta"):
        probes, obs = B.node_lists("hub")
        nb = engine.Baseline(_hg("hub"), x, *_params(narrow, gpu))
        want = nb.influence_rows(probes, obs, DELTA, mode, out=_sentinel(len(probes), len(obs))).cpu().numpy()
        assert (want > 0).any()
        got = _wrows(_wide(gpu, w), mode)
        assert np.array_equal(_bits(got), _bits(want)), mode
        control = _wrows(_wide(gpu, wc), mode)
        assert (_bits(control) != _bits(want)).any(), mode


@functools.lru_cache(maxsize=None)
def _knob_default(mode):
    return _wrows(_wide(torch.device("cuda:0"), B.weights(*W.KNOB_SHAPE)), mode)


@pytest.mark.parametrize("mode", ["sparse", "delta"])
def test_wide_baseline_under_the_item_knobs(gpu, mode):
    """(260, 9): every stage-B knob, the probe chunks of WideBaseline (5 probes each) and the library's own chunks inside every
    slice call give the default's bits."""
    from linkteller_amd import _lib, engine
    want = _knob_default(mode)
    w = B.weights(*W.KNOB_SHAPE)
    for kn in W.ITEM_KNOBS:
        with knobs(**kn):
            assert np.array_equal(_bits(_wrows(_wide(gpu, w), mode)), _bits(want)), kn
    probes, obs = B.node_lists("hub")
    base = _wide(gpu, w)
    base.VEC_BUDGET_BYTES = 5 * len(base.h_slices) * len(obs) * 8 * 4          # (an attribute of this object: the class keeps its own)
    assert engine.WideBaseline.VEC_BUDGET_BYTES == 256 << 20
    assert np.array_equal(_bits(_wrows(base, mode)), _bits(want))
    assert base._buf["key"] == (5, len(obs)) and len(probes) > 3 * 5
    base = _wide(gpu, w)
    budget = 1 << 19
    with knobs(chunk_budget_bytes=budget):
        got = _wrows(base, mode)
    for sub, _ in base._subs.values():
        assert _chunks(sub, len(probes), len(obs), _lib.MODES[mode], budget) >= 3
    assert np.array_equal(_bits(got), _bits(want))


def test_wide_baseline_refresh_after_a_weight_update(gpu):
    """W1 changes in place, refresh("delta"): the bits of a fresh WideBaseline on the changed weights, in both modes."""
    base = _wide(gpu, B.weights(*W.KNOB_SHAPE))
    before = {mode: _wrows(base, mode) for mode in ("delta", "sparse")}
    with torch.no_grad():
        base.w1.mul_(0.75)
    base.refresh("delta")
    after = {mode: _wrows(base, mode) for mode in ("delta", "sparse")}
    fresh = _wide(gpu, {k: t.cpu().numpy() for k, t in zip(("W1", "b1", "W2", "b2"), (base.w1, base.b1, base.w2, base.b2))})
    for mode in ("delta", "sparse"):
        assert np.array_equal(_bits(after[mode]), _bits(_wrows(fresh, mode))), mode
        assert (_bits(after[mode]) != _bits(before[mode])).any(), mode


def _tiny_base(gpu, h, c):
    from linkteller_amd import engine, graph
    t = W.tiny()
    return engine.baseline_for(graph.HipGraph(t.a), torch.from_numpy(t.x).to(gpu), *_params(W.tiny_weights(h, c), gpu))


def test_thirty_two_hidden_slices_and_the_refusal_above(gpu):
    """H = 8192 = 32 x 256 on a 64-node graph: `delta` against the verbatim fp64 oracle, sparse == full; H = 8193 is refused at
    construction."""
    from oracle import linkteller_oracle as O
    t = W.tiny()
    h, c = W.MAX_VEC * W.H_SLICE, 2
    base = _tiny_base(gpu, h, c)
    assert len(base.h_slices) == W.MAX_VEC
    P = {k: torch.from_numpy(v).double() for k, v in W.tiny_weights(h, c).items()}
    xt, adj = torch.from_numpy(t.x).double(), O.to_torch_sparse(t.a).double()
    idx = torch.as_tensor(t.obs.astype(np.int64))
    with torch.no_grad():
        ref64 = np.stack([O.get_gradient_eps_mat(xt, adj, P, int(v), DELTA)[idx].norm(dim=1).numpy() for v in t.probes])
    assert np.abs(W.tiny_ref64(h, c) - ref64).max() <= 1e-9 * ref64.max()
    res = {mode: _wrows(base, mode, (t.probes, t.obs)).astype(np.float64) for mode in ("delta", "sparse", "full")}
    err = np.abs(res["delta"] - ref64).max()
    print(f"wide2 tiny H {h}: max score {ref64.max():.3f}; |delta - ref64| = {err:.3e} ({err / ref64.max():.2e} of max)")
    assert err <= W.GATE * ref64.max()
    assert np.array_equal(res["sparse"], res["full"])
    for got in res.values():
        assert np.all(got[ref64 == 0] == 0) and np.array_equal(got[-1], got[np.flatnonzero(t.probes == t.probes[-1])[0]])
    with pytest.raises(NotImplementedError):
        _tiny_base(gpu, h + 1, c)

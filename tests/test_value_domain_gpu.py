"""`delta` against the fp64 oracle on models whose hidden units and feature columns differ in scale, and with a whole row of
hidden units at their kinks, on every route: the dense product (int8 split and f64 matrix cores, fused and item kernels), the
feature rows (with and without the kept lists), aggregate-first, Baseline3 and WideBaseline.  Inputs and transformations:
value_domain_cases.py.  The oracle matrices (tests/golden/value_domain_ref.npz) do not move by a bit under the rescalings and the
storage model's error per cell is tests/golden/value_domain_model.json: test_value_domain_cpu.py asserts both.

  * exactness: nothing in logits(), `full`, `sparse` or `delta` with fp64 storage is fixed point, and a scale by a power of two
    commutes with every rounding -- the run at k gives the bits of the run at k = 0, or some kernel holds an absolute constant;
  * the claim, where the storage model puts a cell INSIDE the domain (its error <= a quarter of the gate): default knobs within
    1e-5 of the largest score, fp64 storage within 1e-6 (the gates of test_delta_with_a_whole_row_of_hidden_units_at_their_kinks),
    exact zeros where the oracle has exact zeros;
  * outside the domain (cells of M, Q, R and G): fp64 storage still within 1e-6; the default run's error in units of the model's is
    recorded and gated at +10 % (conftest.noise_gate)."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_value_domain_cpu as VC
import value_domain_cases as V
import value_domain_model as MV
from conftest import noise_gate

pytestmark = pytest.mark.gpu

GATE, GATE64 = 1e-5, 1e-6
MODEL = VC.committed_model()
DEFAULT_STORAGE = {"M": "i8+rows31", "Q": "i8+rows31", "R": "rows31", "G": "rows31"}


@contextlib.contextmanager
def knobs(**kw):
    from linkteller_amd import _lib
    try:
        for k, v in kw.items():
            _lib.set_tuning(k, v)
        yield
    finally:
        for k in kw:
            _lib.set_tuning(k, None)


@functools.lru_cache(maxsize=None)
def _refs():
    with np.load(VC.REF_FILE, allow_pickle=False) as g:
        return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def _hg(case):
    from linkteller_amd import graph
    return graph.HipGraph(V.base(case)["a_hat"])


def _baseline(case, x, w):
    from linkteller_amd import engine
    cls = {"G": engine.Baseline3, "W": engine.WideBaseline}.get(case, engine.Baseline)
    return cls(_hg(case), torch.from_numpy(x).cuda(), *[torch.from_numpy(w[k]).cuda() for k in V.WEIGHT_KEYS[V.base(case)["depth"]]])


def _check_route(case, base, kn):
    if case in V.ROUTE:
        assert base.fp64_route() == V.ROUTE[case], (case, base.fp64_route(), kn)
    if case == "R" and "s1_f32" not in kn:
        assert base.feature_list_entries() > 0, kn
    if case == "W":     # the first hidden slice (H = 256 >= F / 2) aggregate-first, the second on the dense product
        assert [base._subs[(si, 0)][0].fp64_route() for si in range(len(base.h_slices))] == [2, 0]
        assert base.h_slices == [(0, 256), (256, 320)] and len(base.c_slices) == 2


_cache = {}


def _run(case, variant, transform, k, what, **kn):
    """One fresh baseline on the cell's inputs under the knobs; float64 logits or [n_probe, n_obs] scores of mode `what`."""
    if transform is None or k == 0:
        transform, k = None, 0
    key = (case, variant, transform, k, what, tuple(sorted(kn.items())))
    if key not in _cache:
        c = V.base(case)
        x, w = V.inputs(case, variant, transform, k)
        with knobs(**kn):
            base = _baseline(case, x, w)
            if what == "logits":
                got = base.logits()
            else:
                out = torch.full((len(c["probes"]), len(c["obs"])), float("nan"), dtype=torch.float32, device="cuda")
                got = base.influence_rows(c["probes"], c["obs"], V.DELTA, what, out=out)
                if what == "delta":
                    _check_route(case, base, kn)
            got = got.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()          # (a cell nobody wrote keeps its NaN)
        _cache[key] = got
    return _cache[key]


def _launches(fn, classes):
    from linkteller_amd import _lib
    lib = _lib.lib()
    lib.lt_profile_reset()
    lib.lt_profile_enable(sum(1 << _lib.KERNEL_IDS[k] for k in classes))
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        for k in classes:
            tot, cnt = C.c_double(), C.c_int64()
            _lib.check(lib.lt_profile_summary(_lib.KERNEL_IDS[k], C.byref(tot), C.byref(cnt)), "lt_profile_summary")
            out[k] = cnt.value
    finally:
        lib.lt_profile_enable(0)
        lib.lt_profile_reset()
    return out


def _label(variant, transform):
    t = transform or "none"
    return t if variant == "plain" else f"{variant}+{t}"


def _id(cell):
    return "-".join(str(p) for p in cell)


# ---- the routes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(V.SHAPES))
def test_cases_reach_their_routes(gpu, case):
    """fp64_route, the kept lists and the wide model's slices are asserted by every `delta` run (_check_route); here also: M's graph
    keeps its records, so "delta_fused" decides between the probe blocks and the item kernels, and "i8_split" changes the bits."""
    for kn in V.KNOBS[case] + [V.FP64_KNOBS[case]]:
        _run(case, "kink", None, 0, "delta", **kn)
    if case != "M":
        return
    # (the K slices of the int8 split as the model cuts them: M has two, Q one -- its rows leave through k_quant_rows_f64)
    assert MV.i8_slices(700, 64, 300) == [(0, 256), (256, 300)] and MV.i8_slices(700, 64, 256) == [(0, 256)]
    c = V.base("M")
    x, w = V.inputs("M", "kink")
    got = {}
    with knobs(aggregate_first=0):
        base = _baseline("M", x, w).enable_fp64()
        for fused in (1, 0):
            with knobs(delta_fused=fused):
                base.refresh()
                n_l = _launches(lambda: got.__setitem__(fused, base.influence_rows(c["probes"], c["obs"], V.DELTA, "delta").cpu().numpy()), ("item_stageA",))
            assert (n_l["item_stageA"] == 0) == (fused == 1), (fused, n_l)
    assert np.array_equal(got[1], got[0])
    i8 = {v: _run("M", "kink", None, 0, "delta", aggregate_first=0, i8_split=v, delta_fused=1) for v in (1, 0)}
    assert not np.array_equal(i8[1], i8[0])


# ---- exactness ---------------------------------------------------------------------------------------------------------------------
# (the kink rows too: a pre-activation of 1e-9 scaled by 2^-20 is where an absolute threshold in a kink test would show)
EXACT = [(case, v, t, k) for case in V.SHAPES for v in V.variants(case) for t in V.transforms(case, v) for k in V.EXACT_KS]


@pytest.mark.parametrize("case,variant,transform,k", EXACT, ids=[_id(c) for c in EXACT])
def test_power_of_two_rescaling_changes_no_bit(gpu, case, variant, transform, k):
    whats = ["logits", "sparse"] + ([] if case == "G" else ["full"])
    for what in whats:
        a, b = _run(case, variant, transform, k, what), _run(case, variant, None, 0, what)
        assert np.array_equal(a, b), (what, int((a != b).sum()), float(np.abs(a - b).max()))
    kn = V.FP64_KNOBS[case]
    a, b = _run(case, variant, transform, k, "delta", **kn), _run(case, variant, None, 0, "delta", **kn)
    assert np.array_equal(a, b), ("delta, fp64 storage", int((a != b).sum()), float(np.abs(a - b).max() / b.max()))


# ---- the claim ---------------------------------------------------------------------------------------------------------------------
def _errors(case, variant, transform, k):
    """({knob id: error of the default-storage run}, error of the fp64-storage run), relative to the oracle's largest score; exact
    zeros asserted on the way."""
    ref = _refs()[f"{case}.{variant}"]
    scale = ref.max()
    errs = {}
    for kn in V.KNOBS[case]:
        got = _run(case, variant, transform, k, "delta", **kn)
        assert np.all(got[ref == 0] == 0), kn
        errs[V.knob_id(kn)] = np.abs(got - ref).max() / scale
    got64 = _run(case, variant, transform, k, "delta", **V.FP64_KNOBS[case])
    assert np.all(got64[ref == 0] == 0)
    return errs, np.abs(got64 - ref).max() / scale


def _report(case, variant, transform, k, errs, e64):
    m = MODEL[V.cell_key(case, variant, transform, k)]
    print(f"VD {V.cell_key(case, variant, transform, k)} model " + " ".join(f"{n}={v:.3e}" for n, v in m.items()) +
          " gpu " + " ".join(f"{n}={v:.3e}" for n, v in errs.items()) + f" fp64-storage={e64:.3e}")


INSIDE_CELLS = [(case,) + cell for case in V.SHAPES for cell in V.cells(case) if VC.inside(MODEL[V.cell_key(case, *cell)])]
OUTSIDE_CELLS = [(case,) + cell for case in V.SHAPES for cell in V.cells(case) if not VC.inside(MODEL[V.cell_key(case, *cell)])]
KINK_CELLS = [(case, v) for case in V.SHAPES for v in V.variants(case)[1:]]


@pytest.mark.parametrize("case,variant,transform,k", INSIDE_CELLS, ids=[_id(c) for c in INSIDE_CELLS])
def test_delta_inside_the_value_domain(gpu, case, variant, transform, k):
    errs, e64 = _errors(case, variant, transform, k)
    _report(case, variant, transform, k, errs, e64)
    assert max(errs.values()) <= GATE, errs
    assert e64 <= GATE64, e64


@pytest.mark.parametrize("case,variant", KINK_CELLS, ids=[_id(c) for c in KINK_CELLS])
def test_delta_with_a_row_at_its_kinks_on_every_route(gpu, case, variant):
    """k = 0: every unit of row r0 (layer 1; for G also layer 2) crosses its kink under every probe that reaches the row."""
    errs, e64 = _errors(case, variant, None, 0)
    _report(case, variant, None, 0, errs, e64)
    assert max(errs.values()) <= GATE, errs
    assert e64 <= GATE64, e64


@pytest.mark.parametrize("case,variant,transform,k", OUTSIDE_CELLS, ids=[_id(c) for c in OUTSIDE_CELLS])
def test_delta_outside_the_value_domain(gpu, case, variant, transform, k):
    """A limit of the storage design, not a bug: the fp64 storage ("s1_f32" = 0, on M also "i8_split" = 0) lifts it on every
    route, and the default run's error stays what the storage model says it is (ratio recorded, +10 %)."""
    errs, e64 = _errors(case, variant, transform, k)
    _report(case, variant, transform, k, errs, e64)
    assert e64 <= GATE64, e64
    model = MODEL[V.cell_key(case, variant, transform, k)][DEFAULT_STORAGE[case]]
    noise_gate(f"value_domain.{case}.{_label(variant, transform)}.{k}", errs[V.knob_id(V.KNOBS[case][0])] / model, ceiling=None)

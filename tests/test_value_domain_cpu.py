"""The instruments of test_value_domain_gpu.py, checked on the CPU: the fp64 oracle does not move by one bit under the power-of-two
rescalings of value_domain_cases.py, the plain fp64 restatement of `delta` (value_domain_model.delta_fp64) agrees with it, and the
storage model's error per (case, variant, transformation, k, storage) is the committed tests/golden/value_domain_model.json.

`python tests/test_value_domain_cpu.py --write` regenerates that file and the oracle matrices tests/golden/value_domain_ref.npz."""
import functools
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import value_domain_cases as V
import value_domain_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_FILE = os.path.join(GOLDEN, "value_domain_model.json")
REF_FILE = os.path.join(GOLDEN, "value_domain_ref.npz")
GATE = 1e-5                 # the claim of DESIGN section 3: |delta - fp64 oracle| <= 1e-5 of the largest score
INSIDE = 0.25 * GATE        # a cell is inside the domain when the MODEL's error is a quarter of the gate: room for another rounding realisation

# the storage forms a case's default-knob runs go through (value_domain_model.py); a wide model's hidden slices are baselines of
# their own: the first (H = 256, F = 300 <= 2 H) forms its pre-activation aggregate-first in fp64, the second on the int8 cores
STORAGES = {
    "M": {"i8+rows31": dict(rows="rows31", i8=True), "rows31": dict(rows="rows31")},
    "Q": {"i8+rows31": dict(rows="rows31", i8=True)},
    "R": {"rows31": dict(rows="rows31")},
    "A": {"none": dict()},
    "G": {"rows31": dict(rows="rows31")},       # (its layer-1 pre-activation comes from an inner 2-layer baseline pinned off aggregate-first)
    "W": {"i8+rows31": dict(rows="rows31", i8=True, h_slices=[(0, 256, False), (256, 320, True)])},
}


def oracle(case, x, w):
    """The reference's probe primitive in fp64, verbatim op order, over the case's node lists."""
    import torch
    from oracle import linkteller_oracle as O
    torch.set_num_threads(1)
    c = V.base(case)
    adj = O.to_torch_sparse(c["a_hat"]).double()
    p = {k: torch.from_numpy(v).double() for k, v in w.items()}
    xt = torch.from_numpy(x).double()
    fwd = O.gcn3_forward if c["depth"] == 3 else O.gcn_forward
    obs = torch.as_tensor(c["obs"].astype(np.int64))
    out = np.zeros((len(c["probes"]), len(c["obs"])))
    with torch.no_grad():
        for i, v in enumerate(c["probes"]):
            out[i] = O.get_gradient_eps_mat(xt, adj, p, int(v), V.DELTA, fwd)[obs].norm(dim=1).numpy()
    return out


@functools.lru_cache(maxsize=None)
def table(case):
    """(refs, moved, errs): the oracle matrix per variant; per cell the largest |oracle(cell) - oracle(k = 0)| (exactly 0 is the
    claim) and the model's error per storage, relative to the largest score ("fp64": no storage)."""
    c = V.base(case)
    refs, moved, errs = {}, {}, {}
    for variant, transform, k in V.cells(case):
        x, w = V.inputs(case, variant, transform, k)
        ref = oracle(case, x, w)
        if k == 0:
            refs[variant] = ref
        key = V.cell_key(case, variant, transform, k)
        moved[key] = float(np.abs(ref - refs[variant]).max()) if np.array_equal(ref.shape, refs[variant].shape) else np.inf
        scale = refs[variant].max()
        errs[key] = {name: float(np.abs(M.delta_fp64(c["a_hat"], x, w, c["probes"], c["obs"], V.DELTA, **kw) - refs[variant]).max() / scale)
                     for name, kw in [("fp64", {})] + list(STORAGES[case].items())}
    return refs, moved, errs


def committed_model():
    with open(MODEL_FILE) as fh:
        return json.load(fh)


def worst(errs_of_cell):
    """A cell's model error: the largest over the case's storage forms."""
    return max(v for k, v in errs_of_cell.items() if k != "fp64")


def inside(errs_of_cell):
    return worst(errs_of_cell) <= INSIDE


CASES = pytest.mark.parametrize("case", list(V.SHAPES))


@CASES
def test_node_lists_and_kink_rows(case):
    c = V.base(case)
    assert 0 < len(c["probes"]) <= V.MAX_PROBES and 0 < len(c["obs"]) <= V.MAX_OBS and c["r0"] in c["probes"]
    a = c["a_hat"].astype(np.float64)
    for variant in V.variants(case)[1:]:
        _, w = V.inputs(case, variant)
        z = a @ (c["x"].astype(np.float64) @ w["W1"].astype(np.float64)) + w["b1"].astype(np.float64)
        if variant == "kink2":
            z = a @ (np.maximum(z, 0.0) @ w["W2"].astype(np.float64)) + w["b2"].astype(np.float64)
        # every unit of the row within an fp32 rounding of its bias of zero
        assert np.abs(z[c["r0"]]).max() <= 2.0 ** -23 * np.abs(w["b2" if variant == "kink2" else "b1"]).max()


@CASES
def test_oracle_does_not_move_under_the_rescalings(case):
    refs, moved, _ = table(case)
    for v, ref in refs.items():
        assert np.isfinite(ref).all() and ref.max() > 0 and (ref > 0).sum() > 20, v
        assert (ref == 0).any() or V.base(case)["depth"] == 3, v          # (three hops reach every observed node of G)
    bad = {k: m for k, m in moved.items() if m != 0.0}
    assert not bad, bad


@CASES
def test_plain_fp64_restatement_agrees_with_the_oracle(case):
    _, _, errs = table(case)
    bad = {k: e["fp64"] for k, e in errs.items() if not e["fp64"] <= 1e-6}
    print(case, "largest |delta_fp64 - oracle| / max:", max(e["fp64"] for e in errs.values()))
    assert not bad, bad


@CASES
def test_committed_fixtures_reproduce(case):
    refs, _, errs = table(case)
    gold = committed_model()
    with np.load(REF_FILE, allow_pickle=False) as g:
        c = V.base(case)
        assert np.array_equal(g[f"{case}.probes"], c["probes"]) and np.array_equal(g[f"{case}.obs"], c["obs"])
        for v, ref in refs.items():
            # (another BLAS may sum in another order: the oracle's own fp64 noise, 1e-10 of the largest score at the most)
            assert np.abs(g[f"{case}.{v}"] - ref).max() <= 1e-10 * ref.max(), v
    assert {k for k in gold if k.startswith(case + ".")} == set(errs)
    for key, e in errs.items():
        assert set(gold[key]) == set(e), key
        for name, val in e.items():
            if name == "fp64":
                continue
            # 10 %, and a floor of 1e-8 of the largest score under which an error is the restatement's own fp64 noise
            assert abs(gold[key][name] - val) <= 0.10 * max(val, gold[key][name]) + 1e-8, (key, name, gold[key][name], val)


@CASES
def test_reference_cells_are_inside_the_domain(case):
    """k = 0 is inside for every case and variant, kink rows included; k = +-4 without a kink row is inside for M, R and A."""
    gold = committed_model()
    for v in V.variants(case):
        key = V.cell_key(case, v, None, 0)
        assert inside(gold[key]), (key, gold[key])
    if case in ("M", "R", "A"):
        for t in V.transforms(case, "plain"):
            for k in (-4, -2, -1, 1, 2, 4):
                key = V.cell_key(case, "plain", t, k)
                assert inside(gold[key]), (key, gold[key])


def write():
    model, arrays = {}, {}
    for case in V.SHAPES:
        refs, moved, errs = table(case)
        assert all(m == 0.0 for m in moved.values()), case
        model.update(errs)
        c = V.base(case)
        arrays[f"{case}.probes"], arrays[f"{case}.obs"] = c["probes"], c["obs"]
        for v, ref in refs.items():
            arrays[f"{case}.{v}"] = ref
        print(case, "done:", len(errs), "cells,", sum(inside(e) for e in errs.values()), "inside")
    with open(MODEL_FILE, "w") as fh:
        json.dump({k: {n: float(f"{v:.4e}") for n, v in e.items()} for k, e in sorted(model.items())}, fh, indent=1)
        fh.write("\n")
    np.savez_compressed(REF_FILE, **arrays)
    print("wrote", MODEL_FILE, os.path.getsize(MODEL_FILE), "bytes;", REF_FILE, os.path.getsize(REF_FILE), "bytes")


if __name__ == "__main__":
    if "--write" in sys.argv:
        write()
    else:
        sys.exit("usage: python tests/test_value_domain_cpu.py --write")

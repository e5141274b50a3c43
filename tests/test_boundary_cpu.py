"""The ladder graphs of boundary_cases.py do what they claim -- exact row, column and member-list lengths, incidence records
for short_ladder and none for hub_ladder -- and the MUTATION MARGIN: remove any one weighted entry of a ladder row (or add its
weight onto its neighbour) and the fp64 reference of that row moves by at least 100 x the tolerance test_boundary_gpu.py holds
the kernels to (for the fp32 modes: 4 x the oracle's own fp32-to-fp64 error).  That is what shows that the GPU tests would
fail on a dropped or doubled entry at a cut.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import boundary_cases as B
from oracle import linkteller_oracle as O

MARGIN = 100.0
MARGIN_FP32 = 4.0
# The member-ladder check is this suite's own addition.  A member of the 257-list is 1 / 257 of its cell when the terms add up
# coherently (they nearly do: every member forwards the same perturbed row through its own ReLU pattern), so 1e5 / 257 = 389 x
# the tolerance is the most a lost member can move it, and less where the member's ReLU pattern passes little of it or its
# term stands across the sum (measured: 11.4 x at the weakest of the 62 tested members per model shape, 135 x at C = 8).  10 x still fails the
# GPU test tenfold.
MARGIN_MEMBER = 10.0
_smallest = {}


def _note(key, ratio):
    _smallest[key] = min(_smallest.get(key, np.inf), float(ratio))


@pytest.mark.parametrize("name", ["hub", "short"])
def test_ladder_lengths_are_exact(name):
    g = B.graph_of(name)
    a = g.a
    assert a.has_sorted_indices and all(np.all(np.diff(a.indices[a.indptr[r]:a.indptr[r + 1]]) > 0) for r in range(g.n))
    assert np.all(a.data > 0)
    row_len = np.diff(a.indptr)
    col_len = np.bincount(a.indices, minlength=g.n)
    want_rows = [d for d in B.LADDER if name == "hub" or d <= B.LT_ROW_SEG]
    want_cols = [c for c in B.LADDER if name == "hub" or c <= B.LT_BIG_RV + 1]
    assert sorted(g.u) == want_rows and sorted(g.v) == want_cols
    for d, u in g.u.items():
        cols = a.indices[a.indptr[u]:a.indptr[u + 1]]
        assert row_len[u] == d and col_len[u] == 0 and np.all(cols < B.N_POOL)
        if d:
            w = a.data[a.indptr[u]:a.indptr[u + 1]]
            assert abs(w.sum() - 1.0) < 1e-12
            assert np.all(w[B.special_positions(d)] >= B.SPECIAL_SHARE - 1e-15)
    csc = a.tocsc()
    csc.sort_indices()
    for c, v in g.v.items():
        rows = csc.indices[csc.indptr[v]:csc.indptr[v + 1]]
        assert col_len[v] == c and row_len[v] == 0 and np.all(rows < B.N_POOL)
        if c:
            w = csc.data[csc.indptr[v]:csc.indptr[v + 1]]
            assert abs(w.sum() - 1.0) < 1e-12 and np.all(w[B.special_positions(c)] >= B.SPECIAL_SHARE - 1e-15)
    # every constant's K - 1, K, K + 1 is on both ladders (short_ladder: up to its caps)
    for k in B.POWERS:
        for s in (-1, 0, 1):
            assert (k + s in g.u) == (name == "hub" or k + s <= B.LT_ROW_SEG)
            assert (k + s in g.v) == (name == "hub" or k + s <= B.LT_BIG_RV + 1)
    if name == "short":
        assert row_len.max() == B.LT_ROW_SEG
    else:
        assert row_len.max() == 2 * B.LT_L2_CHUNK + 1
        # the 2-hop paths u_d -> r -> v_c exist: both ladders use the one pool
        assert len(np.intersect1d(g.row_sets[1025], g.col_sets[513])) > 0


def test_member_ladder_is_exact():
    g = B.hub_ladder()
    csc = g.a.tocsc()
    hub_row = g.row_sets[B.HUB]
    heavy = light = 0
    for (m, kind), node in g.w.items():
        col = csc.indices[csc.indptr[node]:csc.indptr[node + 1]]
        assert len(np.intersect1d(col, hub_row)) == m, (m, kind)
        assert len(col) == (600 if kind == "heavy" else m + 28)
        heavy += len(col) > B.LT_BIG_RV
        light += len(col) <= 100
    assert sorted({m for m, _ in g.w}) == sorted(B.MEMBERS)
    assert heavy >= len(B.MEMBERS) and light >= 5
    probes, obs = B.node_lists("hub")
    assert (obs == g.u[B.HUB]).sum() == 2 and set(g.w.values()) <= set(probes.tolist())
    assert g.u[513] in obs and g.u[257] in obs          # "one chunk plus one" of the C <= 4 and C <= 8 buckets
    big = sum(1 for v in probes if csc.indptr[v + 1] - csc.indptr[v] > B.LT_BIG_RV)
    assert big <= B.LT_BIG_SLOTS                        # every big probe gets its slot: 512 against 513 decides one


def _records(g):
    from linkteller_amd import _lib
    n, nnz, rp, ci, va = B.csr32(g)
    meta = np.zeros(4 * n, dtype=np.int32)
    words = C.c_int64(-1)
    rc = _lib.lib().lt_graph_records_host(n, nnz, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, meta.ctypes.data, None, 0,
                                          C.byref(words))
    return rc, meta.reshape(n, 4), words.value


def test_short_ladder_gets_records_and_hub_ladder_is_refused():
    s = B.short_ladder()
    rc, meta, words = _records(s)
    assert rc == 0 and words > 0
    inc = B.incidences(s.a)
    assert np.array_equal(meta[:, 3], inc)
    assert 4000 <= inc.max() <= B.LT_DL_MAX_T and inc.argmax() == s.v[B.LT_BIG_RV + 1]
    rc, _, _ = _records(B.hub_ladder())
    assert rc == B.LT_ERR_UNSUPPORTED
    # the cap itself: the same graph with that node at exactly LT_DL_MAX_T incidences keeps its records, one more loses them
    at_cap, past = B.short_ladder_at(B.LT_DL_MAX_T), B.short_ladder_at(B.LT_DL_MAX_T + 1)
    assert B.incidences(at_cap.a).max() == B.LT_DL_MAX_T and B.incidences(past.a).max() == B.LT_DL_MAX_T + 1
    rc, meta, _ = _records(at_cap)
    assert rc == 0 and meta[:, 3].max() == B.LT_DL_MAX_T
    assert _records(past)[0] == B.LT_ERR_UNSUPPORTED


# ---- the mutation margin ----------------------------------------------------------------------------------------------------
def _mutations(g):
    for d, u in B.ladder_rows(g):
        for pos in B.special_positions(d):
            for kind in ("drop", "double"):
                if kind == "double" and d < 2:
                    continue
                yield d, u, pos, kind


@pytest.mark.parametrize("name", ["hub", "short"])
def test_mutation_margin_of_the_spmm(name):
    """Row u of A S, with and without bias + ReLU, at the three widths the GPU test uses, against 1e-5 max(1, |want|)."""
    g = B.graph_of(name)
    a = B.f32_values(g.a)
    for ncols in B.SPMM_COLS:
        s, b, prod = B.spmm_inputs(name, ncols)
        s64 = s.astype(np.float64)
        for d, u, pos, kind in _mutations(g):
            row = B.mutate(a, u, pos, kind)[u] @ s64
            for epilogue in (False, True):
                want = B.spmm_want(name, ncols, epilogue)
                tol = 1e-5 * max(1.0, np.abs(want).max())
                got = np.maximum(row + b, 0) if epilogue else row
                move = np.abs(np.asarray(got).ravel() - want[u]).max()
                _note(f"spmm.{name}", move / tol)
                assert move >= MARGIN * tol, (ncols, d, pos, kind, epilogue, move / tol)
    print(f"smallest SpMM margin on {name}: {_smallest[f'spmm.{name}']:.1f} x the tolerance")


def _rounds(g, lengths=None):
    """The mutations in rounds of one per ladder row: a ladder node's column is empty, so nothing but its own row of any result
    reads its row, and one evaluation of the oracle serves one mutation of every row at once (the callers assert that every
    other row keeps its bits)."""
    per_row = {}
    for d, u, pos, kind in _mutations(g):
        if lengths is None or d in lengths:
            per_row.setdefault(u, []).append((d, pos, kind))
    for k in range(max(len(v) for v in per_row.values())):
        yield [(u,) + v[k] for u, v in per_row.items() if k < len(v)]


def _apply(a, batch):
    for u, d, pos, kind in batch:
        a = B.mutate(a, u, pos, kind)
    return a


@pytest.mark.parametrize("h,c", B.MODEL_SHAPES)
def test_mutation_margin_of_the_logits(h, c):
    """Row u of the fp64 logits (oracle.gcn_forward on the mutated adjacency) against 2e-5 max|logits| + 1e-6."""
    torch.set_num_threads(1)
    g = B.hub_ladder()
    ref = B.oracle_logits("hub", h, c)
    tol = 2e-5 * np.abs(ref).max() + 1e-6
    P = {k: torch.from_numpy(v).double() for k, v in B.weights(h, c).items()}
    xt = torch.from_numpy(B.features("hub")).double()
    ladder = np.array(sorted(g.u.values()))
    others = np.setdiff1d(np.arange(g.n), ladder)
    seen = 0
    for batch in _rounds(g):
        got = O.gcn_forward(xt, O.to_torch_sparse(_apply(g.a, batch)).double(), P).numpy()
        assert np.array_equal(got[others], ref[others])
        for u, d, pos, kind in batch:
            move = np.abs(got[u] - ref[u]).max()
            _note(f"logits.{h}.{c}", move / tol)
            assert move >= MARGIN * tol, (d, pos, kind, move / tol)
            seen += 1
    assert seen == sum(1 for _ in _mutations(g))
    print(f"smallest logits margin at H = {h}, C = {c}: {_smallest[f'logits.{h}.{c}']:.1f} x the tolerance")


@pytest.mark.parametrize("h,c", B.MODEL_SHAPES)
def test_mutation_margin_of_the_influence_matrix(h, c):
    """Column u of the fp64 influence matrix over the GPU test's probe list, for the rows of 129, 257 and 1025 entries at d - 1
    and at the segment cuts, and the row of probe v_c over the observed list for the last CSC entry of the columns of 129 and
    513 entries: at least 100 x 1e-5 x the matrix maximum (DELTA's bound) and 4 x the oracle's own fp32-to-fp64 error on
    the case (the fp32 modes' noise unit)."""
    g = B.hub_ladder()
    probes, obs = B.node_lists("hub")
    ref64 = B.oracle_matrix("hub", h, c, "float64")
    e32 = np.abs(B.oracle_matrix("hub", h, c, "float32") - ref64).max()
    x, w = B.features("hub"), B.weights(h, c)
    base = O.RestrictedOracle(x, g.a, w).rows(probes, obs, B.DELTA)
    assert np.abs(base - ref64).max() <= 1e-9 * ref64.max()          # the restricted oracle is the verbatim one
    tol = 1e-5 * ref64.max()
    cols = {g.u[d]: int(np.flatnonzero(obs == g.u[d])[0]) for d in (129, 257, 1025)}
    for batch in _rounds(g, (129, 257, 1025)):
        us = [b[0] for b in batch]
        got = O.RestrictedOracle(x, _apply(g.a, batch), w).rows(probes, us, B.DELTA)
        for k, (u, d, pos, kind) in enumerate(batch):
            move = np.abs(got[:, k] - base[:, cols[u]]).max()
            _note(f"influence.{h}.{c}", move / tol)
            _note(f"influence32.{h}.{c}", move / e32)
            assert move >= MARGIN * tol and move >= MARGIN_FP32 * e32, (d, pos, kind, move / tol, move / e32)
    for cl in (129, 513):
        v = g.v[cl]
        i = int(np.flatnonzero(probes == v)[0])
        for kind in ("drop", "double"):
            got = O.RestrictedOracle(x, B.mutate_column(g.a, v, cl - 1, kind), w).rows([v], obs, B.DELTA)[0]
            move = np.abs(got - base[i]).max()
            _note(f"influence.{h}.{c}", move / tol)
            _note(f"influence32.{h}.{c}", move / e32)
            assert move >= MARGIN * tol and move >= MARGIN_FP32 * e32, (cl, kind, move / tol, move / e32)
    print(f"smallest influence margin at H = {h}, C = {c}: {_smallest[f'influence.{h}.{c}']:.1f} x DELTA's tolerance, "
          f"{_smallest[f'influence32.{h}.{c}']:.1f} x the oracle's fp32 error ({e32:.3e}; matrix maximum {ref64.max():.3f})")


@pytest.mark.parametrize("h,c", B.MODEL_SHAPES)
def test_mutation_margin_of_the_member_ladder(h, c):
    """A member of row(u_1025) /\\ column(w_m) carries 1 / 1000 of the hub row: against the whole matrix's maximum a lost member
    would hide.  The GPU test therefore also holds the member-ladder cells (w_m, u_1025) -- an influence matrix in their own
    right -- to 1e-5 of THEIR largest score.  Losing the member at list position 0, 63, 64, 127, 128 or m - 1 (a refill that
    skips one) moves its cell by at least MARGIN_MEMBER = 10 x that."""
    g = B.hub_ladder()
    probes, obs = B.node_lists("hub")
    rows, col = B.member_cells()
    ref64 = B.oracle_matrix("hub", h, c, "float64")
    tol = 1e-5 * ref64[rows, col].max()
    x, w = B.features("hub"), B.weights(h, c)
    u = g.u[B.HUB]
    csc = g.a.tocsc()
    csc.sort_indices()
    worst = np.inf
    for (m, kind), node in sorted(g.w.items()):
        column = csc.indices[csc.indptr[node]:csc.indptr[node + 1]]
        members = np.flatnonzero(np.isin(column, g.row_sets[B.HUB]))          # CSC positions of the members, in row order
        i = int(np.flatnonzero(probes == node)[0])
        for k in sorted({0, 63, 64, 127, 128, m - 1} & set(range(m))):
            got = O.RestrictedOracle(x, B.mutate_column(g.a, node, int(members[k]), "drop"), w).rows([node], [u], B.DELTA)[0, 0]
            move = abs(got - ref64[i, col])
            worst = min(worst, move / tol)
            assert move >= MARGIN_MEMBER * tol, (m, kind, k, move / tol)
    print(f"smallest member-ladder margin at H = {h}, C = {c}: {worst:.1f} x 1e-5 of the largest member-ladder score "
          f"({ref64[rows, col].max():.3e})")

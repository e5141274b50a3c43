"""The references of test_wide2_gpu.py can see what they are there to see (wide2_cases.py).  No GPU.

  A. the inputs of the lt_wide_combine cases have bite: summed in reversed slice order, or with the classes reversed, the
     restatement gives other bits; the odd pairs are what they claim to be;
  B. the fp64 fma of the restatement is correctly rounded, the fp64 difference vectors have the oracle's norms, and a lost or doubled entry at a cut of the rows of 129, 257 and 1025
     entries moves the affected pair's vector by at least 100 x the gate the GPU test holds every component to;
  C. the shapes cut the slices the issue lists, and the slice limit is where lt_wide_combine puts it."""
import numpy as np
import pytest

import boundary_cases as B
import wide2_cases as W

MARGIN = 100.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vec,C,n_pairs", W.COMBINE_CASES, ids=lambda v: str(v))
def test_combine_inputs_have_bite(n_vec, C, n_pairs):
    v = W.combine_case(n_vec, C, n_pairs)
    for delta in W.COMBINE_DELTAS:
        want = W.combine_restated(list(v), C, delta, None, 1, 1)
        assert want.dtype == np.float32 and want.shape == (n_pairs,) and np.isfinite(want).all() and not np.signbit(want).any()
        if n_vec >= 3:          # (two slices have one order: the sum is commutative)
            other = W.combine_restated(list(v[::-1]), C, delta, None, 1, 1)
            assert (_bits(other) != _bits(want)).any(), "the slice order does not show"
        if C >= 2:
            other = W.combine_restated(list(v[:, :, ::-1]), C, delta, None, 1, 1)
            assert (_bits(other) != _bits(want)).any(), "the class order does not show"
    # a negative delta flips every d and no square
    assert np.array_equal(_bits(W.combine_restated(list(v), C, -1e-4, None, 1, 1)), _bits(W.combine_restated(list(v), C, 1e-4, None, 1, 1)))


def test_combine_odd_pairs():
    tiny = np.finfo(np.float32).tiny
    for n_vec in (1, 2, 3, W.MAX_VEC):
        v = W.combine_inputs(n_vec, W.MAX_C, 257)
        got = W.combine_restated(list(v), W.MAX_C, 1e-4, None, 1, 1)
        assert np.all(v[:, 1] == 0) and np.signbit(v[:, 1]).any() and not np.signbit(v[:, 1]).all()
        assert _bits(got)[1] == 0 and _bits(got)[2] == 0                      # +0.0: all zeros; a square that underflows
        assert 0 < abs(v[0, 2, 0]) < tiny and 0 < abs(v[0, 3, -1]) < tiny and np.abs(v[0, 3, :-1]).min() >= tiny
        if n_vec >= 2:
            assert np.any(v[0, 0] != 0) and np.array_equal(v[1, 0], -v[0, 0]) and _bits(got)[0] == 0
            s = np.float32(v[0, 4, 0] + v[1, 4, 0])
            assert 0 < s < tiny and 0 < s / np.float32(1e-4) < tiny          # a subnormal sum and a subnormal quotient
        assert (got[5:] > 0).all()


def test_combine_chain_is_one_chain():
    """first, middle, last over classes 3 + 3 + 2 is the one fma chain of the 8 classes; the running sum of the middle call is no
    square root."""
    v = W.combine_inputs(3, 8, 257)
    cuts = ((0, 3), (3, 6), (6, 8))
    ss = None
    for k, (c0, c1) in enumerate(cuts):
        ss = W.combine_restated([s[:, c0:c1] for s in v], c1 - c0, 1e-4, ss, int(k == 0), int(k == 2))
        if k == 1:
            mid = ss.copy()
    want = W.combine_restated(list(v), 8, 1e-4, None, 1, 1)
    assert np.array_equal(_bits(ss), _bits(want))
    assert (_bits(mid) != _bits(np.sqrt(mid))).any() and (mid[5:] <= want[5:] ** 2 * (1 + 1e-6)).all()


# ---- B ------------------------------------------------------------------------------------------------------------------------
def test_fma64_is_correctly_rounded():
    """Against exact rationals: operands of order one, sums of every relative size, and near-total cancellations."""
    from fractions import Fraction
    rng = np.random.RandomState(3)
    n = 4000
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    c = rng.standard_normal(n) * 10.0 ** rng.uniform(-17, 2, n)
    c[: n // 4] = -(a * b)[: n // 4] * (1 + 1e-15 * rng.standard_normal(n // 4))
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(W.fma64(a, b, c), want)
    assert (a * b + c != want).sum() > n // 10          # (the unfused form is another number in many of them)
    x, w = rng.standard_normal((7, 5)), rng.standard_normal((5, 3))
    chain = np.zeros((7, 3))
    for i in range(7):
        for j in range(3):
            acc = 0.0
            for k in range(5):
                acc = float(Fraction(x[i, k]) * Fraction(w[k, j]) + Fraction(acc))
            chain[i, j] = acc
    assert np.array_equal(W.dense_chain(x, w), chain)


@pytest.mark.parametrize("h,c", B.MODEL_SHAPES)
def test_difference_vectors_have_the_oracle_norms(h, c):
    """The row norms of diff_vectors64 against B.oracle_matrix(..., "float64"), to 1e-12 of the largest score.  (The same
    quantity with numpy's and scipy's own summation orders -- blas_vectors64 -- stands 3.6e-12, 6.3e-12 and 2.0e-12 from the
    oracle: one rounding of a logit of 1.4 over DELTA = 1e-4 is 1.6e-12 of a largest score of 0.97.  In the oracle's order the
    norms agree to 9e-17.)"""
    ref64 = B.oracle_matrix("hub", h, c, "float64")
    vec = W.diff_vectors64("hub", h, c)
    probes, obs = B.node_lists("hub")
    assert vec.shape == (len(probes), len(obs), c)
    err = np.abs(np.linalg.norm(vec, axis=2) - ref64).max() / ref64.max()
    print(f"H {h} C {c}: |norm(diff_vectors64) - oracle| / max = {err:.2e}")
    assert err <= 1e-12
    assert np.array_equal(np.linalg.norm(vec, axis=2) == 0, ref64 == 0)
    # both signs, every class: a swapped or negated component shows
    assert (vec > 0).any(axis=(0, 1)).all() and (vec < 0).any(axis=(0, 1)).all()


@pytest.mark.parametrize("h,c", B.MODEL_SHAPES)
def test_difference_vectors_in_another_order(h, c):
    """The same vectors with the products as numpy and scipy sum them: within 1e-9 of the largest score, component by component."""
    ref64 = B.oracle_matrix("hub", h, c, "float64")
    vec = W.blas_vectors64("hub", h, c)
    probes, obs = B.node_lists("hub")
    assert np.abs(vec - W.diff_vectors64("hub", h, c)).max() <= 1e-9 * ref64.max()
    assert np.array_equal(np.linalg.norm(vec, axis=2) == 0, ref64 == 0)
    # A[u] @ (the difference of H1 W2) is the same vector: what the mutation test below evaluates
    a = B.f32_values(B.hub_ladder().a)
    hid = W.hidden_differences64("hub", h, c)
    via = np.stack([a[obs] @ hid[i] for i in range(len(probes))])
    assert np.abs(via - vec).max() <= 1e-9 * ref64.max()


@pytest.mark.parametrize("h,c", B.MODEL_SHAPES)
def test_mutation_margin_of_the_difference_vectors(h, c):
    """Drop or double the entry at a weighted position of the rows of 129, 257 and 1025 entries: over the probes, the largest
    component of the affected pair's fp64 vector moves by at least 100 x 1e-5 x the largest score -- the gate
    test_wide2_gpu.py holds every component of vec / DELTA to."""
    g = B.hub_ladder()
    a = B.f32_values(g.a)
    hid = W.hidden_differences64("hub", h, c)
    tol = W.GATE * B.oracle_matrix("hub", h, c, "float64").max()
    worst = np.inf
    for d in (129, 257, 1025):
        u = g.u[d]
        base = np.stack([np.asarray(a[u] @ hv).ravel() for hv in hid])
        for pos in B.special_positions(d):
            for kind in ("drop", "double"):
                row = B.mutate(a, u, pos, kind)[u]
                move = np.abs(np.stack([np.asarray(row @ hv).ravel() for hv in hid]) - base).max()
                worst = min(worst, move / tol)
                assert move >= MARGIN * tol, (d, pos, kind, move / tol)
    print(f"smallest vector margin at H = {h}, C = {c}: {worst:.1f} x the component gate")


# ---- C ------------------------------------------------------------------------------------------------------------------------
def test_shapes_cut_the_slices_they_name():
    widths = {hc: ([s1 - s0 for s0, s1 in W.slices(*hc)[0]], [t1 - t0 for t0, t1 in W.slices(*hc)[1]]) for hc in W.WIDE_SHAPES}
    assert widths == {(257, 2): ([256, 1], [2]), (260, 9): ([256, 4], [8, 1]), (512, 8): ([256, 256], [8]),
                      (513, 3): ([256, 256, 1], [3]), (64, 17): ([64], [8, 8, 1]), (256, 24): ([256], [8, 8, 8])}
    assert len(W.slices(8192, 2)[0]) == W.MAX_VEC and len(W.slices(8193, 2)[0]) == W.MAX_VEC + 1
    for h, c in W.WIDE_SHAPES:
        assert B.weights(h, c)["W1"].shape == (B.F, h) and B.weights(h, c)["W2"].shape == (h, c)


def test_relation_weights():
    for kind, cut in (("hidden", 256), ("classes", 8)):
        w, narrow = W.relation_weights(kind)
        wc, _ = W.relation_weights(kind, control=True)
        block = (lambda m: m["W2"][cut:]) if kind == "hidden" else (lambda m: m["W2"][:, cut:])
        assert not block(w).any() and block(wc).all() and np.abs(block(wc)).max() < 1e-2
        assert narrow["W2"].shape == ((256, 2) if kind == "hidden" else (64, 8)) and narrow["W2"].any()


def test_tiny_graph_of_the_slice_limit():
    t = W.tiny()
    assert t.a.shape == (W.TINY_N, W.TINY_N) and t.x.shape == (W.TINY_N, W.TINY_F) and len(t.probes) > 8
    ref = W.tiny_ref64(8192, 2)
    assert ref.shape == (len(t.probes), W.TINY_N) and ref.max() > 0 and (ref == 0).any()
    assert np.array_equal(ref[-1], ref[np.flatnonzero(t.probes == t.probes[-1])[0]])

"""The conditions of the inputs of test_gcn3_shapes_gpu.py, checked without a GPU (gcn3_shape_cases.py):

  * the width and class ladders reach every lane-group size of lt_lpr_for from 1 to 64 for Hp1, Hp2 and Cp, full groups and groups
    one column over the previous one, and every residue of H and C mod 4 -- from a restatement of lt_round_up / lt_lpr_for that is
    compared with the library's source text;
  * every (graph, shape) of the ladder has a positive largest fp64 score and between a tenth and nine tenths exact zeros: the
    conditions of the GPU file's zero check, not measurements;
  * the graph of 516 bitmap words has probes whose R2 spans all three stretches of 256 words and holds the stretches' end ids;
  * the kink rows sit at their kinks, the storage model puts them inside the value domain, and the fp64 oracle does not move by a
    bit under the power-of-two rescaling of layer 2."""
import functools
import os
import re

import numpy as np
import pytest

import gcn3_shape_cases as S
from conftest import REPO

LPRS = {1, 2, 4, 8, 16, 32, 64}


# ---- 1. coverage -----------------------------------------------------------------------------------------------------------------
def test_width_rules_restate_the_library():
    src = open(os.path.join(REPO, "linkteller_amd", "csrc", "lt_rows.hip.h")).read()
    body = re.search(r"static inline int lt_lpr_for\(int Hp\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "need = Hp / 4, l = 1" in body and "while (l < need) l <<= 1" in body
    internal = open(os.path.join(REPO, "linkteller_amd", "csrc", "lt_internal.h")).read()
    assert "lt_round_up(int x, int m) { return (x + m - 1) / m * m; }" in internal
    gcn3 = open(os.path.join(REPO, "linkteller_amd", "csrc", "lt_gcn3.hip")).read()
    assert "b->Hp1 = lt_round_up(H1, 4); b->Hp2 = lt_round_up(H2, 4);" in gcn3 and "b->Cp = lt_round_up(C, 4);" in gcn3
    assert [S.round_up4(v) for v in (1, 3, 4, 5, 253, 256)] == [4, 4, 4, 8, 256, 256]
    assert [S.lpr_for(v) for v in (4, 8, 12, 16, 20, 64, 68, 128, 132, 256)] == [1, 2, 4, 4, 8, 16, 32, 32, 64, 64]


def test_ladders_cover_every_lane_group():
    assert len(S.NARROW) == 13 and len(S.WIDE) == 19 and len(set(S.LADDER)) == 32
    assert all(1 <= c <= 8 for _, _, c in S.NARROW) and all(1 <= c <= 256 for _, _, c in S.WIDE)
    assert all(1 <= h <= 256 for s, _ in S.LADDER for h in s[:2])
    for cases in (S.NARROW, S.WIDE):                     # each handle kind on its own: the stage kernels differ
        wide = cases is S.WIDE
        got = [S.lprs(s, wide) for s in cases]
        assert {g[0] for g in got} == LPRS, wide              # k3d_items1<LPR>
        assert {g[1] for g in got} == LPRS, wide              # k3_stageB / k3d_stageB<LPR> (narrow), k3dw_stageB<LPR> (wide)
    assert {S.lprs(s, True)[2] for s in S.WIDE} == LPRS          # k3dw_stageC<LPR>
    assert all(S.lprs(s, False)[2] is None for s in S.NARROW)
    hs = {h for s, _ in S.LADDER for h in s[:2]}
    cs = {c for _, _, c in S.WIDE}
    # one column over the previous group's width (the first lane of the next group holds ONE live column) ...
    assert {5, 9, 17, 33, 65, 129} <= hs and {5, 17, 33, 65, 129} <= cs
    # ... groups that are exactly full, with and without pad columns in the last lane
    assert {256, 255, 253} <= hs and {4, 16, 32, 64, 128, 255} <= cs
    # (no H1 of the ladder is a multiple of 4: the suite's older shapes are all of that kind)
    assert {h % 4 for h, _, _ in S.NARROW + S.WIDE} == {1, 2, 3} and {h % 4 for _, h, _ in S.NARROW + S.WIDE} == {0, 1, 2, 3}
    assert {c % 4 for c in cs} == {0, 1, 2, 3} == {c % 4 for _, _, c in S.NARROW}
    # every shape but three needs padding in both hidden layers; the relations and the odd-stride graph run on padded shapes only
    assert sum(1 for s, w in S.LADDER if not all(S.padded(s, w)[:2])) == 3
    for s, w in S.ER29 + S.RELATIONS:
        assert all(S.padded(s, w)[:2]) and (s, w) in S.LADDER
    assert all(S.padded(s, True)[2] for s, w in S.RELATIONS if w)


def test_er29_is_the_er_recipe():
    a, x, probes, obs, zrow = S.small_graph("er")
    a2, x2, probes2, obs2, zrow2 = S.er_recipe(32)
    assert (a != a2).nnz == 0 and np.array_equal(a.data, a2.data) and np.array_equal(x, x2)
    assert np.array_equal(probes, probes2) and np.array_equal(obs, obs2) and zrow == zrow2
    a3, x3, probes3, obs3, zrow3 = S.small_graph("er29")
    assert (a != a3).nnz == 0 and x3.shape == (300, 29) and x3.strides[0] == 29 * 4 and not x3[probes3[zrow3]].any()
    assert np.array_equal(probes, probes3) and np.array_equal(obs, obs3)
    assert S.small_params("er29", (7, 9, 3))["W1"].shape == (29, 7)


# ---- 2. the oracle's scores per case ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref64(name, shape):
    import test_gcn3_wide_attack_gpu as W
    a_hat, x, probes, obs, _ = S.small_graph(name)
    return W._oracle(a_hat, x, S.small_params(name, shape), probes, obs)


SMALL = [(g,) + c for g in S.GRAPHS for c in S.LADDER] + [("er29",) + c for c in S.ER29]


@pytest.mark.parametrize("name,shape,wide", SMALL, ids=[f"{c[0]}-{S.case_id(c[1:])}" for c in SMALL])
def test_scores_are_positive_and_zeros_are_neither_rare_nor_all(name, shape, wide):
    ref = ref64(name, shape)
    _, _, probes, obs, zrow = S.small_graph(name)
    assert ref.shape == (len(probes), len(obs)) and np.isfinite(ref).all()
    zeros = float((ref == 0).mean())
    assert ref.max() > 0 and 0.1 <= zeros <= 0.9, (ref.max(), zeros)
    assert np.all(ref[zrow] == 0)


# ---- 3. the graph of 516 bitmap words --------------------------------------------------------------------------------------------
def test_big_graph_spans_three_stretches():
    a_hat, x, probes, obs, zrow = S.big_graph()
    n = S.BIG_N
    assert a_hat.shape == (n, n) and (n + 31) // 32 == 516 and x.shape == (n, 32)
    assert {0, 8191, 8192, n - 1} <= set(probes.tolist()) and len(set(probes.tolist())) < len(probes)
    assert set(S.stretch_of(S.BIG_SPECIAL).tolist()) == {0, 1, 2} and S.BIG_SPECIAL[-1] == n - 1
    r2 = {int(v): S.hops(a_hat, int(v), 2) for v in set(probes.tolist())}
    # (A A)'s pattern, the definition itself, on two probes
    aa = (a_hat != 0).astype(np.int64)
    aa = (aa @ aa).tocsc()
    for v in (0, int(probes[-1])):
        assert np.array_equal(np.sort(aa[:, v].indices), r2[v])
    three = [v for v, m in r2.items() if set(S.stretch_of(m).tolist()) == {0, 1, 2}]
    assert len(three) >= 2, three
    assert any(set(S.BIG_SPECIAL) <= set(m.tolist()) for m in r2.values())
    # members in every stretch BEHIND the first one, several of them: a lost carry moves more than one item
    for v in three[:2]:
        counts = np.bincount(S.stretch_of(r2[v]), minlength=3)
        assert counts.min() >= 1 and counts[0] >= 2, (v, counts)
    assert not x[probes[zrow]].any()
    reach = np.unique(np.concatenate([S.hops(a_hat, int(v), 3) for v in probes]))
    assert np.isin(obs, reach).sum() >= 40 and (~np.isin(obs, reach)).sum() >= 8 and len(set(obs.tolist())) < len(obs)


@pytest.mark.parametrize("shape,wide", S.BIG, ids=[S.case_id(c) for c in S.BIG])
def test_big_graph_scores(shape, wide):
    import test_gcn3_wide_attack_gpu as W
    a_hat, x, probes, obs, zrow = S.big_graph()
    ref = W._oracle(a_hat, x, S.big_params(shape), probes, obs)
    zeros = float((ref == 0).mean())
    assert ref.max() > 0 and 0.1 <= zeros <= 0.9, (ref.max(), zeros)
    assert np.all(ref[zrow] == 0)
    # cells that only the second and third stretch of a probe's R2 can serve are non-zero: observed 16383 / 16384 / n - 1 of probe 0
    col = [int(np.flatnonzero(obs == s)[0]) for s in S.BIG_SPECIAL]
    assert np.all(ref[0, col] > 0)


@pytest.mark.parametrize("shape", S.ALL_PROBES, ids=lambda s: "x".join(map(str, s)))
def test_every_node_as_a_probe_scores(shape):
    import test_gcn3_wide_attack_gpu as W
    a_hat, x, _, obs, _ = S.small_graph("er")
    ref = W._oracle(a_hat, x, S.small_params("er", shape), np.arange(300, dtype=np.int32), obs)
    zeros = float((ref == 0).mean())
    assert ref.shape == (300, len(obs)) and ref.max() > 0 and 0.1 <= zeros <= 0.9, zeros


# ---- 4. a row at its kinks -------------------------------------------------------------------------------------------------------
KINK_CASES = [(w, s, v) for w, s, _ in S.KINKS for v in S.VARIANTS]
KINK_IDS = ["x".join(map(str, w)) + f"-seed{s}-{v}" for w, s, v in KINK_CASES]


def test_kink_cases_take_the_lists_of_case_g():
    import value_domain_cases as V
    c, g = S.kink_base(), V.base("G")
    assert c["a_hat"] is g["a_hat"] and c["x"] is g["x"] and c["r0"] == g["r0"] and c["r0"] in c["probes"]
    # the weights: base()'s own draw at base()'s seed and widths
    w = S.kink_weights((32, 16, 2), V.WEIGHT_SEED["G"])
    assert all(np.array_equal(w[k], g["w"][k]) for k in S.KEYS)
    wk = S.kink_weights((32, 16, 2), V.WEIGHT_SEED["G"], "kink2")
    assert all(np.array_equal(wk[k], V.kink_row("G", 2)[k]) for k in S.KEYS)
    wr = S.kink_weights((32, 16, 2), V.WEIGHT_SEED["G"], "kink", k=8)
    want = V.rescale_units(V.kink_row("G", 1), 8, 2, np.arange(0, 16, 2))
    assert all(np.array_equal(wr[k], want[k]) for k in S.KEYS)


@pytest.mark.parametrize("widths,seed,variant", KINK_CASES, ids=KINK_IDS)
def test_kink_rows_storage_model_and_rescaling(widths, seed, variant):
    import test_value_domain_cpu as VC
    import value_domain_model as MV
    c = S.kink_base()
    w = S.kink_weights(widths, seed, variant)
    if variant != "plain":
        layer = 2 if variant == "kink2" else 1
        z = S.pre_activation(c, w, layer)
        # every unit of the row within an fp32 rounding of its bias of zero (test_value_domain_cpu.test_node_lists_and_kink_rows)
        assert np.abs(z[c["r0"]]).max() <= 2.0 ** -23 * np.abs(w[f"b{layer}"]).max()
    ref = VC.oracle("G", c["x"], w)
    assert np.isfinite(ref).all() and ref.max() > 0 and (ref > 0).sum() > 20
    # what the fixed-point product rows alone cost (value_domain_model.py), relative to the largest score: inside the domain, so
    # the GPU file's 1e-5 gate is a statement about the kernels
    err = np.abs(MV.delta_fp64(c["a_hat"], c["x"], w, c["probes"], c["obs"], S.DELTA, rows="rows31") - ref).max() / ref.max()
    e64 = np.abs(MV.delta_fp64(c["a_hat"], c["x"], w, c["probes"], c["obs"], S.DELTA) - ref).max() / ref.max()
    print(f"gcn3 kink {widths} seed {seed} {variant}: rows31 {err:.2e} fp64 {e64:.2e}")
    assert e64 <= 1e-6 and err <= VC.INSIDE, (err, e64)
    if variant == "plain":
        assert err < 1e-7
    # the oracle does not move by a bit when the even units of layer 2 are rescaled by 2^k
    for k in S.EXACT_KS:
        assert np.array_equal(VC.oracle("G", c["x"], S.kink_weights(widths, seed, variant, k)), ref), k

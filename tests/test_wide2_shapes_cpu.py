"""The conditions of the inputs of test_wide2_shapes_gpu.py, checked without a GPU (wide2_shape_cases.py):

  * the (H, C) ladder reaches every lane-group size of lt_lpr_for from 1 to 64 on the hidden side and on the class side, each on its
    own, every residue mod 4, widths one column over a full group, full widths, class counts on both sides of every 64-column tile
    edge of the product dS2x = dH1x W2 and inner dimensions below one 16-deep tile, behind full tiles and beyond the 128-term fold
    -- from restatements of the library's rules that are compared with its source text;
  * every (graph, shape) of the ladder has a positive largest fp64 score, between a tenth and nine tenths exact zeros and a zero
    row for the all-zero probe: conditions of the GPU file's checks, not measurements;
  * every storage case meets the shape rules of the form it claims, the plain fp64 restatement of `delta` agrees with the oracle
    and the storage model (value_domain_model.py) puts the case inside the value domain, so that the GPU file's 1e-5 gate is a
    statement about the kernels that read and write the stored form;
  * the graph of 516 bitmap words has cells that only an item beyond id 8192 (16384) can serve, and they are non-zero; the probes
    of the hub ladder have the column lengths the item-count test relies on."""
import os
import re

import numpy as np
import pytest

import boundary_cases as B
import gcn3_shape_cases as S
import value_domain_model as MV
import wide2_shape_cases as W
from conftest import REPO
from test_value_domain_cpu import INSIDE

LPRS = {1, 2, 4, 8, 16, 32, 64}


def _src(name):
    with open(os.path.join(REPO, "linkteller_amd", "csrc", name)) as fh:
        return fh.read()


# ---- 1. coverage -----------------------------------------------------------------------------------------------------------------
def test_width_rules_restate_the_library():
    body = re.search(r"static inline int lt_lpr_for\(int Hp\) \{(.*?)\n\}", _src("lt_rows.hip.h"), flags=re.S).group(1)
    assert "need = Hp / 4, l = 1" in body and "while (l < need) l <<= 1" in body
    assert "lt_round_up(int x, int m) { return (x + m - 1) / m * m; }" in _src("lt_internal.h")
    gcn3 = _src("lt_gcn3.hip")
    create = re.search(r'extern "C" int lt_baseline2w_create\(.*?\n\}', gcn3, flags=re.S).group(0)
    assert "b->Hp = lt_round_up(H, 4); b->Cp = lt_round_up(C, 4);" in create
    impl = re.search(r"static int influence2w_impl\(.*?\n\}", gcn3, flags=re.S).group(0)
    assert "const int lpr1 = lt_lpr_for(Hp), lprc = lt_lpr_for(Cp);" in impl
    assert "lt_launch_gemm_mdev(w.dH1x, Hp, b->W2, C, w.dS2x, Cp, (int)m_bound, w.off + nb, C, b->H, st)" in impl
    carve = re.search(r"static infl2w_ws carve2w\(.*?\n\}", gcn3, flags=re.S).group(0)
    assert f"if (chunk > {W.CAP}) chunk = {W.CAP};" in carve
    assert [W.round_up4(v) for v in (1, 3, 4, 5, 253, 256)] == [4, 4, 4, 8, 256, 256]
    assert [W.lpr_for(v) for v in (4, 8, 12, 16, 20, 64, 68, 128, 132, 256)] == [1, 2, 4, 4, 8, 16, 32, 32, 64, 64]


def test_storage_rules_restate_the_library():
    fp64 = _src("lt_fp64.hip")
    assert "return (long long)b->n * b->Hp * (long long)sizeof(double) < ((long long)32 << 20) && b->H <= 256 && b->H % 4 == 0;" in fp64
    assert "static bool fp64_big(int n, int H) { return n >= 1024 && H % GE_BN == 0; }" in fp64
    assert re.search(r"#define GE_BN 128\b", fp64)
    assert "defer = defer && H % 4 == 0 && H <= 256 && b->fd_rs != nullptr;" in fp64
    assert "float *s1x = (defer && b->S1x && b->S1qs && lt_tune().s1_f32 != 0) ? b->S1x : nullptr;" in fp64
    i8 = _src("lt_i8_split.hip.h")
    assert ("bool lt_i8_shapes_ok(int n, int H, int F) { return n >= 256 && F >= 256 && H >= 64 && H % 64 == 0 && F < (1 << 15); }"
            in i8)


def test_ladder_covers_every_lane_group_and_tile_edge():
    assert len(set(W.LADDER)) == len(W.LADDER) and all(1 <= h <= 256 and 1 <= c <= 256 for h, c in W.LADDER)
    hs, cs = {h for h, _ in W.LADDER}, {c for _, c in W.LADDER}
    assert {W.lpr_for(W.round_up4(h)) for h in hs} == LPRS            # 1. k3d_items1<LPR>
    assert {W.lpr_for(W.round_up4(c)) for c in cs} == LPRS            # 2. k3dw_stageC<LPR> / k3dw_stageC_pairs<LPR>
    assert {h % 4 for h in hs} == {0, 1, 2, 3} == {c % 4 for c in cs}  # 3.
    assert {5, 9, 17, 33, 65, 129} <= hs and {5, 9, 17, 33, 65, 129} <= cs      # 4. one column over a full group
    assert {256, 255, 253} <= hs and {4, 16, 32, 64, 128, 255, 256} <= cs       # 5. exactly full widths
    assert {63, 64, 65, 127, 128, 129, 192, 193} <= cs                          # 6. the 64-column tile edges of k_gemm_f32_mfma
    assert {1, 3, 5} <= hs and {17, 30} <= hs and {129, 253} <= hs              # 7. K = H
    # the relations run on shapes padded on both sides, one of them beyond 64 classes
    assert len(W.RELATIONS) == 4 and all(s in W.LADDER and s[0] % 4 and s[1] % 4 for s in W.RELATIONS)
    assert any(c > 64 for _, c in W.RELATIONS)
    assert all(s in W.LADDER for s in W.ER29)


# ---- 2. the oracle's scores per case ---------------------------------------------------------------------------------------------
SMALL = [(g, s) for g in W.GRAPHS for s in W.LADDER]


@pytest.mark.parametrize("name,shape", SMALL, ids=[f"{g}-{W.shape_id(s)}" for g, s in SMALL])
def test_scores_are_positive_and_zeros_are_neither_rare_nor_all(name, shape):
    ref = W.ladder_ref(name, shape)
    _, x, probes, obs, zrow = W.small_graph(name)
    assert ref.shape == (len(probes), len(obs)) and np.isfinite(ref).all()
    zeros = float((ref == 0).mean())
    assert ref.max() > 0 and 0.1 <= zeros <= 0.9, (ref.max(), zeros)
    assert not x[probes[zrow]].any() and np.all(ref[zrow] == 0)


# ---- 3. the storage cases --------------------------------------------------------------------------------------------------------
def test_storage_cases_meet_the_rules_of_their_forms():
    n = 300
    for case, (kind, f, h, c, kn, form) in W.STORAGE.items():
        nn = S.BIG_N if form.get("big") else n
        x = W.storage_case(case)["x"]
        assert x.shape == (nn, f) and 9 <= c <= 256 and h <= 256, case
        i8 = W.i8_shapes_ok(nn, h, f) and kn.get("i8_split", 1) != 0 and form["route"] == 0
        assert i8 == form["i8"], case
        if "slices" in form:
            assert len(MV.i8_slices(nn, h, f)) == form["slices"], case
        if form["route"] == 0:
            assert form["fixed"] == (W.dense_quant_shapes(nn, h) and kn.get("s1_f32", 1) != 0), case
            assert not form["deferred"], case
        else:
            # the detector's side of the rule is asserted on the GPU (the twin's route); here: an indicator matrix, few distinct
            # values per column, every row within the 384 differing columns a wave's list holds
            assert kind == "twitch" and max(len(np.unique(x[:, j])) for j in range(f)) <= 2, case
            defer = h % 4 == 0 and kn.get("defer_cref", 1) != 0
            assert form["deferred"] == defer and form["fixed"] == (defer and kn.get("s1_f32", 1) != 0), case
        assert bool(form.get("big")) == W.fp64_big(nn, h), case
    f_, h_ = W.STORAGE["f"][1:3]
    assert W.round_up4(h_) != h_ and W.STORAGE["i"][2] % 4 != 0 and W.STORAGE["j"][1] % 2 == 1
    assert W.STORAGE["c"][2] == 256                              # four 64-column tiles of H
    # cases that differ in their knobs alone share their inputs
    assert len({W.inputs_key(k) for k in ("a", "d", "e", "l")}) == 1 and len({W.inputs_key(k) for k in ("g", "k1", "k0", "h")}) == 1
    assert (S.BIG_N + 31) // 32 == 516


STORED = list(W.STORAGE)


@pytest.mark.parametrize("case", STORED)
def test_storage_model_is_inside_the_domain(case):
    """What the stored precision alone costs (value_domain_model.delta_fp64 behind the case's storage), relative to the largest
    score: at most INSIDE = a quarter of the gate.  On the feature-difference route (g, j, k) `rows31` is an ESTIMATE: the kernel
    stores S1d - cref against other row maxima (value_domain_model's docstring)."""
    c = W.storage_case(case)
    ref = W.storage_ref(case)
    zeros = float((ref == 0).mean())
    assert ref.shape == (len(c["probes"]), len(c["obs"])) and ref.max() > 0 and 0.1 <= zeros <= 0.9, (ref.max(), zeros)
    if c["zrow"] is not None:
        assert not c["x"][c["probes"][c["zrow"]]].any() and np.all(ref[c["zrow"]] == 0)
    e64 = np.abs(MV.delta_fp64(c["a_hat"], c["x"], c["w"], c["probes"], c["obs"], W.DELTA) - ref).max() / ref.max()
    assert e64 <= 1e-6, e64
    if not W.stores(case):
        print(f"wide2 storage {case}: max {ref.max():.3g} zeros {zeros:.2f} fp64 restatement {e64:.2e} (nothing stored)")
        return
    err = np.abs(MV.delta_fp64(c["a_hat"], c["x"], c["w"], c["probes"], c["obs"], W.DELTA, **W.model_kw(case)) - ref).max() / ref.max()
    print(f"wide2 storage {case}: max {ref.max():.3g} zeros {zeros:.2f} fp64 restatement {e64:.2e} model {W.model_kw(case)} {err:.2e}"
          + (" (estimate: route 1)" if c["form"]["route"] == 1 else ""))
    assert err <= INSIDE, (case, err)


@pytest.mark.parametrize("case", W.REFRESH)
def test_refresh_inputs_move_the_scores_and_stay_inside(case):
    c = W.storage_case(case)
    before = W.storage_ref(case)
    for what in ("w1", "x"):
        x, w = W.updated(case, what)
        ref = W.updated_ref(case, what)
        # (ten gates: a handle that did not follow the update cannot pass the gate of the new oracle)
        assert ref.max() > 0 and np.abs(ref - before).max() > 10 * W.GATE * ref.max(), what
        err = np.abs(MV.delta_fp64(c["a_hat"], x, w, c["probes"], c["obs"], W.DELTA, **W.model_kw(case)) - ref).max() / ref.max()
        print(f"wide2 storage {case} after {what}: model {err:.2e}")
        assert err <= INSIDE, (what, err)
        before = ref
    x, _ = W.updated(case, "x")
    assert (x != c["x"]).sum() == 3 and (x != c["x"]).any(axis=1).sum() == 1


@pytest.mark.parametrize("case", W.REFRESH)
@pytest.mark.parametrize("kind", list(W.BEHIND3))
def test_storage_model_behind_three_layers(case, kind):
    c = W.storage_case(case)
    p = W.behind3_params(case, kind)
    ref = W.behind3_ref(case, kind)
    assert (p["W2"].shape, p["W3"].shape) == ((64, 19), (19, W.BEHIND3[kind][1])) and ref.max() > 0
    assert (W.BEHIND3["narrow"][1] <= 8) and (W.BEHIND3["wide"][1] > 8)
    e64 = np.abs(MV.delta_fp64(c["a_hat"], c["x"], p, c["probes"], c["obs"], W.DELTA) - ref).max() / ref.max()
    err = np.abs(MV.delta_fp64(c["a_hat"], c["x"], p, c["probes"], c["obs"], W.DELTA, **W.model_kw(case)) - ref).max() / ref.max()
    print(f"wide2 storage {case} behind three layers ({kind}): zeros {(ref == 0).mean():.2f} fp64 {e64:.2e} model {err:.2e}")
    assert e64 <= 1e-6 and err <= INSIDE, (e64, err)


# ---- 4. bitmap words, chunk sizes, item counts -----------------------------------------------------------------------------------
def test_big_graph_cells_that_only_a_far_item_serves():
    a_hat, x, probes, obs, zrow = W.big_graph2()
    n = S.BIG_N
    assert a_hat.shape == (n, n) and (n + 31) // 32 == 516 and x.shape == (n, 32) and not x[probes[zrow]].any()
    assert set(S.BIG_SPECIAL) <= set(probes.tolist()) and set(S.BIG_SPECIAL) <= set(obs.tolist()) and len(set(obs.tolist())) < len(obs)
    reach = np.unique(np.concatenate([S.hops(a_hat, int(v), 2) for v in probes]))
    assert np.isin(obs, reach).sum() >= 40 and (~np.isin(obs, reach)).sum() >= 8
    for v, r, first in W.STRETCH_CELLS:
        u, items = W.stretch_cell(a_hat, v, r)
        assert v in probes and u in obs and r >= first and len(items) >= 3
        # items of the probe in every stretch in front of r's: a lost carry of the positions would move r's slot
        assert (items < r).sum() >= 1 and S.stretch_of([r])[0] == first // 8192
        assert np.array_equal(np.intersect1d(a_hat[u].indices, items), [r])


@pytest.mark.parametrize("shape", W.BIG, ids=W.shape_id)
def test_big_graph_scores(shape):
    _, _, probes, obs, zrow = W.big_graph2()
    ref = W.big_ref(shape)
    zeros = float((ref == 0).mean())
    assert ref.max() > 0 and 0.1 <= zeros <= 0.9, (ref.max(), zeros)
    assert np.all(ref[zrow] == 0)
    a_hat = W.big_graph2()[0]
    for v, r, _ in W.STRETCH_CELLS:
        u, _ = W.stretch_cell(a_hat, v, r)
        assert ref[int(np.flatnonzero(probes == v)[0]), int(np.flatnonzero(obs == u)[0])] > 0, (v, r, u)
    # the special ids as probes and as observed nodes: probe 0 is tied to every one of them
    col = [int(np.flatnonzero(obs == s)[0]) for s in S.BIG_SPECIAL]
    assert np.all(ref[0, col] > 0) and all(ref[int(np.flatnonzero(probes == s)[0])].max() > 0 for s in S.BIG_SPECIAL)


@pytest.mark.parametrize("shape", W.ALL_PROBES, ids=W.shape_id)
def test_every_node_as_a_probe_scores(shape):
    _, _, _, obs, _ = W.small_graph("er")
    ref = W.all_probes_ref(shape)
    zeros = float((ref == 0).mean())
    assert ref.shape == (300, len(obs)) and ref.max() > 0 and 0.1 <= zeros <= 0.9, zeros


def test_cap_lists():
    a_hat, x, _, _, zrow = W.small_graph("loops")
    probes, tiled, obs = W.cap_lists()
    assert a_hat.shape[0] == 120 and len(tiled) == W.CAP_PROBES == W.CAP + 3 and len(obs) == 3
    assert np.array_equal(tiled[:28], probes) and np.array_equal(tiled[-17:], probes[:17]) and W.CAP_PROBES == 28 * 2340 + 17
    assert 5 in probes and not x[probes[zrow]].any() and a_hat[5].nnz <= 1
    ref = W.cap_ref()
    assert ref.max() > 0 and (ref == 0).any() and np.all(ref[zrow] == 0)
    assert W.lpr_for(W.round_up4(W.CAP_SHAPE[0])) == 2 and W.CAP_SHAPE[0] % 4 and W.CAP_SHAPE[1] % 4


def test_hub_probes_have_the_item_counts_of_the_tile_edges():
    g = B.hub_ladder()
    a_hat = W.small_graph("hub")[0]
    assert (a_hat != g.a.astype(np.float32)).nnz == 0
    probes, obs = W.hub_lists()
    at = a_hat.T.tocsr()
    assert set(W.HUB_COLUMNS) <= set(B.LADDER) and {1, 63, 64, 65, 128, 129, 513} == set(W.HUB_COLUMNS)
    assert [at[int(v)].nnz for v in probes] == list(W.HUB_COLUMNS)            # the device-side item count of a chunk of one
    assert [a_hat[int(u)].nnz for u in obs[:3]] == [129, 257, 1025]
    sums = np.cumsum(W.HUB_COLUMNS)
    assert sums[-1] == 963 and sums[1] == 64 and sums[2] == 128              # (chunks of two and of all seven: other counts again)
    ref = W.hub_ref()
    assert ref.max() > 0 and np.all(ref.max(axis=1) > 0)                      # every probe has a cell that reads its items
    assert W.HUB_SHAPE == (18, 65) and W.HUB_SHAPE[0] % 4 and W.HUB_SHAPE[1] % 4


def test_er29_rows_have_an_odd_stride():
    a, x, probes, obs, zrow = S.small_graph("er29")
    assert x.shape == (300, 29) and x.strides[0] == 29 * 4 and not x[probes[zrow]].any()
    for shape in W.ER29:
        p = W.er29_params(shape)
        assert p["W1"].shape == (29, shape[0]) and p["W2"].shape == shape

"""Attack metrics on the GPU: lt_score_curve (engine.score_curve) against the shared restatement (tests/curve_restate.py), its
refusals, and Attacker.evaluate against the result file of the attack it replaces.

Exact: D, P, N, auc2, tps, fps, and the thresholds as bit patterns (the zero group +0.0).  AP: a sum of at most D + 1
non-negative float64 terms that total at most 1, each from at most three roundings, so two summation orders differ by at most
2 (D + 4) 2^-53 (curve_restate.ap_bound, from the case's own D).  A second call gives identical bytes.

One class missing: the counts and the integers are still right; ``ScoreCurve.summary()`` reports ``auc`` = NaN (it does not
raise) and ``ap`` = 0.0 without positives."""
import argparse
import math
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, csr_from
from curve_restate import ap_bound, restate

pytestmark = pytest.mark.gpu

# the cuts of linkteller_amd/csrc/lt_metrics.hip
MC_MIN_CHUNK = 512       # items per block per pass
MC_MAX_BLOCKS = 512      # the grid stops growing at MC_MIN_CHUNK * MC_MAX_BLOCKS items; the ranges grow instead
MC_THREADS = 256         # k_mc_scan (per digit) and k_mc_block_scan, both over the blocks: a thread's stretch goes from 1 to 2 at
                         # 256 -> 257 blocks
BLOCK_SCAN_CUT = MC_THREADS * MC_MIN_CHUNK
GRID_CUT = MC_MIN_CHUNK * MC_MAX_BLOCKS
SIZES = ([1, 2, 3, 63, 64, 65, 255, 256, 257]
         + [MC_MIN_CHUNK - 1, MC_MIN_CHUNK, MC_MIN_CHUNK + 1]
         + [3 * MC_MIN_CHUNK + 164]                                  # three blocks and a ragged tail
         + [4 * MC_MIN_CHUNK - 1, 4 * MC_MIN_CHUNK, 4 * MC_MIN_CHUNK + 1]      # four blocks -> five
         + [BLOCK_SCAN_CUT - 1, BLOCK_SCAN_CUT, BLOCK_SCAN_CUT + 1]
         + [GRID_CUT - 1, GRID_CUT, GRID_CUT + 1])
FLT_MAX = np.float32(3.4028235e38)
TINY = np.float32(1.4e-45)                                           # the smallest subnormal


def _pool(rng, n, values):
    values = np.array(values, dtype=np.float32)
    v = rng.choice(values, n)
    k = min(n, values.size)
    v[:k] = values[:k]                                   # (every value is present as soon as n allows)
    return v


def _digit(rng, n, d):
    """keys that differ in digit position d only: byte d of 0x40404040 replaced by a random byte (finite for every byte)"""
    bits = np.full(n, 0x40404040, dtype=np.uint32) & ~np.uint32(0xff << (8 * d))
    return (bits | (rng.randint(0, 256, n).astype(np.uint32) << np.uint32(8 * d))).view(np.float32)


def _values(rng, n):
    out = {"zeros": np.zeros(n, dtype=np.float32),
           "distinct": ((rng.permutation(n).astype(np.float64) - n // 2) * 0.37).astype(np.float32)}
    v = np.zeros(n, dtype=np.float32)
    nz = rng.random_sample(n) < 0.1
    v[nz] = (rng.random_sample(int(nz.sum())) + 0.05).astype(np.float32)
    out["ninety_percent_zeros"] = v
    for d in range(4):
        out[f"digit{d}"] = _digit(rng, n, d)
    out["around_the_sign"] = _pool(rng, n, [TINY, -TINY, 2 * TINY, -2 * TINY, 1e-38, -1e-38])
    out["signed_zeros"] = _pool(rng, n, [0.0, -0.0, 0.5])
    out["subnormals_next_to_zero"] = _pool(rng, n, [-0.0, TINY, 0.0, 2 * TINY, -TINY, 1e-40])
    out["flt_max"] = _pool(rng, n, [FLT_MAX, -FLT_MAX, 0.0, 1.0])
    assert out["distinct"].size == np.unique(out["distinct"]).size
    return out


def _check(gpu, s_items, y, dev_scores, dev_index, tag):
    """one case: two calls against the restatement of the items' own (score, label) list"""
    from linkteller_amd import engine
    r = restate(s_items, y)
    D = r["thresholds"].size
    labels = torch.from_numpy(np.ascontiguousarray(y, dtype=np.uint8)).to(gpu)
    a = engine.score_curve(dev_scores, labels, dev_index)
    b = engine.score_curve(dev_scores, labels, dev_index)
    w = [int(x) for x in a.raw.cpu().tolist()]
    assert w[5:] == [0, 0, 0], tag
    assert (w[0], w[1], w[2], w[3]) == (D, r["P"], r["N"], r["auc2"]), tag
    thr, tps, fps = a.counts()
    assert thr.dtype == np.float32 and tps.dtype == np.int64 and fps.dtype == np.int64
    assert np.array_equal(tps, r["tps"]) and np.array_equal(fps, r["fps"]), tag
    assert np.array_equal(thr.view(np.int32), r["thresholds"].view(np.int32)), tag      # bit patterns; the zero group is +0.0
    s = a.summary()
    assert (s["n_thresholds"], s["n_pos"], s["n_neg"]) == (D, r["P"], r["N"]), tag
    if r["P"] and r["N"]:
        assert s["auc"] == r["auc2"] / (2 * r["P"] * r["N"]), tag
    else:
        assert math.isnan(s["auc"]) and r["auc2"] == 0, tag
    if r["P"] == 0:
        assert s["ap"] == 0.0 and w[4] == 0, tag
    assert abs(s["ap"] - r["ap"]) <= ap_bound(D), (tag, s["ap"], r["ap"])
    # the second call: identical bytes
    assert torch.equal(a.raw, b.raw), tag
    assert torch.equal(a.tps[:D], b.tps[:D]) and torch.equal(a.fps[:D], b.fps[:D]), tag
    assert torch.equal(a.thresholds[:D].view(torch.int32), b.thresholds[:D].view(torch.int32)), tag
    return r


@pytest.mark.parametrize("n", SIZES)
def test_score_curve_against_the_restatement(gpu, n):
    """Every value class with every label set (random, all 0, all 1) at every size."""
    rng = np.random.RandomState(2000 + n % 9973)
    y_random = rng.randint(0, 2, n)
    for name, v in _values(rng, n).items():
        dev = torch.from_numpy(v).to(gpu)
        for lname, y in (("random", y_random), ("all0", np.zeros(n, dtype=np.int64)), ("all1", np.ones(n, dtype=np.int64))):
            r = _check(gpu, v, y, dev, None, f"n={n} values={name} labels={lname}")
        D = r["thresholds"].size
        if name == "zeros":
            assert D == 1
        if name == "distinct":
            assert D == n
        if name == "signed_zeros":
            assert int((r["thresholds"] == 0).sum()) == 1                 # -0.0 and +0.0 form ONE threshold
        if name == "subnormals_next_to_zero" and n >= 6:
            assert {float(t) for t in r["thresholds"]} >= {0.0, float(TINY), float(-TINY)}      # distinct from 0 and from each other


def test_score_curve_through_an_index(gpu):
    from linkteller_amd import engine
    rng = np.random.RandomState(77)
    # a strided n x lds matrix read through the cells of its strict lower triangle: everything else is NaN, which any stray read
    # would report in summary[5]
    n, lds = 67, 80
    buf = np.full((n + 2, lds), np.nan, dtype=np.float32)
    ii, jj = np.tril_indices(n, -1)
    vals = np.zeros(ii.size, dtype=np.float32)
    nz = rng.random_sample(ii.size) < 0.1
    vals[nz] = (rng.random_sample(int(nz.sum())) + 0.05).astype(np.float32)
    buf[ii, jj] = vals
    big = torch.from_numpy(buf).to(gpu)
    view = big[:n, :n]
    assert view.stride(0) == lds and not view.is_contiguous()
    index = torch.from_numpy(ii.astype(np.int64) * lds + jj).to(gpu)
    y = rng.randint(0, 2, ii.size)
    _check(gpu, vals, y, view, index, "lower triangle of a strided matrix")
    with pytest.raises(ValueError):
        engine.score_curve(view, torch.from_numpy(y.astype(np.uint8)).to(gpu)[:n * n])      # no index: contiguous scores only
    # repeated indices: more items than scores
    s = ((rng.permutation(300).astype(np.float64) - 100) * 0.25).astype(np.float32)
    idx = rng.randint(0, s.size, 1500).astype(np.int64)
    _check(gpu, s[idx], rng.randint(0, 2, idx.size), torch.from_numpy(s).to(gpu), torch.from_numpy(idx).to(gpu), "repeated indices")
    # a subset in scrambled order; what is not listed (NaN) is not read
    s = rng.standard_normal(5000).astype(np.float32)
    idx = rng.permutation(s.size)[:1700].astype(np.int64)
    holed = np.full(s.size, np.nan, dtype=np.float32)
    holed[idx] = s[idx]
    _check(gpu, s[idx], rng.randint(0, 2, idx.size), torch.from_numpy(holed).to(gpu), torch.from_numpy(idx).to(gpu), "scrambled subset")


def test_score_curve_order_does_not_show(gpu):
    """the outputs are a function of the multiset of (score, label) pairs: a permutation of the items changes no byte"""
    from linkteller_amd import engine
    rng = np.random.RandomState(5)
    n = 3 * MC_MIN_CHUNK + 164
    v = np.round(rng.standard_normal(n), 1).astype(np.float32)              # many ties
    y = rng.randint(0, 2, n).astype(np.uint8)
    p = rng.permutation(n)
    a = engine.score_curve(torch.from_numpy(v).to(gpu), torch.from_numpy(y).to(gpu))
    b = engine.score_curve(torch.from_numpy(v[p]).to(gpu), torch.from_numpy(y[p]).to(gpu))
    D = a.summary()["n_thresholds"]
    assert torch.equal(a.raw, b.raw)
    assert torch.equal(a.tps[:D], b.tps[:D]) and torch.equal(a.fps[:D], b.fps[:D]) and torch.equal(a.thresholds[:D], b.thresholds[:D])


@pytest.mark.parametrize("what", ["nan", "+inf", "-inf", "index -1", "index n_scores", "label 2"])
def test_score_curve_refusals(gpu, what):
    """each runs once; the kernels replace a bad index by 0 before the load and take a bad label as 1, so nothing is provoked"""
    from linkteller_amd import engine
    rng = np.random.RandomState(9)
    n = 700
    s = rng.standard_normal(n).astype(np.float32)
    y = rng.randint(0, 2, n).astype(np.uint8)
    idx = rng.permutation(n).astype(np.int64)
    exc = ValueError
    if what == "nan":
        s[idx[123]] = np.nan
    elif what == "+inf":
        s[idx[5]] = np.inf
    elif what == "-inf":
        s[idx[699]] = -np.inf
    elif what == "index -1":
        idx[300], exc = -1, IndexError
    elif what == "index n_scores":
        idx[0], exc = n, IndexError
    else:
        y[650] = 2
    c = engine.score_curve(torch.from_numpy(s).to(gpu), torch.from_numpy(y).to(gpu), torch.from_numpy(idx).to(gpu))
    w = c.raw.cpu().numpy()
    assert [int(w[5]), int(w[6]), int(w[7])] == [int(what in ("nan", "+inf", "-inf")), int(what.startswith("index")), int(what == "label 2")]
    with pytest.raises(exc):
        c.summary()
    with pytest.raises(exc):
        c.counts()


def test_score_curve_wrapper_checks(gpu):
    from linkteller_amd import _lib, engine
    s = torch.zeros(8, dtype=torch.float32, device=gpu)
    y = torch.zeros(8, dtype=torch.uint8, device=gpu)
    with pytest.raises(_lib.LinkTellerHipError):
        engine.score_curve(s.cpu(), y)
    with pytest.raises(_lib.LinkTellerHipError):
        engine.score_curve(s, y.cpu())
    with pytest.raises(TypeError):
        engine.score_curve(s.double(), y)
    with pytest.raises(TypeError):
        engine.score_curve(s, y.long())
    with pytest.raises(TypeError):
        engine.score_curve(s, y, torch.zeros(8, dtype=torch.int32, device=gpu))
    with pytest.raises(TypeError):
        engine.score_curve(s, y, torch.zeros(7, dtype=torch.int64, device=gpu))
    with pytest.raises(ValueError):
        engine.score_curve(s[:4], y)
    with pytest.raises(ValueError):
        engine.score_curve(s, y[:0])


# ---- Attacker.evaluate against the attack's own result file ---------------------------------------------------------------------
def _world(gpu, prefix_adj, xkey):
    from linkteller_amd import graph
    g = np.load(os.path.join(GOLDEN, "next_rows.npz"), allow_pickle=False)
    a = csr_from(g, prefix_adj)
    x = torch.from_numpy(g[xkey]).to(gpu)
    adj_t = graph.sparse_mx_to_torch_sparse_tensor(graph.first_order_gcn(a)).to(gpu)
    return g, types.SimpleNamespace(features_2=x, adj_2=adj_t, adj_ori=a, n_nodes=a.shape[0])


def _model(gpu, g, kind):
    from linkteller_amd.gcn import GCN, GCN3
    if kind == "gcn2":
        model = GCN(64, 32, 2, 0.5)
        model.load_state_dict({k: torch.from_numpy(g[f"sd.{k}"]) for k in ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias")})
    else:
        model = GCN3(64, 32, 16, 2, 0.5)
        model.load_state_dict({k: torch.from_numpy(g[f"gcn3.sd.{k}"]) for k in
                               ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias", "gc3.weight", "gc3.bias")})
    return model.to(gpu).eval()


def _against_the_file(atk, attack, filename):
    """run the attack method (it writes `filename`), then evaluate(curves=True): the six arrays equal the file's, the two numbers
    agree within the bound"""
    attack()
    auc, ap = atk.auc, atk.ap
    saved = torch.load(filename, weights_only=False)
    out = atk.evaluate(curves=True)
    c = out["curves"]
    for side, keys in (("auc", ("fpr", "tpr", "thresholds")), ("pr", ("precision", "recall", "thresholds"))):
        for k in keys:
            got, exp = c[side][k], np.asarray(saved[side][k])
            assert got.dtype == exp.dtype == np.float64 and np.array_equal(got, exp), (side, k)
    y = np.asarray(saved["result"]["y"])
    assert out["n_pos"] == int(y.sum()) and out["n_neg"] == int(y.size - y.sum())
    assert out["n_thresholds"] == c["pr"]["thresholds"].size
    bound = ap_bound(out["n_thresholds"])
    assert atk.auc == out["auc"] and atk.ap == out["ap"]
    assert abs(out["auc"] - auc) <= bound and abs(out["ap"] - ap) <= bound, (out["auc"] - auc, out["ap"] - ap, bound)
    assert abs(c["auc_value"] - auc) <= bound and abs(c["ap_value"] - ap) <= bound
    return out


@pytest.mark.parametrize("kind,mode", [("gcn2", "delta"), ("gcn2", "sparse"), ("gcn3", "delta")])
def test_evaluate_efficient_unbalanced(gpu, tmp_path, monkeypatch, capsys, kind, mode):
    from linkteller_amd.attacker import Attacker
    g, w = _world(gpu, "adj", "x")
    monkeypatch.chdir(tmp_path)
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=32, sample_seed=42, influence=1e-4,
                              mode="vanilla-clean", attack_mode="efficient", influence_mode=mode)
    atk = Attacker(args, _model(gpu, g, kind), w)
    atk.prepare_test_data()
    name = os.path.join("eval_twitch/ES/RU", "efficient_unbalanced_32_42.pt")
    capsys.readouterr()
    out = _against_the_file(atk, atk.link_prediction_attack_efficient, name)
    printed = capsys.readouterr().out
    assert printed.count("auc = ") == 2 and printed.count("ap = ") == 2 and f"auc = {out['auc']}" in printed
    files = sorted(os.listdir("eval_twitch/ES/RU"))
    assert files == ["efficient_unbalanced_32_42.pt"]                     # evaluate wrote nothing
    # the index is built once per sample ...
    first = atk._metric_cache[4]
    assert atk.evaluate()["auc"] == out["auc"] and atk._metric_cache[4] is first
    # ... and a new prepare_test_data() replaces it
    os.remove(name)
    args.sample_seed = 43
    atk.prepare_test_data()
    name2 = os.path.join("eval_twitch/ES/RU", "efficient_unbalanced_32_43.pt")
    _against_the_file(atk, atk.link_prediction_attack_efficient, name2)
    assert atk._metric_cache[4] is not first and atk._metric_cache[0] is atk.exist_edges


def test_evaluate_naive(gpu, tmp_path, monkeypatch):
    from linkteller_amd.attacker import Attacker
    g, w = _world(gpu, "adj", "x")
    monkeypatch.chdir(tmp_path)
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="unbalanced", n_test=32, sample_seed=42, influence=1e-4,
                              mode="vanilla-clean", attack_mode="naive")
    for kind in ("gcn2", "gcn3"):          # lt_influence_pairs' device tensor / pair_scores' host result, uploaded
        atk = Attacker(args, _model(gpu, g, kind), w)
        atk.prepare_test_data()
        _against_the_file(atk, atk.link_prediction_attack, atk.naive_result_filename())
        os.remove(atk.naive_result_filename())


def test_evaluate_balanced_full(gpu, tmp_path, monkeypatch):
    from linkteller_amd.attacker import Attacker
    g, w = _world(gpu, "bf.adj", "bf.x")
    monkeypatch.chdir(tmp_path)
    args = argparse.Namespace(dataset="twitch/ES/RU", sample_type="balanced-full", n_test=7, sample_seed=82, influence=1e-4,
                              mode="vanilla-clean", attack_mode="efficient")
    atk = Attacker(args, _model(gpu, g, "gcn2"), w)
    atk.prepare_test_data()
    _against_the_file(atk, atk.link_prediction_attack_efficient_balanced, atk.result_filename())
    args.attack_mode = "baseline"
    with pytest.raises(NotImplementedError):
        atk.evaluate()


def test_cli_metrics_only_end_to_end(gpu, tmp_path, monkeypatch, capsys):
    import re
    from test_cli_worker_dp import _write_musae
    from linkteller_amd import main as lt_main, synth
    from linkteller_amd.gcn import GCN
    a1, a2 = synth.powerlaw_graph(260, 1200, seed=1), synth.powerlaw_graph(320, 1500, seed=2)
    _write_musae(str(tmp_path), "ES", a1, 400, 1)
    _write_musae(str(tmp_path), "RU", a2, 400, 2)
    torch.manual_seed(0)
    torch.save(GCN(3170, 256, 2, 0.5).state_dict(), tmp_path / "model.pt")
    monkeypatch.chdir(tmp_path)
    base = (f"--mode vanilla-clean --dataset twitch/ES/RU --hidden 256 --norm FirstOrderGCN --test --model-path {tmp_path}/model.pt "
            f"--attack --attack-mode efficient --sample-type unbalanced --n-test 60 --data-root {tmp_path}").split()
    lt_main.main(base + ["--metrics-only"])
    out = capsys.readouterr().out
    assert "attack results saved" not in out and not os.path.exists("eval_twitch")
    got = [float(re.search(rf"^{k} = (\S+)$", out, flags=re.M).group(1)) for k in ("auc", "ap")]
    lt_main.main(base)
    out = capsys.readouterr().out
    assert "attack results saved to: eval_twitch/ES/RU/efficient_unbalanced_60_42.pt" in out
    ref = [float(re.search(rf"^{k} = (\S+)$", out, flags=re.M).group(1)) for k in ("auc", "ap")]
    bound = ap_bound(60 * 59 // 2)
    assert abs(got[0] - ref[0]) <= bound and abs(got[1] - ref[1]) <= bound

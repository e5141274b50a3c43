"""Attack metrics without a GPU: the shared restatement (tests/curve_restate.py) and linkteller_amd/metrics.py against sklearn,
the argument checks of lt_score_curve that happen before any device call, and the command line's --metrics-only.

AP and the trapezoid AUC are sums of at most D + 1 non-negative float64 terms that total at most 1, each from at most three
roundings, so two summation orders differ by at most 2 (D + 4) 2^-53 (curve_restate.ap_bound); every array and every integer
is compared exactly."""
import os

import numpy as np
import pytest

from curve_restate import ap_bound, restate


@pytest.fixture(scope="module")
def lt():
    from linkteller_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _labels(rng, n_pos, n_neg):
    return rng.permutation(np.r_[np.ones(n_pos, dtype=np.int64), np.zeros(n_neg, dtype=np.int64)])


def _cases():
    """Every case has P and N powers of two.  roc_auc_score is sklearn's float64 trapezoid over fpr = fps / N and tpr = tps / P:
    with dyadic P and N every quotient, product and partial sum of it is exact, so it IS the Mann-Whitney value and `==` against
    auc2 / (2 P N) is provable.  With other class counts the trapezoid carries its own rounding: 201 positives / 199 negatives
    drawn from {0.0, -0.0, 0.5, -0.5} gave auc2 / (2 P N) - roc_auc_score = -5.55e-17, one ulp of sklearn's sum, not of the
    integer quotient."""
    rng = np.random.RandomState(5)
    out = {}
    n = 512 + 4096
    v = np.zeros(n, dtype=np.float32)
    nz = rng.permutation(n)[:n // 10]
    v[nz] = np.unique(rng.random_sample(4 * n).astype(np.float32) + 0.01)[:nz.size]
    out["ninety_percent_zeros"] = (v, _labels(rng, 512, 4096))
    n = 1024 + 2048
    out["all_distinct"] = (rng.permutation(np.unique(rng.standard_normal(3 * n).astype(np.float32))[:n]), _labels(rng, 1024, 2048))
    out["one_value"] = (np.full(48, 0.25, dtype=np.float32), _labels(rng, 16, 32))
    out["negatives"] = (-np.abs(rng.standard_normal(320)).astype(np.float32).round(1), _labels(rng, 64, 256))
    out["signed_zeros"] = (rng.choice(np.array([0.0, -0.0, 0.5, -0.5], dtype=np.float32), 384), _labels(rng, 128, 256))
    out["subnormals"] = (rng.choice(np.array([0.0, -0.0, 1.4e-45, 2.8e-45, -1.4e-45, 1e-40, 1.1754942e-38, 1.17549435e-38],
                                             dtype=np.float32), 576), _labels(rng, 64, 512))
    # runs of one label at distinct scores: collinear ROC points that drop_intermediate drops
    y = np.repeat(np.array([1, 0, 1, 0, 0, 1], dtype=np.int64), [8, 8, 4, 16, 8, 4])
    out["collinear_runs"] = (np.arange(y.size, 0, -1).astype(np.float32), y)
    out["two_items"] = (np.array([0.0, 1.0], dtype=np.float32), np.array([0, 1]))
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_and_curves_against_sklearn(name):
    from sklearn import metrics as skm
    from linkteller_amd import metrics
    s, y = CASES[name]
    assert s.dtype == np.float32
    r = restate(s, y)
    D = r["thresholds"].size
    assert r["thresholds"].dtype == np.float32 and r["tps"].dtype == np.int64 and r["fps"].dtype == np.int64
    assert not np.signbit(r["thresholds"][r["thresholds"] == 0]).any()          # the zero group reports +0.0
    assert r["P"] == int(y.sum()) and r["N"] == int(y.size - y.sum())
    s64 = s.astype(np.float64)                                                 # the reference's score list is float64
    # the restatement's counts are sklearn's
    fpr_all, tpr_all, thr_all = skm.roc_curve(y, s64, drop_intermediate=False)
    assert np.array_equal(thr_all[1:], r["thresholds"].astype(np.float64))
    assert np.array_equal(fpr_all[1:], r["fps"] / r["fps"][-1]) and np.array_equal(tpr_all[1:], r["tps"] / r["tps"][-1])
    for c_ in (r["P"], r["N"]):
        assert c_ & (c_ - 1) == 0                   # (see _cases)
    print(name, "auc2 / (2 P N) - roc_auc_score =", r["auc2"] / (2 * r["P"] * r["N"]) - skm.roc_auc_score(y, s64))
    assert r["auc2"] / (2 * r["P"] * r["N"]) == skm.roc_auc_score(y, s64)
    assert abs(r["ap"] - skm.average_precision_score(y, s64)) <= ap_bound(D)
    # the module's curves are sklearn's defaults, bit for bit
    c = metrics.curves_from_counts(r["thresholds"], r["tps"], r["fps"])
    fpr, tpr, thr = skm.roc_curve(y, s64)
    precision, recall, thr2 = skm.precision_recall_curve(y, s64)
    for got, exp in ((c["auc"]["fpr"], fpr), (c["auc"]["tpr"], tpr), (c["auc"]["thresholds"], thr),
                     (c["pr"]["precision"], precision), (c["pr"]["recall"], recall), (c["pr"]["thresholds"], thr2)):
        assert got.dtype == exp.dtype == np.float64 and np.array_equal(got, exp)
    assert c["auc_value"] == skm.auc(fpr, tpr)
    assert abs(c["auc_value"] - r["auc2"] / (2 * r["P"] * r["N"])) <= ap_bound(D)
    assert abs(c["ap_value"] - skm.average_precision_score(y, s64)) <= ap_bound(D)
    assert abs(c["ap_value"] - r["ap"]) <= ap_bound(D)
    if name == "collinear_runs":
        assert fpr.size < fpr_all.size, "drop_intermediate dropped nothing: the case does not test it"
    if name in ("signed_zeros", "subnormals"):
        assert int((r["thresholds"] == 0).sum()) == 1
    if name == "subnormals":
        assert D == 7                              # +-0 is one threshold, every subnormal its own


def test_one_class_missing_raises():
    from linkteller_amd import metrics
    s = np.array([0.5, 0.25, 0.0], dtype=np.float32)
    for y in (np.ones(3, dtype=np.int64), np.zeros(3, dtype=np.int64)):
        r = restate(s, y)
        with pytest.raises(ValueError, match="one class"):
            metrics.curves_from_counts(r["thresholds"], r["tps"], r["fps"])
    with pytest.raises(ValueError):
        metrics.curves_from_counts(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))


def test_metrics_module_needs_no_gpu_import():
    import subprocess
    import sys
    from conftest import REPO
    code = ("import sys; import linkteller_amd.metrics; "
            "assert 'torch' not in sys.modules and 'sklearn' not in sys.modules and 'linkteller_amd.engine' not in sys.modules")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1000:]


def test_score_curve_argument_errors(lt):
    h = lt.lib()
    q = h.lt_score_curve_workspace_bytes
    assert q(1) > 0 and q(124750) >= 10 * 124750 and q(1999000) > q(124750) and q(2 ** 31 - 1) > 10 * (2 ** 31 - 1)
    assert q(0) == 0 and q(-1) == 0 and q(2 ** 31) == 0
    # host memory stands in for the device pointers: every check below returns before anything is enqueued or dereferenced
    buf = np.zeros(1 << 16, dtype=np.int64)
    p = buf.ctypes.data
    need = q(100)

    def call(scores=p, n_scores=100, index=p, labels=p, n_items=100, thr=p, tps=p, fps=p, summary=p, ws=p, ws_bytes=buf.nbytes):
        return h.lt_score_curve(scores, n_scores, index, labels, n_items, thr, tps, fps, summary, ws, ws_bytes, None)

    for kw in (dict(scores=None), dict(labels=None), dict(thr=None), dict(tps=None), dict(fps=None), dict(summary=None), dict(ws=None)):
        assert call(**kw) == -1 and b"NULL" in h.lt_last_error(), kw
    assert call(n_items=0) == -1 and b"n_items" in h.lt_last_error()
    assert call(n_items=-1) == -1 and b"n_items" in h.lt_last_error()
    assert call(n_scores=0) == -1 and b"n_scores" in h.lt_last_error()
    assert call(n_scores=-5) == -1
    assert call(index=None, n_scores=99) == -1 and b"without an index" in h.lt_last_error()
    assert call(ws_bytes=need - 1) == -1 and b"workspace" in h.lt_last_error()
    assert call(ws=p + 4) == -1 and b"aligned" in h.lt_last_error()
    assert call(ws_bytes=0) == -1


def test_cli_metrics_only_flag():
    from linkteller_amd import main as lt_main
    assert lt_main.get_arguments([]).metrics_only is False
    a = lt_main.get_arguments("--attack --attack-mode efficient --sample-type unbalanced --metrics-only".split())
    assert a.metrics_only is True
    lt_main.check_metrics_only(a)                                   # the served combinations pass
    lt_main.check_metrics_only(lt_main.get_arguments("--attack --attack-mode naive --metrics-only".split()))
    lt_main.check_metrics_only(lt_main.get_arguments("--attack --attack-mode baseline".split()))       # off: nothing to refuse


@pytest.mark.parametrize("argv", [
    "--test --attack --metrics-only --attack-mode baseline --sample-type unbalanced",
    "--test --attack --metrics-only --attack-mode baseline-feat --sample-type balanced-full",
])
def test_cli_metrics_only_refused_before_a_worker_is_built(argv, monkeypatch):
    from linkteller_amd import main as lt_main, worker

    def boom(*a, **k):
        raise AssertionError("a Worker was built")
    monkeypatch.setattr(worker, "Worker", boom)
    monkeypatch.setattr(lt_main, "init_distributed", boom)
    with pytest.raises(NotImplementedError, match="--metrics-only"):
        lt_main.main(argv.split())


def test_evaluate_refuses_the_baseline_attacks():
    import argparse
    import types
    import scipy.sparse as sp
    import torch
    from linkteller_amd.attacker import Attacker
    w = types.SimpleNamespace(features_2=torch.zeros(4, 3), adj_2=None, adj_ori=sp.identity(4, format="csr"), n_nodes=4)
    for am in ("baseline", "baseline-feat"):
        args = argparse.Namespace(dataset="twitch/x", sample_type="unbalanced", n_test=4, attack_mode=am)
        with pytest.raises(NotImplementedError, match="evaluate"):
            Attacker(args, None, w).evaluate()

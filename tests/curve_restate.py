"""The plain restatement of lt_score_curve shared by tests/test_metrics_cpu.py and tests/test_metrics_gpu.py (numpy only)."""
import numpy as np


def restate(scores, labels):
    """``scores``: float32 [n], ``labels``: 0 / 1 [n] -> dict with ``thresholds`` (float32 [D], descending, the zero group as
    +0.0), ``tps`` / ``fps`` (int64 [D]), ``P``, ``N``, ``auc2`` (Python int), ``ap`` (float)."""
    s = np.asarray(scores, dtype=np.float32).reshape(-1) + np.float32(0.0)      # -0.0 -> +0.0; subnormals stay
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    order = np.argsort(-s, kind="stable")
    s, y = s[order], y[order]
    ends = np.r_[np.nonzero(s[1:] != s[:-1])[0], s.size - 1]      # np.diff(s) != 0 without the overflow at +-FLT_MAX
    tps = np.cumsum(y)[ends]
    fps = 1 + ends - tps
    P, N = int(tps[-1]), int(fps[-1])
    pos = np.diff(np.r_[0, tps])
    neg = np.diff(np.r_[0, fps])
    prev = np.r_[0, tps[:-1]]
    auc2 = sum(int(n_) * (2 * int(t_) + int(p_)) for n_, t_, p_ in zip(neg, prev, pos))
    ap = float(np.sum((pos / P) * (tps / (tps + fps)))) if P else 0.0
    return {"thresholds": s[ends], "tps": tps.astype(np.int64), "fps": fps.astype(np.int64), "P": P, "N": N, "auc2": auc2, "ap": ap}


def ap_bound(D):
    """|AP_a - AP_b| for two summation orders of the same at most D + 1 non-negative float64 terms that total at most 1, each from
    at most three roundings."""
    return 2 * (D + 4) * 2.0 ** -53

"""The curves of the attack's result file from the counts table of ``lt_score_curve`` (host only, plain numpy, O(D)).

``engine.score_curve`` leaves, for the D distinct scores in descending order, ``tps[d]`` / ``fps[d]`` = the positives / negatives
scoring at least ``thresholds[d]`` -- what sklearn's ``_binary_clf_curve`` returns.  Everything ``Attacker.compute_and_save``
stores under "auc" and "pr" (reference attacker.py:378-389: ``metrics.roc_curve`` and ``metrics.precision_recall_curve`` with
their defaults) follows from those three arrays by the arithmetic below, which repeats sklearn's operation by operation so that
the arrays come out equal bit for bit (checked against sklearn 1.7 in tests/test_metrics_cpu.py)."""
from __future__ import annotations

import numpy as np

_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def curves_from_counts(thresholds, tps, fps) -> dict:
    """``{"auc": {"fpr", "tpr", "thresholds"}, "pr": {"precision", "recall", "thresholds"}, "auc_value", "ap_value"}``.

    ROC side (``roc_curve(..., drop_intermediate=True)``): interior points collinear with their neighbours are dropped, the
    ``(0, 0, inf)`` point is prepended.  PR side (``precision_recall_curve``): every threshold kept, the arrays reversed so that
    recall decreases, ending in precision 1 / recall 0.  Thresholds are widened to float64, the dtype of the reference's score
    list.  ``auc_value`` is ``metrics.auc(fpr, tpr)`` (the trapezoid rule), ``ap_value`` is ``average_precision_score``.
    Raises ``ValueError`` when one class is missing (sklearn warns and returns NaNs there)."""
    thr = np.asarray(thresholds).astype(np.float64).reshape(-1)
    tps = np.asarray(tps).astype(np.float64).reshape(-1)       # (sklearn's counts are float64: cumsum of y_true * 1.0)
    fps = np.asarray(fps).astype(np.float64).reshape(-1)
    if not (thr.size == tps.size == fps.size) or thr.size == 0:
        raise ValueError(f"thresholds, tps and fps must be equally long and not empty (got {thr.size}, {tps.size}, {fps.size})")
    if tps[-1] <= 0 or fps[-1] <= 0:
        raise ValueError(f"only one class present ({int(tps[-1])} positives, {int(fps[-1])} negatives): the curves are not defined")

    # ---- roc_curve
    r_fps, r_tps, r_thr = fps, tps, thr
    if len(fps) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        r_fps, r_tps, r_thr = fps[keep], tps[keep], thr[keep]
    r_tps = np.r_[0, r_tps]
    r_fps = np.r_[0, r_fps]
    r_thr = np.r_[np.inf, r_thr]
    fpr = r_fps / r_fps[-1]
    tpr = r_tps / r_tps[-1]
    auc_value = float(_trapezoid(tpr, fpr))                     # (fpr is non-decreasing: metrics.auc's direction is +1)

    # ---- precision_recall_curve
    ps = tps + fps
    precision = np.zeros_like(tps)
    np.divide(tps, ps, out=precision, where=(ps != 0))
    recall = tps / tps[-1]
    precision = np.hstack((precision[::-1], 1))
    recall = np.hstack((recall[::-1], 0))
    ap_value = float(max(0.0, -np.sum(np.diff(recall) * np.array(precision)[:-1])))

    return {"auc": {"fpr": fpr, "tpr": tpr, "thresholds": r_thr},
            "pr": {"precision": precision, "recall": recall, "thresholds": thr[::-1]},
            "auc_value": auc_value, "ap_value": ap_value}


def rare_class_f1(output, labels, bare_zero=True):
    """F1 / precision / recall / AP of the minority class of a two-class problem (reference gcn_trainer.py:262-284,
    mlp_trainer.py:181-202): ``output`` [n, 2] logits, ``labels`` [n] of 0 / 1.  The rare class is 1 unless there are more
    ones than zeros; AP scores the confidence of the predicted class against "is the rare class", as the reference does.
    When no row is predicted as the rare class the reference returns a bare 0: so does ``bare_zero=True``; otherwise
    (0.0, 0.0, 0.0, AP).  When rows are predicted rare and none of them is (precision = recall = 0, where the reference
    divides by zero) F1 is 0.0."""
    import torch
    import torch.nn.functional as F
    from sklearn.metrics import average_precision_score
    ind = [torch.where(labels == 0)[0], torch.where(labels == 1)[0]]
    rare = int(len(ind[0]) > len(ind[1]))
    conf, pred = F.softmax(output, dim=1).max(1)
    ap = average_precision_score(labels.cpu() if rare == 1 else 1 - labels.cpu(), conf.detach().cpu())
    pred = pred.type_as(labels)
    tp = torch.sum(pred[ind[rare]] == rare).item()
    t, p = len(ind[rare]), torch.sum(pred == rare).item()
    if p == 0:
        return 0 if bare_zero else (0.0, 0.0, 0.0, ap)
    precision, recall = tp / p, tp / t
    if tp == 0:
        return 0.0, precision, recall, ap
    return 2 * precision * recall / (precision + recall), precision, recall, ap

"""Edge recovery under a density belief -- the host arithmetic of the reference's post-processing script
(attack_stats_all.py:44-116): the ladder of beliefs around the sampled subgraph's density, the number of pairs each belief
predicts as edges, and precision / recall / F1 of a ranked prediction.  Pure numpy: nothing here touches the GPU; the ranking
itself is ``engine.top_pairs_lower`` (``Attacker.recover_edges``).
"""
from __future__ import annotations

import math

import numpy as np


def _one_digit(value: float):
    """(digit, exponent) with value ~ digit / 10**exponent, one significant digit, a half rounding UP -- the float steps of the
    reference's ``get_closest`` (attack_stats_all.py:56-65): scale by 10 until >= 1, truncate, add one when the rest is >= 0.5.
    The digit can come out as 10 (0.95 -> 10 / 10**1 = 1.0) and a value >= 1 is only truncated / rounded to an integer."""
    exponent = 0
    while value < 1:
        value *= 10
        exponent += 1
    digit = int(value)
    if value - digit >= 0.5:
        digit += 1
    return digit, exponent


def density_ladder(n_edges: int, n_nodes: int):
    """``[r/4, r/2, r, 2r, 4r]`` for r = the density n_edges / (n_nodes (n_nodes - 1) / 2) rounded to one significant digit
    (attack_stats_all.py:44-89).  ``n_edges == 0`` raises: the reference's rounding loop never ends there."""
    n_edges, n_nodes = int(n_edges), int(n_nodes)
    if n_nodes < 2:
        raise ValueError(f"n_nodes={n_nodes}: no node pairs")
    if n_edges <= 0:
        raise ValueError("n_edges == 0: the density has no significant digit (the reference loops forever here); "
                         "give the beliefs explicitly")
    n_total = (n_nodes - 1) * n_nodes // 2
    digit, exponent = _one_digit(n_edges / n_total)
    r = digit / 10 ** exponent
    return [r / 4, r / 2, r, r * 2, r * 4]


def belief_counts(beliefs, n_total: int) -> np.ndarray:
    """``ceil(belief * n_total)`` (attack_stats_all.py:109) clipped to [1, n_total], int64."""
    n_total = int(n_total)
    if n_total < 1:
        raise ValueError(f"n_total={n_total}: no node pairs")
    out = np.empty(len(beliefs), dtype=np.int64)
    for k, b in enumerate(beliefs):
        out[k] = min(max(math.ceil(float(b) * n_total), 1), n_total)
    return out


def recovery_stats(ranked_is_edge, n_edges: int, counts) -> dict:
    """For every count m: tp = the edges among the first m entries of the ranked 0/1 label list, precision = tp / m, recall =
    tp / n_edges, f1 = their harmonic mean, 0 when either is 0 (attack_stats_all.py:76-78, 111-116).  ``n_edges == 0`` gives
    recall 0 (the reference divides 0 by 0 there)."""
    labels = np.asarray(ranked_is_edge).astype(np.int64).reshape(-1)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if counts.size and (int(counts.min()) < 1 or int(counts.max()) > labels.size):
        raise ValueError(f"counts outside [1, {labels.size}]")
    run = np.concatenate([[0], np.cumsum(labels)])
    tp = run[counts]
    precision = tp / counts
    recall = tp / n_edges if n_edges > 0 else np.zeros(len(counts))
    f1 = np.zeros(len(counts))
    ok = (precision > 0) & (recall > 0)
    f1[ok] = 2 * precision[ok] * recall[ok] / (precision[ok] + recall[ok])
    return {"tp": tp.astype(np.int64), "precision": precision.astype(np.float64), "recall": np.asarray(recall, dtype=np.float64),
            "f1": f1}

"""numpy / scipy restatement of one epoch of the 2-layer trainers with a list of training rows set
(lt_gcn*_trainer_set_train_rows, include/linkteller_hip.h): the whole graph is forwarded, the loss head sees the listed rows
only.  Written on top of train_restate (mask, near-kink and fragile-row helpers) and train_wide_restate (head_reference, which
serves the narrow head's cross-entropy too: the same formula), for fp64 and fp32; the reference of test_train_rows_gpu.py, and
the builder of its cases."""
import numpy as np
import scipy.sparse as sp

import train_cases as K
import train_restate as T
import train_wide_cases as KW
import train_wide_restate as TW

NAMES = TW.NAMES
N, F, H = 600, 40, 32          # every case: n <= 600, F <= 40, hidden <= 32
P = 0.5


def epoch_reference_rows(adj, x, y, params, keep, scale, loss, rows, dtype=np.float64, relu_on=None):
    """One epoch up to the gradients with the loss over ``rows`` (distinct ids, any order), in ``dtype``:
        Z1 = A (X W1) + b1; H1d = keep * scale * relu(Z1); Z2 = A (H1d W2) + b2
        (loss, dZ2[rows], counts) = head(Z2[rows], y[rows]) with the divisor m = len(rows); dZ2 = 0 on every other row
        dS2 = A^T dZ2; dW2 = H1d^T dS2; db2 = sum_r dZ2; dZ1 = relu_on * keep * scale * (dS2 W2^T); db1 = sum_r dZ1
        dW1 = X^T (A^T dZ1)
    ``relu_on`` as in train_wide_restate.epoch_reference_wide.  Returns Z1, H1d, Z2, loss, counts ([C, 3] over the listed
    rows), correct (ce: listed rows whose first argmax is the label), dZ2 and the four gradients."""
    a = adj.tocsr().astype(dtype)
    at = a.T.tocsr()
    x = np.asarray(x).astype(dtype)
    w1, b1, w2, b2 = (np.asarray(p).astype(dtype) for p in params)
    rows = np.asarray(rows, dtype=np.int64)
    z1 = a @ (x @ w1) + b1
    drop = np.asarray(keep).astype(dtype) * dtype(scale)
    h1d = np.maximum(z1, dtype(0)) * drop
    z2 = a @ (h1d @ w2) + b2
    val, dz_rows, counts = TW.head_reference(z2[rows], np.asarray(y)[rows], loss, dtype, divisor_rows=len(rows))
    dz2 = np.zeros_like(z2)
    dz2[rows] = dz_rows
    ds2 = at @ dz2
    on = (z1 > 0) if relu_on is None else np.asarray(relu_on, dtype=bool)
    dz1 = (ds2 @ w2.T) * drop * on.astype(dtype)
    correct = int((z2[rows].argmax(axis=1) == np.asarray(y)[rows].reshape(-1)).sum()) if loss == "ce" else None
    return dict(Z1=z1, H1d=h1d, Z2=z2, loss=val, counts=counts, correct=correct, dZ2=dz2, dW1=x.T @ (at @ dz1),
                db1=dz1.sum(axis=0), dW2=h1d.T @ ds2, db2=dz2.sum(axis=0))


def fragile(z2_rows, loss):
    """Listed rows (ce) or listed elements (bce) whose prediction may differ between two roundings (the existing helpers)."""
    return T.fragile_rows(z2_rows) if loss == "ce" else TW.bce_small_logits(z2_rows)


def row_list(n, m, seed):
    """m distinct ids of [0, n) in shuffled order; row n - 1 and then row 0 sit in the middle of the list (m = 1: row 0 alone)."""
    if m == 1:
        return np.array([0], dtype=np.int64)
    inner = np.random.RandomState(1000 + seed).permutation(np.arange(1, n - 1))[:m - 2]
    rows = np.insert(inner, len(inner) // 2, [n - 1, 0]).astype(np.int64)
    assert len(rows) == m == len(np.unique(rows)) and not np.array_equal(rows, np.sort(rows))
    return rows


def hub_graph(n, seed):
    """A symmetric graph whose row 0 has more than 128 entries (a hub: the segmented rows of the layer kernels), normalised."""
    from linkteller_amd import graph, synth
    a = synth.erdos_renyi_graph(n, 5 * n, seed=seed).tolil()
    nb = np.random.RandomState(seed + 3).permutation(np.arange(1, n))[:200]
    a[0, nb] = 1
    a[nb, 0] = 1
    return graph.first_order_gcn(sp.csr_matrix(a))


def make(c, loss, graph_kind="er", seed=0):
    """One case at (N, F, H) with C = ``c`` classes: dict(adj, x, y, params, p, n, F, H, C, loss).  ``graph_kind``: "er"
    (symmetric, normalised), "directed" (train_cases.directed_graph) or "hub" (hub_graph).  bce cases draw b2 as
    train_wide_cases does, so that no logit sits at the sign threshold."""
    from linkteller_amd import graph, synth
    if graph_kind == "directed":
        adj = K.directed_graph(N, seed)
    elif graph_kind == "hub":
        adj = hub_graph(N, seed)
    else:
        adj = graph.first_order_gcn(synth.erdos_renyi_graph(N, 5 * N, seed=seed))
    x = synth.gaussian_features(N, F, seed=seed)
    return dict(adj=K._f32(adj), x=x, y=KW.labels_for(N, c, loss, seed), params=KW.init_params(F, H, c, loss, seed), p=P, n=N, F=F,
                H=H, C=c, loss=loss, graph=graph_kind)


def analyse(case, params, epoch, rows):
    """r64 / r32 at ``params`` with that epoch's mask, tau and the near-kink elements, the fragile listed rows / elements."""
    keep = T.dropout_keep(case["n"], case["H"], epoch, K.SEED, case["p"])
    scale = T.dropout_scale(case["p"])
    args = (case["adj"], case["x"], case["y"], params, keep, scale, case["loss"], rows)
    r64 = epoch_reference_rows(*args, np.float64)
    r32 = epoch_reference_rows(*args, np.float32)
    tau, near = T.near_kink(r64["Z1"], r32["Z1"], keep)
    return dict(r64=r64, r32=r32, keep=keep, args=args, tau=tau, near=near, fragile=fragile(r64["Z2"][rows], case["loss"]))

"""numpy / scipy restatement of one epoch of the 2-layer trainer with the wide head (lt_gcn2_trainer_create_wide,
include/linkteller_hip.h; lt_train_wide.hip.h), without autograd, for both losses; the reference of test_train_wide_gpu.py.
The Philox mask, the Adam step and the near-kink helper are train_restate's.  test_train_wide_cpu.py checks this file against
torch's fp64 autograd."""
import numpy as np

NAMES = ("dW1", "db1", "dW2", "db2")


def head_reference(z, y, loss, dtype=np.float64, divisor_rows=None):
    """The loss head on logits ``z`` [m, C] in ``dtype``: (loss as a Python float, dZ [m, C], counts int64 [C, 3] = (tp, fp, fn)).
    ``loss="ce"``: ``y`` int [m]; loss = mean_r (logsumexp(z_r) - z[r, y_r]), dZ = (softmax - onehot) / m, prediction = first
    argmax.  ``loss="bce"``: ``y`` 0 / 1 [m, C]; per element max(z, 0) - z y + log1p(exp(-|z|)), loss = their sum / (m C),
    dZ = (sigmoid(z) - y) / (m C) with the sigmoid formed through exp(-|z|), predicted positive iff z > 0."""
    z = np.asarray(z).astype(dtype)
    m, c = z.shape
    rows_div = m if divisor_rows is None else divisor_rows
    counts = np.zeros((c, 3), np.int64)
    if loss == "ce":
        y = np.asarray(y).astype(np.int64).reshape(-1)
        r = np.arange(m)
        mx = z.max(axis=1, keepdims=True)
        e = np.exp(z - mx)
        s = e.sum(axis=1, keepdims=True)
        val = ((mx[:, 0] + np.log(s[:, 0])) - z[r, y]).sum(dtype=dtype) / dtype(rows_div)
        dz = e / s
        dz[r, y] -= dtype(1)
        dz = dz / dtype(rows_div)
        arg = z.argmax(axis=1)
        hit = arg == y
        np.add.at(counts[:, 0], y[hit], 1)
        np.add.at(counts[:, 1], arg[~hit], 1)
        np.add.at(counts[:, 2], y[~hit], 1)
        return float(val), dz, counts
    if loss != "bce":
        raise ValueError(loss)
    yb = np.asarray(y).astype(bool)
    yf = yb.astype(dtype)
    t = np.exp(-np.abs(z))
    val = ((np.maximum(z, dtype(0)) - z * yf) + np.log1p(t)).sum(dtype=dtype) / dtype(rows_div * c)
    sig = np.where(z >= 0, dtype(1) / (dtype(1) + t), t / (dtype(1) + t))
    dz = (sig - yf) / dtype(rows_div * c)
    pred = z > 0
    counts[:, 0] = (pred & yb).sum(axis=0)
    counts[:, 1] = (pred & ~yb).sum(axis=0)
    counts[:, 2] = (~pred & yb).sum(axis=0)
    return float(val), dz, counts


def epoch_reference_wide(adj, x, y, params, keep, scale, loss, dtype=np.float64, relu_on=None):
    """One epoch of the wide route's contract up to the gradients, in ``dtype``:
        Z1 = A (X W1) + b1; H1d = keep * scale * relu(Z1); Z2 = A (H1d W2) + b2; (loss, dZ2, counts) = head(Z2, y)
        dS2 = A^T dZ2; dW2 = H1d^T dS2; db2 = sum_r dZ2; dZ1 = relu_on * keep * scale * (dS2 W2^T); db1 = sum_r dZ1
        dW1 = X^T (A^T dZ1)
    ``relu_on`` (bool [n, H]) substitutes the ReLU's derivative pattern (None: Z1 > 0 in ``dtype``); the forward values do not
    depend on it.  Returns a dict: Z1, H1d, Z2, loss, counts, dZ2 and the four gradients."""
    a = adj.tocsr().astype(dtype)
    at = a.T.tocsr()
    x = np.asarray(x).astype(dtype)
    w1, b1, w2, b2 = (np.asarray(p).astype(dtype) for p in params)
    z1 = a @ (x @ w1) + b1
    drop = np.asarray(keep).astype(dtype) * dtype(scale)
    h1d = np.maximum(z1, dtype(0)) * drop
    z2 = a @ (h1d @ w2) + b2
    val, dz2, counts = head_reference(z2, y, loss, dtype)
    ds2 = at @ dz2
    on = (z1 > 0) if relu_on is None else np.asarray(relu_on, dtype=bool)
    dz1 = (ds2 @ w2.T) * drop * on.astype(dtype)
    return dict(Z1=z1, H1d=h1d, Z2=z2, loss=val, counts=counts, dZ2=dz2, dW1=x.T @ (at @ dz1), db1=dz1.sum(axis=0),
                dW2=h1d.T @ ds2, db2=dz2.sum(axis=0))


def ce_margin_rows(z2, tiny=1e-4):
    """Rows whose top-2 logit margin is below ``tiny`` (none for a single class)."""
    if z2.shape[1] < 2:
        return 0
    top = np.sort(z2, axis=1)
    return int(((top[:, -1] - top[:, -2]) < tiny).sum())


def bce_small_logits(z2, tiny=1e-4):
    """Elements whose logit magnitude is below ``tiny``: their predicted sign may differ between two roundings."""
    return int((np.abs(z2) < tiny).sum())


def f1_reference(counts):
    """(micro, macro, weighted) F1 from [C, 3] counts, spelled out class by class in Python integers and floats."""
    f1s, sup = [], []
    for tp, fp, fn in np.asarray(counts).astype(np.int64).tolist():
        den = 2 * tp + fp + fn
        f1s.append(2.0 * tp / den if den else 0.0)
        sup.append(tp + fn)
    tp, fp, fn = (int(v) for v in np.asarray(counts).astype(np.int64).sum(axis=0))
    den = 2 * tp + fp + fn
    micro = 2.0 * tp / den if den else 0.0
    macro = sum(f1s) / len(f1s) if f1s else 0.0
    weighted = sum(f * s for f, s in zip(f1s, sup)) / sum(sup) if sum(sup) else 0.0
    return micro, macro, weighted

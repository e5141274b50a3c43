"""numpy restatements for the 3-layer trainer (lt_gcn3_trainer_*, include/linkteller_hip.h): the per-layer Philox4x32-10
dropout mask and one whole epoch written out in numpy / scipy (epoch_reference3), the high-precision reference of
test_train3_backward_gpu.py.  The Philox rounds, the Adam step and the near-kink / fragile-row helpers are train_restate's."""
import numpy as np

import train_restate as T

_LO = np.uint64(0xFFFFFFFF)
NAMES3 = ("dW1", "db1", "dW2", "db2", "dW3", "db3")


def dropout_keep3(n, h, epoch, seed, p, layer):
    """bool [n, h]: element (r, j) of hidden layer ``layer`` (0 or 1) kept in epoch ``epoch`` -- i = r * h + j, word i & 3 of
    Philox(counter (q lo, q hi, epoch, layer), key (seed lo, seed hi)), q = i >> 2, kept iff >= floor(p 2^32)."""
    if p == 0:
        return np.ones((n, h), dtype=bool)
    i = np.arange(n * h, dtype=np.uint64)
    q = i >> np.uint64(2)
    ctr = np.stack([q & _LO, q >> np.uint64(32), np.full_like(q, epoch), np.full_like(q, layer)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), (q.size, 2))
    words = T.philox4x32_10(ctr, key)
    u = words[np.arange(q.size), (i & np.uint64(3)).astype(np.int64)].astype(np.uint64)
    return (u >= np.uint64(int(np.floor(p * 4294967296.0)))).reshape(n, h)


def epoch_reference3(adj, x, y, params, keep1, keep2, scale, dtype=np.float64, on1=None, on2=None):
    """One epoch of the 3-layer trainer's contract up to the gradients, in numpy / scipy in ``dtype`` with no autograd:
        Z1 = A (X W1) + b1; H1d = keep1 * scale * relu(Z1); Z2 = A (H1d W2) + b2; H2d = keep2 * scale * relu(Z2)
        Z3 = A (H2d W3) + b3; loss = mean_r (logsumexp(Z3[r]) - Z3[r, y[r]]); dZ3 = (softmax(Z3) - onehot(y)) / n
        dS3 = A^T dZ3; dW3 = H2d^T dS3; db3 = sum_r dZ3; dZ2 = on2 * keep2 * scale * (dS3 W3^T); db2 = sum_r dZ2
        dS2 = A^T dZ2; dW2 = H1d^T dS2; dZ1 = on1 * keep1 * scale * (dS2 W2^T); db1 = sum_r dZ1; dW1 = X^T (A^T dZ1)
    ``on1`` / ``on2`` (bool [n, H1] / [n, H2]) substitute the ReLU derivative patterns (None: Z_k > 0 in ``dtype``); the
    forward values do not depend on them.  Returns a dict: Z1, Z2, Z3, H1d, H2d, loss (a Python float), argmax, and the six
    gradients -- arrays in ``dtype``."""
    a = adj.tocsr().astype(dtype)
    at = a.T.tocsr()
    x = np.asarray(x).astype(dtype)
    w1, b1, w2, b2, w3, b3 = (np.asarray(p).astype(dtype) for p in params)
    y = np.asarray(y).astype(np.int64).reshape(-1)
    n = x.shape[0]
    rows = np.arange(n)
    drop1 = np.asarray(keep1).astype(dtype) * dtype(scale)
    drop2 = np.asarray(keep2).astype(dtype) * dtype(scale)
    z1 = a @ (x @ w1) + b1
    h1d = np.maximum(z1, dtype(0)) * drop1
    z2 = a @ (h1d @ w2) + b2
    h2d = np.maximum(z2, dtype(0)) * drop2
    z3 = a @ (h2d @ w3) + b3
    mx = z3.max(axis=1, keepdims=True)
    e = np.exp(z3 - mx)
    s = e.sum(axis=1, keepdims=True)
    loss = ((mx[:, 0] + np.log(s[:, 0])) - z3[rows, y]).sum(dtype=dtype) / dtype(n)
    dz3 = e / s
    dz3[rows, y] -= dtype(1)
    dz3 = dz3 / dtype(n)
    ds3 = at @ dz3
    o2 = (z2 > 0) if on2 is None else np.asarray(on2, dtype=bool)
    dz2 = (ds3 @ w3.T) * drop2 * o2.astype(dtype)
    ds2 = at @ dz2
    o1 = (z1 > 0) if on1 is None else np.asarray(on1, dtype=bool)
    dz1 = (ds2 @ w2.T) * drop1 * o1.astype(dtype)
    return dict(Z1=z1, Z2=z2, Z3=z3, H1d=h1d, H2d=h2d, loss=float(loss), argmax=z3.argmax(axis=1),
                dW1=x.T @ (at @ dz1), db1=dz1.sum(axis=0), dW2=h1d.T @ ds2, db2=dz2.sum(axis=0), dW3=h2d.T @ ds3,
                db3=dz3.sum(axis=0))

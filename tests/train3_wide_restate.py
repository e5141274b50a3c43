"""numpy / scipy restatement of one epoch of the 3-layer trainer with the wide head (lt_gcn3_trainer_create_wide,
include/linkteller_hip.h): train3_restate.epoch_reference3's two hidden layers under train_wide_restate.head_reference's head,
without autograd, for both losses; the reference of test_train3_wide_gpu.py.  The Philox masks are train3_restate's, the Adam
step and the near-kink helper train_restate's.  test_train3_wide_cpu.py checks this file against torch's fp64 autograd."""
import numpy as np

import train_wide_restate as TW

NAMES = ("dW1", "db1", "dW2", "db2", "dW3", "db3")


def epoch_reference3_wide(adj, x, y, params, keep1, keep2, scale, loss, dtype=np.float64, on1=None, on2=None):
    """One epoch of the wide GCN3 route's contract up to the gradients, in ``dtype``:
        Z1 = A (X W1) + b1; H1d = keep1 * scale * relu(Z1); Z2 = A (H1d W2) + b2; H2d = keep2 * scale * relu(Z2)
        Z3 = A (H2d W3) + b3; (loss, dZ3, counts) = head(Z3, y)
        dS3 = A^T dZ3; dW3 = H2d^T dS3; db3 = sum_r dZ3; dZ2 = on2 * keep2 * scale * (dS3 W3^T); db2 = sum_r dZ2
        dS2 = A^T dZ2; dW2 = H1d^T dS2; dZ1 = on1 * keep1 * scale * (dS2 W2^T); db1 = sum_r dZ1; dW1 = X^T (A^T dZ1)
    ``on1`` / ``on2`` (bool [n, H1] / [n, H2]) substitute the ReLU derivative patterns (None: Z_k > 0 in ``dtype``); the
    forward values do not depend on them.  Returns a dict: Z1, Z2, Z3, H1d, H2d, loss, counts, dZ3 and the six gradients."""
    a = adj.tocsr().astype(dtype)
    at = a.T.tocsr()
    x = np.asarray(x).astype(dtype)
    w1, b1, w2, b2, w3, b3 = (np.asarray(p).astype(dtype) for p in params)
    drop1 = np.asarray(keep1).astype(dtype) * dtype(scale)
    drop2 = np.asarray(keep2).astype(dtype) * dtype(scale)
    z1 = a @ (x @ w1) + b1
    h1d = np.maximum(z1, dtype(0)) * drop1
    z2 = a @ (h1d @ w2) + b2
    h2d = np.maximum(z2, dtype(0)) * drop2
    z3 = a @ (h2d @ w3) + b3
    val, dz3, counts = TW.head_reference(z3, y, loss, dtype)
    ds3 = at @ dz3
    o2 = (z2 > 0) if on2 is None else np.asarray(on2, dtype=bool)
    dz2 = (ds3 @ w3.T) * drop2 * o2.astype(dtype)
    ds2 = at @ dz2
    o1 = (z1 > 0) if on1 is None else np.asarray(on1, dtype=bool)
    dz1 = (ds2 @ w2.T) * drop1 * o1.astype(dtype)
    return dict(Z1=z1, Z2=z2, Z3=z3, H1d=h1d, H2d=h2d, loss=val, counts=counts, dZ3=dz3,
                dW1=x.T @ (at @ dz1), db1=dz1.sum(axis=0), dW2=h1d.T @ ds2, db2=dz2.sum(axis=0), dW3=h2d.T @ ds3,
                db3=dz3.sum(axis=0))

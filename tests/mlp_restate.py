"""numpy restatement of the minibatch MLP trainer's contract (include/linkteller_hip.h, lt_mlp.hip): one optimiser step and one
epoch of the feature-only baselines written out without autograd, in any dtype; the Philox shuffle; the per-step dropout mask.
Shared by test_mlp_cpu.py and the GPU tests of the MLP trainer."""
import numpy as np

import train_restate as R


def shuffle_order(n, epoch, seed):
    """int64 [n]: the Philox order of epoch ``epoch``: rows sorted ascending by (key, r), key of row r = word 0 of Philox4x32-10
    with counter (r, 0, epoch, 2) and key (seed lo, seed hi)."""
    r = np.arange(n, dtype=np.uint64)
    ctr = np.stack([r, np.zeros_like(r), np.full_like(r, epoch), np.full_like(r, 2)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), (n, 2))
    keys = R.philox4x32_10(ctr, key)[:, 0]
    return np.argsort(keys, kind="stable").astype(np.int64)


def step_keep(b, h, step, seed, p):
    """bool [b, h]: the mask of optimiser step ``step`` (steps since creation): element (j, k), j the row's position inside its
    batch -- train_restate's contract with the step in the counter's epoch word."""
    return R.dropout_keep(b, h, step, seed, p)


def step_reference(x, labels, params, rows, depth, loss="ce", keep=None, scale=1.0, dtype=np.float64, relu_on=None):
    """One step over the batch ``rows`` (row ids into x / labels) up to the gradients, in ``dtype``:
        depth 2: Z1 = X_b W1 + b1; H1d = keep * scale * relu(Z1); Z = H1d W2 + b2
        depth 1: Z = X_b W + b
        ce:  loss = mean_j (logsumexp(Z[j]) - Z[j, y_j]); dZ = (softmax(Z) - onehot(y)) / b; count = #(first argmax == y)
        bce: loss = sum (max(z, 0) - z y + log1p(exp(-|z|))) / (b C); dZ = (sigmoid(z) - y) / (b C); count = #(z > 0 and y)
        dW2 = H1d^T dZ; db2 = sum_j dZ; dZ1 = relu_on * keep * scale * (dZ W2^T); db1 = sum_j dZ1; dW1 = X_b^T dZ1
    ``relu_on`` (bool [b, H]): the ReLU's derivative; None takes Z1 > 0 in ``dtype``.  Returns a dict: Z1 (depth 2), Z, loss
    (Python float), count (int), margin (per row: ce the top-2 logit gap, bce min |z|), grads (tuple in parameter order)."""
    rows = np.asarray(rows, dtype=np.int64)
    xb = np.asarray(x)[rows].astype(dtype)
    ps = [np.asarray(p).astype(dtype) for p in params]
    b = rows.size
    out = {}
    if depth == 2:
        w1, b1, w2, b2 = ps
        z1 = xb @ w1 + b1
        drop = (np.ones_like(z1) if keep is None else np.asarray(keep).astype(dtype)) * dtype(scale)
        h1d = np.maximum(z1, dtype(0)) * drop
        z = h1d @ w2 + b2
        out["Z1"] = z1
    else:
        w, bias = ps
        z = xb @ w + bias
    c = z.shape[1]
    if loss == "ce":
        y = np.asarray(labels)[rows].astype(np.int64).reshape(-1)
        j = np.arange(b)
        mx = z.max(axis=1, keepdims=True)
        e = np.exp(z - mx)
        s = e.sum(axis=1, keepdims=True)
        lval = ((mx[:, 0] + np.log(s[:, 0])) - z[j, y]).sum(dtype=dtype) / dtype(b)
        dz = e / s
        dz[j, y] -= dtype(1)
        dz = dz / dtype(b)
        count = int((z.argmax(axis=1) == y).sum())
        top = np.sort(z, axis=1)
        margin = top[:, -1] - top[:, -2] if c > 1 else np.full(b, np.inf)
    else:
        y = (np.asarray(labels)[rows] != 0).astype(dtype)
        ez = np.exp(-np.abs(z))
        lval = ((np.maximum(z, dtype(0)) - z * y) + np.log1p(ez)).sum(dtype=dtype) / dtype(b * c)
        sig = np.where(z >= 0, dtype(1) / (dtype(1) + ez), ez / (dtype(1) + ez))
        dz = (sig - y) / dtype(b * c)
        count = int(((z > 0) & (y != 0)).sum())
        margin = np.abs(z).min(axis=1)
    out.update(Z=z, loss=float(lval), count=count, margin=margin)
    if depth == 2:
        on = (z1 > 0) if relu_on is None else np.asarray(relu_on, dtype=bool)
        dz1 = (dz @ w2.T) * drop * on.astype(dtype)
        out["grads"] = (xb.T @ dz1, dz1.sum(axis=0), h1d.T @ dz, dz.sum(axis=0))
    else:
        out["grads"] = (xb.T @ dz, dz.sum(axis=0))
    return out


def batches(order, batch_size):
    """The batches of one epoch's order: consecutive stretches of ``batch_size``, the last one shorter (drop_last=False)."""
    order = np.asarray(order, dtype=np.int64)
    return [order[o:o + batch_size] for o in range(0, order.size, batch_size)]


class State:
    """fp32 parameters and Adam moments, and the optimiser step count."""

    def __init__(self, params):
        self.params = [np.array(p, dtype=np.float32) for p in params]
        self.m = [np.zeros_like(p) for p in self.params]
        self.v = [np.zeros_like(p) for p in self.params]
        self.step = 0

    def adam(self, grads, lr, weight_decay):
        self.step += 1
        for k, g in enumerate(grads):
            self.params[k], self.m[k], self.v[k] = R.adam_step(self.params[k], np.asarray(g, dtype=np.float32), self.m[k],
                                                                self.v[k], self.step, lr, weight_decay=weight_decay)


def run_epoch(state, x, labels, order, depth, batch_size, lr, weight_decay, loss="ce", p=0.0, seed=0, dtype=np.float64):
    """One epoch on ``state`` (updated in place): per batch of ``order`` a step_reference in ``dtype`` at the current fp32
    parameters under the step's Philox mask, then Adam (train_restate.adam_step).  Returns (losses, counts) per step."""
    losses, counts = [], []
    for rows in batches(order, batch_size):
        keep = None
        if depth == 2 and p > 0:
            keep = step_keep(rows.size, state.params[0].shape[1], state.step, seed, p)
        ref = step_reference(x, labels, state.params, rows, depth, loss, keep, R.dropout_scale(p) if p > 0 else 1.0, dtype)
        losses.append(ref["loss"])
        counts.append(ref["count"])
        state.adam(ref["grads"], lr, weight_decay)
    return np.array(losses), np.array(counts, dtype=np.int64)

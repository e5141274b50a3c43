"""numpy restatements of the training kernels' bit-level contracts (include/linkteller_hip.h, lt_train.hip): the
Philox4x32-10 dropout mask and the fp32 Adam op order; and one whole epoch written out in numpy / scipy (epoch_reference), the
high-precision reference of test_train_backward_gpu.py.  Shared by test_train_cpu.py and the GPU training tests."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: uint32 [..., 2] -> uint32 [..., 4]."""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] for i in range(4)]
    k0, k1 = (np.asarray(key, dtype=np.uint64)[..., i] for i in range(2))
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _LO, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _LO]
    return np.stack(c, axis=-1).astype(np.uint32)


def dropout_keep(n, h, epoch, seed, p):
    """bool [n, h]: element (r, j) kept in epoch `epoch` (i = r * h + j, word i & 3 of Philox(counter (q lo, q hi, epoch, 0),
    key (seed lo, seed hi)), q = i >> 2, kept iff >= floor(p 2^32))."""
    if p == 0:
        return np.ones((n, h), dtype=bool)
    i = np.arange(n * h, dtype=np.uint64)
    q = i >> np.uint64(2)
    ctr = np.stack([q & _LO, q >> np.uint64(32), np.full_like(q, epoch), np.zeros_like(q)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), (q.size, 2))
    words = philox4x32_10(ctr, key)
    u = words[np.arange(q.size), (i & np.uint64(3)).astype(np.int64)].astype(np.uint64)
    return (u >= np.uint64(int(np.floor(p * 4294967296.0)))).reshape(n, h)


def dropout_scale(p):
    return np.float32(1.0 / (1.0 - p)) if p < 1 else np.float32(0)


def epoch_reference(adj, x, y, params, keep, scale, dtype=np.float64, relu_on=None):
    """One epoch of the trainer's contract (include/linkteller_hip.h) up to the gradients, written out in numpy / scipy
    in ``dtype`` with no autograd:
        S1 = X W1; Z1 = A S1 + b1; H1d = keep * scale * relu(Z1); Z2 = A (H1d W2) + b2
        loss = mean_r (logsumexp(Z2[r]) - Z2[r, y[r]]); dZ2 = (softmax(Z2) - onehot(y)) / n; dS2 = A^T dZ2
        dW2 = H1d^T dS2; db2 = sum_r dZ2; dZ1 = relu_on * keep * scale * (dS2 W2^T); db1 = sum_r dZ1; dW1 = X^T (A^T dZ1)
    ``keep`` is the dropout mask (bool [n, H]), ``scale`` its 1 / (1 - p).  ``relu_on`` (bool [n, H]) is the derivative of the
    ReLU; None takes Z1 > 0 in ``dtype``.  Passing it lets a caller evaluate the gradients with chosen elements switched
    off or on (the forward values do not depend on it).  Returns a dict: Z1, Z2, loss (a Python float), argmax (first
    maximum of each row), dW1, db1, dW2, db2 -- arrays in ``dtype``."""
    a = adj.tocsr().astype(dtype)
    at = a.T.tocsr()
    x = np.asarray(x).astype(dtype)
    w1, b1, w2, b2 = (np.asarray(p).astype(dtype) for p in params)
    y = np.asarray(y).astype(np.int64).reshape(-1)
    n = x.shape[0]
    rows = np.arange(n)
    z1 = a @ (x @ w1) + b1
    drop = np.asarray(keep).astype(dtype) * dtype(scale)
    h1d = np.maximum(z1, dtype(0)) * drop
    z2 = a @ (h1d @ w2) + b2
    mx = z2.max(axis=1, keepdims=True)
    e = np.exp(z2 - mx)
    s = e.sum(axis=1, keepdims=True)
    loss = ((mx[:, 0] + np.log(s[:, 0])) - z2[rows, y]).sum(dtype=dtype) / dtype(n)
    dz2 = e / s
    dz2[rows, y] -= dtype(1)
    dz2 = dz2 / dtype(n)
    ds2 = at @ dz2
    on = (z1 > 0) if relu_on is None else np.asarray(relu_on, dtype=bool)
    dz1 = (ds2 @ w2.T) * drop * on.astype(dtype)
    return dict(Z1=z1, Z2=z2, loss=float(loss), argmax=z2.argmax(axis=1), dW1=x.T @ (at @ dz1), db1=dz1.sum(axis=0),
                dW2=h1d.T @ ds2, db2=dz2.sum(axis=0))


def near_kink(z1_64, z1_32, keep):
    """(tau, bool [n, H]): the kept pre-activations within tau = 8 max|Z1_fp32 - Z1_fp64| of the ReLU's kink.  An fp32
    evaluation whose error is within twice the fp32 reference's may put such an element on the other side (a flip needs an
    error of at least |z|; 8 is a 4x margin over that), and then its derivative legitimately differs from the fp64 one."""
    tau = 8.0 * float(np.abs(np.asarray(z1_32, dtype=np.float64) - z1_64).max())
    return tau, np.asarray(keep, dtype=bool) & (np.abs(z1_64) <= tau)


def fragile_rows(z2, tiny=1e-4):
    """Rows whose top-2 logit margin is below ``tiny``: their argmax may differ between two roundings (the convention of
    golden/generate_train.py).  A single class has no second logit and no fragile row."""
    if z2.shape[1] < 2:
        return 0
    top = np.sort(z2, axis=1)
    return int((np.abs(top[:, -1] - top[:, -2]) < tiny).sum())


def fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c): a * b is exact in float64; the float64 sum's rounding error (TwoSum) decides
    the one case where rounding that sum to float32 would round twice (a sum exactly halfway between two floats)."""
    a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c)))
    prod = a * b
    s = prod + c
    bb = s - prod
    err = (prod - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    halfway = (bits & 0x1FFFFFFF) == 0x10000000
    fix = halfway & (err != 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, sqrt=np.sqrt):
    """One step of lt_adam_step in numpy fp32 (returns new p, m, v): torch's _single_tensor_adam op by op with the
    rounding of torch's CPU kernels -- the weight-decay add, lerp_ and addcmul_ are fused multiply-adds there -- except
    that sqrt is correctly rounded (``sqrt`` may substitute another); the Python scalars are formed in double and rounded
    once to float32."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    bc1 = 1.0 - beta1 ** float(step)
    bc2 = 1.0 - beta2 ** float(step)
    if weight_decay != 0:
        g = fma32(p, f(weight_decay), g)
    w1 = f(1.0 - beta1)
    d = g - m
    m = fma32(w1, d, m) if w1 < 0.5 else fma32(w1 - f(1), d, g)
    v = v * f(beta2)
    v = fma32(f(1.0 - beta2) * g, g, v)
    denom = np.asarray(sqrt(v), dtype=np.float32) / f(bc2 ** 0.5) + f(eps)
    p = p + (f(-(lr / bc1)) * m) / denom
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)

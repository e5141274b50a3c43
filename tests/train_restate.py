"""numpy restatements of the training kernels' bit-level contracts (include/linkteller_hip.h, lt_train.hip): the
Philox4x32-10 dropout mask and the fp32 Adam op order.  Shared by test_train_cpu.py and test_train_gpu.py."""
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

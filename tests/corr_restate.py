"""The plain restatement of lt_corr_square / lt_corr_pairs shared by tests/test_corr_cpu.py and tests/test_corr_gpu.py (numpy only):
widen to float64, column mean, centre, ``d @ d.T``, ``g / n_i / n_j`` with the norms from the Gram's own diagonal.

``well_conditioned`` is the input check the tests assert on the CPU: every non-degenerate centred row has
``||d_i||_inf >= 1e-3 max|x|``.  Then no score is a quotient of cancelled quantities and two fp64 summation orders of it differ
by far less than ORDER_SLACK (measured on the shapes of the tests: at most 5e-16).

GATE is the value gate of the GPU tests: half an fp32 ulp at |s| <= 1 (the ONE rounding of the store) plus ORDER_SLACK.  An fp32
Gram errs by 1e-7 and more on these inputs and cannot pass it."""
import numpy as np

ORDER_SLACK = 1e-12
GATE = 2.0 ** -25 + ORDER_SLACK


def centred(V, rows=None):
    """float64 rows of V (all, or the listed ones) minus the column mean over exactly those rows."""
    x = np.asarray(V)[:, :] if rows is None else np.asarray(V)[np.asarray(rows, dtype=np.int64)]
    x = x.astype(np.float64)
    return x - x.sum(axis=0) / x.shape[0]


def square(V, nodes):
    """float64 [k, k]: the correlation of rows nodes[i], nodes[j], the mean over the k listed rows (repeats count).  NaN where a
    centred row is zero (0 / 0), as the reference."""
    d = centred(V, nodes)
    g = d @ d.T
    nrm = np.sqrt(np.diag(g))
    with np.errstate(invalid="ignore", divide="ignore"):
        s = g / nrm[:, None] / nrm[None, :]
    s[nrm == 0, :] = np.nan
    s[:, nrm == 0] = np.nan
    return s


def pairs(V, u, v):
    """float64 [m]: the correlation of rows u[p], v[p], the mean over ALL rows."""
    d = centred(V)
    nrm = np.sqrt((d * d).sum(axis=1))
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (d[u] * d[v]).sum(axis=1) / nrm[u] / nrm[v]
    s[(nrm[u] == 0) | (nrm[v] == 0)] = np.nan
    return s


def well_conditioned(V, rows=None):
    """min over the non-degenerate centred rows of ||d_i||_inf >= 1e-3 max|x| (rows: the square's sample; None: all rows)."""
    d = centred(V, rows)
    inf = np.abs(d).max(axis=1)
    inf = inf[inf > 0]
    x = np.asarray(V) if rows is None else np.asarray(V)[np.asarray(rows, dtype=np.int64)]
    return inf.size == 0 or float(inf.min()) >= 1e-3 * float(np.abs(x).max())


def fp32_square(V, nodes):
    """The reference's own arithmetic (attacker.py:305-313) in torch float32 on the CPU, widened."""
    import torch
    vec = torch.from_numpy(np.ascontiguousarray(V, dtype=np.float32))
    nodes = torch.as_tensor(np.asarray(nodes, dtype=np.int64))
    d = vec[nodes] - torch.mean(vec[nodes], dim=0)
    nrm = torch.norm(d, dim=1)
    return ((d @ d.T) / nrm[:, None] / nrm[None, :]).numpy().astype(np.float64)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def normal_rows(rng, n, D):
    return rng.standard_normal((n, D)).astype(np.float32)


def softmax_rows(rng, n, C):
    z = rng.standard_normal((n, C)) * 2.0
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def indicator_rows(rng, n, D, density=0.1):
    """0/1 indicator columns standardised per column in float32 (what the twitch loader hands the model); an all-equal column
    stays zero."""
    x = (rng.random_sample((n, D)) < density).astype(np.float32)
    mu, sd = x.mean(axis=0, dtype=np.float32), x.std(axis=0, dtype=np.float32)
    sd[sd == 0] = 1.0
    return ((x - mu) / sd).astype(np.float32)

"""A numpy restatement of the three fixed-point storage forms behind the default `delta` path, and of the `delta` arithmetic in
fp64 behind them: what the stored precision alone costs, rounding realisations aside.

  * rows31: the fp64 product rows S1 = X W1 leave as 32-bit fixed point, 31 bits against the row's largest value over all hidden
    units (k_sum_slabs_f64_q, k_quant_rows_f64, the store of k_s1d_feature_rows);
  * i8_x / i8_w: the int8 split of the dense product cuts X to 39 bits against the largest value of its (row, K slice) and W1 to 31
    bits against the largest value of its (column, K slice) (lt_i8_split.hip.h); K slices as lt_i8_steps_per_slice cuts them.

An absolute error eps in a stored term reaches the score as eps / delta wherever a unit crosses its ReLU kink, so a unit whose
values are 2^-k of its row's (or slice's) largest loses k bits of the storage's resolution.

Deliberately left out:
  * the digit-pair orders below 3 that the int8 split drops (< 2^-38 of a full-scale term) and its one fp64 rounding per K slice;
  * every fp32 rounding after the kink test (dh, the products with W2, the sums over a row's members, the norm): they are
    relative errors of 2^-24 on terms that carry no cancellation;
  * the feature route (route 1) stores S1d - cref, the differences to the reference row's product, and adds cref back in fp64: its
    row maxima are not those of S1, so for route 1 `rows31` is an ESTIMATE of the stored precision, not the kernel's arithmetic;
  * the aggregate-first route (route 2) keeps fp64 throughout: nothing to model, its storage is `none`.  The 3-layer baseline
    takes its layer-1 pre-activation from an inner 2-layer baseline that is pinned off aggregate-first, so its product rows are
    `rows31` (F < 256: no int8 split); its second layer is fp64 and inherits the first's error through relu(Z1) W2;
  * the order of the fp64 sums."""
import numpy as np

ROW_STEPS = 2147483000.0
I8_KS = 32


def rows31(s):
    mx = np.abs(s).max(axis=1, keepdims=True)
    scale = np.where(mx > 0, mx / ROW_STEPS, 1.0)
    return np.rint(s / scale) * scale


def i8_steps_per_slice(n, h, f):
    """lt_i8_steps_per_slice: as many K slices as keep the 64 x 128 tiles within 512 workgroups, at least 8 steps of 32 columns."""
    steps = (f + I8_KS - 1) // I8_KS
    tiles = ((n + 63) // 64) * (((h + 63) // 64 * 64 + 127) // 128)
    want = max(512 // tiles, 1)
    per = max((steps + want - 1) // want, 8)
    return max(min(per, steps), 1)


def i8_slices(n, h, f):
    per = i8_steps_per_slice(n, h, f) * I8_KS
    return [(k0, min(k0 + per, f)) for k0 in range(0, f, per)]


def _exponent(mx):
    """e with mx < 2^e (i8_exponent: the biased exponent of the largest value - 126), clamped at -96."""
    return np.maximum(np.frexp(mx)[1], -96)


def _fixed(v, mx, bits):
    e = _exponent(mx).astype(np.float64)
    return np.rint(v * 2.0 ** (bits - e)) * 2.0 ** (e - bits)


def i8_x(x, slices):
    out = np.empty_like(x, dtype=np.float64)
    for k0, k1 in slices:
        out[:, k0:k1] = _fixed(x[:, k0:k1].astype(np.float64), np.abs(x[:, k0:k1]).max(axis=1, keepdims=True).astype(np.float64), 38)
    return out


def i8_w(w1, slices):
    out = np.empty_like(w1, dtype=np.float64)
    for k0, k1 in slices:
        out[k0:k1] = _fixed(w1[k0:k1].astype(np.float64), np.abs(w1[k0:k1]).max(axis=0, keepdims=True).astype(np.float64), 30)
    return out


def product_rows(x, w1, rows=None, i8=False, h_slices=None):
    """S1 = X W1 in fp64 behind the chosen storage.  h_slices: (first unit, end, stored) of the hidden slices a wide model is
    served in (each a baseline of its own: its own K slices, its own row maxima, its own route -- `stored` False: plain fp64)."""
    n, f = x.shape
    h = w1.shape[1]
    out = np.empty((n, h))
    for s0, s1, stored in (h_slices or [(0, h, True)]):
        xs, ws = x.astype(np.float64), w1[:, s0:s1].astype(np.float64)
        if i8 and stored:
            sl = i8_slices(n, s1 - s0, f)
            xs, ws = i8_x(x, sl), i8_w(w1[:, s0:s1], sl)
        s = xs @ ws
        out[:, s0:s1] = rows31(s) if rows == "rows31" and stored else s
    return out


def relu_diff(z, dz):
    """relu(z + dz) - relu(z), piecewise as stage A writes it (no subtraction of nearly equal numbers)."""
    z1 = z + dz
    return np.where(z > 0.0, np.where(z1 > 0.0, dz, -z), np.where(z1 > 0.0, z1, 0.0))


def delta_fp64(a_hat, x, w, probes, obs, delta=1e-4, rows=None, i8=False, h_slices=None):
    """[n_probe, n_obs]: the perturbation delta * X[v] of each probe v propagated exactly through the layers, in fp64 except
    dz = A_hat[r, v] * (delta * S1[v]), which is rounded to fp32 at each step as the kernel forms it."""
    a = a_hat.astype(np.float64).tocsr()
    at = a.T.tocsr()
    depth = 3 if "W3" in w else 2
    d32 = np.float32(delta)
    s1 = product_rows(x, w["W1"], rows, i8, h_slices)
    z = [a @ s1 + w["b1"].astype(np.float64)]
    for l in range(2, depth):
        z.append(a @ (np.maximum(z[-1], 0.0) @ w[f"W{l}"].astype(np.float64)) + w[f"b{l}"].astype(np.float64))
    out = np.zeros((len(probes), len(obs)))
    a_obs = a[np.asarray(obs)]
    for i, v in enumerate(probes):
        col = at[int(v)]
        ds = d32 * s1[int(v)].astype(np.float32)
        dh = np.zeros_like(z[0])
        dz = (col.data.astype(np.float32)[:, None] * ds[None, :]).astype(np.float64)
        dh[col.indices] = relu_diff(z[0][col.indices], dz)
        for l in range(2, depth):
            dh = relu_diff(z[l - 1], a @ (dh @ w[f"W{l}"].astype(np.float64)))
        out[i] = np.linalg.norm(a_obs @ (dh @ w[f"W{depth}"].astype(np.float64)), axis=1) / float(d32)
    return out

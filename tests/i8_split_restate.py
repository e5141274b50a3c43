"""The arithmetic of the int8 split of the dense fp64 product (lt_i8_split.hip.h: k_i8_w_max, k_i8_w_digits, k_gemm_i8split<AV, 3>;
the slab sums and the 32-bit row storage of lt_fp64.hip: k_sum_slabs_f64, k_sum_slabs_f64_q, k_quant_rows_f64) restated in numpy,
EXACTLY: the route is integer arithmetic with one rounding per K slice, so what the kernels leave is compared bit for bit.

Per K slice (value_domain_model.i8_slices: a function of the FULL product's n, never of the row range formed):
  * ex[row] = max(biased exponent of the largest |x| of the slice - 126, -96); ew[col] the same over the slice's rows of W1;
  * qx = rint(double(x) * 2^(38 - ex)); qw = rintf(w * 2^(30 - ew)) in fp32 (a power of two: the scaling itself is exact);
  * balanced base-256 digits, d = ((q + 128) & 255) - 128, q = (q - d) >> 8, the top digit what remains: five of X, four of W1;
  * A_o = sum of DX_i @ DW_j over the pairs with i + j = o, for the orders o = 3 .. 7 (fourteen pairs);
  * v = sum_o A_o 256^(o - 3) in int64, slab = ldexp(double(v), ex + ew - 44).
The product is slab 0 plus the slabs 1, 2, ... in slice order; the stored form is one scale per row, mx * (1 / 2147483000) (a
product with the rounded reciprocal, not a division), and words rint(value * (1 / scale)).

Why float64 BLAS forms the integer sums exactly: a digit product is at most 2^14, an order has at most 4 pairs and a slice is less
than 2^15 columns deep, so every partial sum is an integer below 2^31 < 2^53 whatever the order of the additions (asserted).  The
same count is why the kernel's int32 accumulators cannot wrap: 4 * 2^14 * K_slice reaches 2^31 only at K_slice = 2^15 columns of
digits that are ALL +-128, and the shapes rule keeps F < 2^15; with the slicing rule a slice that deep needs an X of gigabytes, so no
test forms one.

Left out on purpose: fp32 denormals (whether the compiler flushes them is not this arithmetic's business) and non-finite values
(the engine refuses them; the kernel answers NaN).

`variant` restates a MISTAKE instead (tests/test_i8_split_cpu.py: inputs on which every one of them changes the bits can see it)."""
import types

import numpy as np

from value_domain_model import i8_slices

XD, WD, ORD_MIN = 5, 4, 3
PAIRS = [(i, j) for i in range(XD) for j in range(WD) if i + j >= ORD_MIN]
ROW_STEPS_INV = 1.0 / 2147483000.0


def exponent(mx32):
    """i8_exponent: e with |x| < 2^e from the bits of the largest |x| (fp32), clamped at -96."""
    bits = np.ascontiguousarray(mx32, dtype=np.float32).view(np.uint32)
    assert (bits < 0x7f800000).all(), "non-finite values are not restated"
    return np.maximum((bits >> 23).astype(np.int64) - 126, -96)


def digits(q, nd, check=True):
    out = []
    q = q.astype(np.int64)
    for _ in range(nd - 1):
        d = ((q + 128) & 255) - 128
        q = (q - d) >> 8
        out.append(d)
    out.append(q)
    if check:
        assert all(d.min() >= -128 and d.max() <= 127 for d in out), "a digit left [-128, 127]"
    return out


def restate_slabs(x, w1, n_full, variant=None):
    """[slices, rows of x, H] float64: the slabs k_gemm_i8split<AV, 3> leaves for these rows of an n_full-row product.
    variant: ("drop", i, j) one digit pair lost; ("trunc", "w" | "x") truncation in place of rint; ("skip32",) the first 32 columns
    of a slice left out of a row's exponent.  The range assertions hold for the true arithmetic only."""
    assert x.dtype == np.float32 and w1.dtype == np.float32
    m, f = x.shape
    h = w1.shape[1]
    check = variant is None
    kind = variant[0] if variant else None
    slices = i8_slices(n_full, h, f)
    slabs = np.empty((len(slices), m, h))
    for s, (k0, k1) in enumerate(slices):
        xs, ws = x[:, k0:k1], w1[k0:k1]
        seen = xs[:, 32:] if kind == "skip32" and k1 - k0 > 32 else xs
        ex = exponent(np.abs(seen).max(axis=1))
        ew = exponent(np.abs(ws).max(axis=0))
        sx = np.ldexp(xs.astype(np.float64), (38 - ex)[:, None])
        sw = ws * np.ldexp(np.float32(1.0), (30 - ew).astype(np.int32))[None, :]
        assert sw.dtype == np.float32
        with np.errstate(invalid="ignore" if variant else "warn"):       # (a mistaken exponent may push a value past int64)
            qx = (np.trunc(sx) if variant == ("trunc", "x") else np.rint(sx)).astype(np.int64)
        qw = (np.trunc(sw) if variant == ("trunc", "w") else np.rint(sw)).astype(np.int64)
        dx = [d.astype(np.float64) for d in digits(qx, XD, check)]
        dw = [d.astype(np.float64) for d in digits(qw, WD, check)]
        v = np.zeros((m, h), dtype=np.int64)
        for o in range(ORD_MIN, XD + WD - 1):
            a = np.zeros((m, h))
            for i, j in PAIRS:
                if i + j == o and variant != ("drop", i, j):
                    a += dx[i] @ dw[j]
            if check:
                assert np.abs(a).max(initial=0.0) < 2.0 ** 31
            v += a.astype(np.int64) << (8 * (o - ORD_MIN))
        if check:
            assert np.abs(v).max(initial=0) < 1 << 60
        slabs[s] = np.ldexp(v.astype(np.float64), (ex[:, None] + ew[None, :] - 68 + 8 * ORD_MIN).astype(np.int32))
    return slabs


def sum_slabs(slabs, reverse=False):
    """k_sum_slabs_f64 / k_sum_slabs_f64_q: slab 0, then + slab 1, + slab 2, ... (reverse: the mistake of starting at the end)."""
    order = range(len(slabs))[::-1] if reverse else range(len(slabs))
    acc = None
    for z in order:
        acc = slabs[z].copy() if acc is None else acc + slabs[z]
    return acc


def restate_product(x, w1, n_full=None, variant=None):
    n_full = x.shape[0] if n_full is None else n_full
    if variant == ("reverse",):
        return sum_slabs(restate_slabs(x, w1, n_full), reverse=True)
    return sum_slabs(restate_slabs(x, w1, n_full, variant))


def restate_stored(product):
    """(int32 words, float64 scales) of k_sum_slabs_f64_q / k_quant_rows_f64 for finished fp64 rows."""
    mx = np.abs(product).max(axis=1)
    scale = np.where(mx > 0.0, mx * ROW_STEPS_INV, 1.0)
    inv = 1.0 / scale
    return np.rint(product * inv[:, None]).astype(np.int32), scale


# ---- the inputs of the GPU tests (and of the sensitivity test that asks whether they can see a mistake) -------------------------
ONES = np.float32(2.0 - 2.0 ** -23)        # all mantissa bits set
DIGIT_WORDS = (0x808080, 0x7f7f7f, 0x800000, 0xffffff, 0x808081, 0x7f7f80, 0x008080, 0x007f80, 0x80, 0x7f, 0x8000, 0x7fff)


def plant_edges(x, w1, slices):
    """Rows of X and columns of W1 at the edges of the fixed point, in place.  Rows sit in the first tile (0, 5, 17, 33, 63), across
    the first tile boundary (64), further on and in the last row; every pattern restarts at each K slice, so that a slice's exponent
    is the one the pattern was written for."""
    n, f = x.shape
    h = w1.shape[1]
    rows = [0, 5, 17, 33, 63, 64, 100, 130, 131, 200, 201, n - 1]
    x[rows[0]] = 0.0                                          # an all-zero row
    if len(slices) > 1:
        x[rows[1], slices[-1][0]:] = 0.0                      # zero in the last slice only
    else:
        x[rows[1], :32] = 0.0                                 # (one slice: a zero first step)
    x[rows[2]] = -ONES                                        # all mantissa ones, negative
    x[rows[3]] = np.clip(x[rows[3]], -3.0, 3.0)
    x[rows[4]] = -0.0
    x[rows[6]] = np.float32(1e-30)                            # the exponent clamp at -96
    x[rows[7], min(21, f - 1)] = np.float32(2.0 ** 40)                    # a huge value next to ordinary ones (second half of a step's columns)
    x[rows[8], 5] = np.float32(-2.0 ** 40)                    # ... and in the first half
    sign = np.where(np.arange(f) % 3 == 2, -1.0, 1.0)
    for k0, k1 in slices:
        k = np.arange(k1 - k0)
        x[rows[3], k0 + min(17, k1 - k0 - 1)] = 4.0           # the largest value an exact power of two
        # 3.0 leads (ex = 2, one step of the fixed point is 2^-36): digit bytes at -128 and 127 with carries, in the low, middle and
        # high digits (every value is a 24-bit integer times a power of two: an fp32)
        words = np.array([DIGIT_WORDS[i % len(DIGIT_WORDS)] for i in k], dtype=np.float64) * 2.0 ** np.array([(0, 8, 14)[(i // 12) % 3] for i in k])
        pat = words * 2.0 ** -36 * sign[k0:k1]
        pat[0] = 3.0
        assert np.abs(pat).max() < 4.0
        x[rows[-1], k0:k1] = x[rows[5], k0:k1] = pat.astype(np.float32)
        # 1.0 leads (ex = 1, one step is 2^-37): halves of a step are ties (to even), quarters are not
        tie = np.array([(1, 3, 5, 7, -1, -3, -5)[i % 7] for i in k], dtype=np.float64) * 2.0 ** -38
        tie[0] = 1.0
        x[rows[9], k0:k1] = tie.astype(np.float32)
        quarter = np.array([(3, 1, -3, -1)[i % 4] for i in k], dtype=np.float64) * 2.0 ** -39
        quarter[0] = 1.0
        x[rows[10], k0:k1] = quarter.astype(np.float32)
    cols = [0, 31, 32, 63, h - 1, h - 2]
    w1[:, cols[0]] = 0.0                                      # an all-zero column
    if len(slices) > 1:
        w1[slices[-1][0]:, cols[1]] = 0.0                     # zero in the last slice only
    else:
        w1[:32, cols[1]] = 0.0
    w1[:, cols[2]] = (ONES * np.float32(0.125)) * np.where(np.arange(f) % 2, -1.0, 1.0).astype(np.float32)
    w1[:, cols[4]] = np.float32(1e-30)
    for k0, k1 in slices:
        k = np.arange(k1 - k0)
        # 1.0 leads (ew = 1, one step is 2^-29): halves of a step are ties in rintf, and to even every one of these rounds DOWN by
        # half a step -- against the row of -ONES the errors add up to nearly the whole bound; 1.5 * 2^-31 (three eighths) is no tie
        tie = np.array([(1, 5, 9, -3, -7, 13, -11)[i % 7] for i in k], dtype=np.float64) * 2.0 ** -30
        tie[0] = 1.0
        w1[k0:k1, cols[3]] = tie.astype(np.float32)
        eighth = np.array([(1.5, -1.5)[i % 2] for i in k], dtype=np.float64) * 2.0 ** -31
        eighth[0] = 1.0
        w1[k0:k1, cols[5]] = eighth.astype(np.float32)
    return rows, cols


SHAPES = [(256, 256, 64), (257, 257, 192), (319, 258, 128), (301, 544, 256), (301, 1400, 64), (5441, 544, 256), (16449, 288, 256)]
_cases = {}


def case(n, f, h, i8=True):
    """Gaussian features, gcn_weights, the planted edges (i8: the patterns restart at the int8 split's K slices; else once per row);
    built once per shape and never changed."""
    if (n, f, h, i8) not in _cases:
        from linkteller_amd import synth
        x = synth.gaussian_features(n, f, seed=n + f)
        w = synth.gcn_weights(f, h, 2, seed=h + f)
        rows, cols = plant_edges(x, w["W1"], i8_slices(n, h, f) if i8 else [(0, f)])
        for a in [x] + list(w.values()):
            a.setflags(write=False)
        _cases[(n, f, h, i8)] = types.SimpleNamespace(n=n, f=f, h=h, x=x, w=w, rows=rows, cols=cols)
    return _cases[(n, f, h, i8)]

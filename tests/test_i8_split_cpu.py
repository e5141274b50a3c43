"""The numpy restatement of the int8 split (tests/i8_split_restate.py) is itself right -- against exact arithmetic, within a derived
bound -- and the inputs the GPU tests run it on can see the mistakes a kernel could make.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import i8_split_restate as R
from value_domain_model import i8_slices

# Per term x w of a slice, with |x| < 2^ex and |w| < 2^ew:
#   x = qx 2^(ex - 38) + dx, |dx| <= 2^(ex - 39);  w = qw 2^(ew - 30) + dw, |dw| <= 2^(ew - 31)
#   |x w - qx qw 2^(ex + ew - 68)| <= |dx| |w| + |x| |dw| + |dx| |dw| < 2^(ex + ew) (2^-39 + 2^-31 + 2^-70)
#   the six digit pairs of order 0, 1 and 2 that are dropped, every digit at most 128 in size:
#   128^2 (1 + 2 * 256 + 3 * 65536) 2^(ex + ew - 68) = 197121 * 2^-54 * 2^(ex + ew)        (= 2^-36.41 2^(ex + ew))
TERM = 2.0 ** -39 + 2.0 ** -31 + 2.0 ** -70 + 197121 * 2.0 ** -54


def error_bound(x, w1, n_full):
    """Entry by entry: sum over the slices of K_slice 2^(ex + ew) TERM, plus the fp64 roundings -- one where a slice's integer becomes
    a double and one where its slab is added, each at most 2^-53 of a sum that |X| |W1| (with its own error, < 2^-20 of it) bounds."""
    h = w1.shape[1]
    slices = i8_slices(n_full, h, x.shape[1])
    bound = np.zeros((x.shape[0], h))
    for k0, k1 in slices:
        ex = R.exponent(np.abs(x[:, k0:k1]).max(axis=1)).astype(np.float64)
        ew = R.exponent(np.abs(w1[k0:k1]).max(axis=0)).astype(np.float64)
        bound += (k1 - k0) * TERM * 2.0 ** (ex[:, None] + ew[None, :])
    mag = np.abs(x).astype(np.float64) @ np.abs(w1).astype(np.float64)
    return bound + 2 * len(slices) * 2.0 ** -53 * (1 + 2.0 ** -20) * mag


def test_restatement_against_exact_arithmetic():
    """A 40 x 300 x 8 product (two slices, 256 + 44 columns; planted rows and columns as far as they fit) against Python fractions
    -- fp32 values are dyadic, the product is exact -- and the shapes of the GPU tests against np.longdouble (64 mantissa bits: its
    own error, F 2^-64 |X| |W1|, is 2^-22 of the bound's smallest term).  The error stays within error_bound, entry by entry.

    Largest observed error / bound: 0.967 on the small case, 0.966 .. 0.970 on the seven shapes of the GPU tests -- the row of all
    mantissa ones against the column whose rintf ties all round the same way; gaussian rows and columns alone stay below 0.01."""
    rng = np.random.RandomState(11)
    x = rng.standard_normal((40, 300)).astype(np.float32)
    w1 = rng.uniform(-0.35, 0.35, (300, 8)).astype(np.float32)
    x[0] = 0.0
    x[1] = -R.ONES
    x[2] = np.float32(1e-30)
    x[3, 21] = np.float32(2.0 ** 40)
    x[4, 1:] = (np.array([R.DIGIT_WORDS[i % 12] for i in range(299)]) * 2.0 ** -36).astype(np.float32)
    x[4, 0] = x[4, 256] = 3.0
    x[5] = (np.array([(1, 3, 5, -1, -3)[i % 5] for i in range(300)]) * 2.0 ** -38).astype(np.float32)
    x[5, 0] = x[5, 256] = 1.0
    w1[:, 0] = 0.0
    w1[:, 1] = R.ONES
    w1[:, 2] = (np.array([(1, 5, -3, -7)[i % 4] for i in range(300)]) * 2.0 ** -30).astype(np.float32)      # (ties that all round down)
    w1[0, 2] = w1[256, 2] = 1.0
    w1[:, 3] = np.float32(1e-30)
    got = R.restate_product(x, w1)
    fx = [[Fraction(float(v)) for v in row] for row in x]
    fw = [[Fraction(float(w1[k, c])) for k in range(300)] for c in range(8)]
    bound = error_bound(x, w1, 40)
    worst = 0.0
    for r in range(40):
        for c in range(8):
            exact = sum(a * b for a, b in zip(fx[r], fw[c]))
            err = abs(Fraction(float(got[r, c])) - exact)
            assert err <= Fraction(float(bound[r, c])), (r, c)
            worst = max(worst, float(err / Fraction(float(bound[r, c]))) if bound[r, c] > 0 else 0.0)
    print(f"40 x 300 x 8 against fractions: largest error {worst:.3f} of the bound")
    assert worst > 0.01, "the bound is idle: nothing in this input comes near it"
    for n, f, h in R.SHAPES:
        cs = R.case(n, f, h)
        keep = np.arange(n) if n < 1000 else np.r_[0:64, n - 100:n]
        xs = cs.x[keep]
        got = R.restate_product(xs, cs.w["W1"], n)
        exact = xs.astype(np.longdouble) @ cs.w["W1"].astype(np.longdouble)
        err = np.abs(got.astype(np.longdouble) - exact).astype(np.float64)
        bound = error_bound(xs, cs.w["W1"], n)
        ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
        print(f"{(n, f, h)}: largest error {ratio.max():.3f} of the bound; {err.max() / np.abs(exact).max():.3g} of the largest value")
        assert (err <= bound).all()


def test_the_inputs_see_every_restated_mistake():
    """On the inputs of the GPU tests the restated bits change under every mistake: any one of the fourteen digit pairs dropped,
    truncation in place of rint (of W1's fixed point, of X's), the first 32 columns of a slice left out of a row's exponent, and
    the slabs summed last to first (where there are three or more: two commute)."""
    for n, f, h in R.SHAPES:
        cs = R.case(n, f, h)
        keep = np.arange(n) if n < 1000 else np.r_[0:64, n - 100:n]
        xs, w1 = cs.x[keep], cs.w["W1"]
        want = R.restate_product(xs, w1, n)
        assert np.isfinite(want).all()
        variants = [("drop", i, j) for i, j in R.PAIRS] + [("trunc", "w"), ("trunc", "x"), ("skip32",)]
        if len(i8_slices(n, h, f)) >= 3:
            variants.append(("reverse",))
        assert len(R.PAIRS) == 14
        for v in variants:
            other = R.restate_product(xs, w1, n, variant=v)
            changed = (other != want).mean()
            assert changed > 0, f"{(n, f, h)}: variant {v} leaves every bit as it is: these inputs cannot see it"


def test_variants_stay_close():
    """The mistakes are subtle ones: each stays within 1e-6 of the row's largest value (so no fp32 score would show it)."""
    cs = R.case(301, 544, 256)
    rows = [r for r in range(301) if r not in cs.rows]
    xs, w1 = cs.x[rows], cs.w["W1"]
    want = R.restate_product(xs, w1, 301)
    top = np.abs(want).max(axis=1, keepdims=True)
    for v in [("drop", 0, 3), ("trunc", "w"), ("reverse",)]:
        other = R.restate_product(xs, w1, 301, variant=v)
        assert (np.abs(other - want) / top).max() < 1e-6


@pytest.mark.parametrize("shape,lengths", [
    ((256, 256, 64), [256]),
    ((257, 257, 192), [256, 1]),
    ((319, 258, 128), [256, 2]),
    ((301, 544, 256), [256, 256, 32]),
    ((301, 1400, 64), [256] * 5 + [120]),
    ((5441, 544, 256), [288, 256]),
    ((16449, 288, 256), [288]),
])
def test_slicing_of_the_shapes(shape, lengths):
    n, f, h = shape
    sl = i8_slices(n, h, f)
    assert [k1 - k0 for k0, k1 in sl] == lengths
    assert sl[0][0] == 0 and sl[-1][1] == f and all(a[1] == b[0] for a, b in zip(sl[:-1], sl[1:]))
    assert shape in R.SHAPES


def test_stored_form_is_a_product_with_the_rounded_reciprocal():
    """restate_stored: scale = mx * (1 / 2147483000), not mx / 2147483000 -- the two differ in the last bit for some rows, and the
    inputs of the GPU tests hold such rows."""
    for n, f, h in [(257, 257, 192), (301, 1400, 64), (256, 256, 64)]:
        cs = R.case(n, f, h)
        prod = R.restate_product(cs.x, cs.w["W1"])
        words, scale = R.restate_stored(prod)
        mx = np.abs(prod).max(axis=1)
        assert (scale[mx > 0] != (mx / 2147483000.0)[mx > 0]).any()
        assert (scale[mx == 0] == 1.0).all() and not words[mx == 0].any()
        assert np.abs(words.astype(np.int64)).max() <= 2147483001
        assert (np.abs(words * scale[:, None] - prod) <= 0.5 * scale[:, None] * (1 + 2.0 ** -50)).all()

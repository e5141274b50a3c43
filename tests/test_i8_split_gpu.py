"""The dense fp64 product S1d = X W1 of `delta` (launch_dense_s1d, lt_fp64.hip) on both of its routes, looked at DIRECTLY -- the rows
lt_baseline_refresh_rows_fp64 forms and the arrays a `delta` call leaves (fp64_arrays) -- not through scores rounded to fp32.

  * "i8_split" = 1 (lt_i8_split.hip.h): integer arithmetic with one rounding per K slice, restated exactly in numpy
    (tests/i8_split_restate.py): every comparison is bit for bit;
  * "i8_split" = 0: the f64 matrix cores, whose summation order is not restated: |got - exact| <= (F + splits) 2^-53 |X| |W1| entry
    by entry (the product of two fp32 values is exact in fp64; any order of F additions and the slab sums obeys it), splits <= 64.

Inputs: gaussian features and gcn_weights with rows and columns planted at the edges of the fixed point (i8_split_restate.plant_edges:
zeros, -0.0, all mantissa ones, digit bytes at -128 / 127 with carries, rint ties, the exponent clamp at 1e-30, 2^40 next to ordinary
values).  Left out: fp32 denormals (the compiler's denormal mode is not for this test to pin) and non-finite values (engine refuses
them)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import i8_split_restate as R
from test_fp64_row_trips_gpu import knobs

pytestmark = pytest.mark.gpu
DELTA = 1e-4
I8 = dict(feature_delta=0, aggregate_first=0, i8_split=1)
F64 = dict(feature_delta=0, aggregate_first=0, i8_split=0)


@functools.lru_cache(maxsize=None)
def _graph(n):
    from linkteller_amd import graph, synth
    a_hat = graph.first_order_gcn(synth.erdos_renyi_graph(n, 4 * n, seed=3))
    return a_hat, graph.HipGraph(a_hat)


def _baseline(cs, dev):
    """A baseline on the matrix-core route (set the knobs first) with the fp64 product formed once; the weights' device tensors."""
    from linkteller_amd import engine
    par = [torch.tensor(cs.w[k]).to(dev) for k in ("W1", "b1", "W2", "b2")]
    base = engine.Baseline(_graph(cs.n)[1], torch.tensor(cs.x).to(dev), *par).enable_fp64()
    assert base.fp64_route() == 0
    return base, par


def _rows(base, a, b):
    """Rows [a, b) of the product as lt_baseline_refresh_rows_fp64 forms them: [b - a, Hp] float64 (the buffer is NaN before)."""
    from linkteller_amd import _lib, engine
    hp = (base.h + 3) // 4 * 4
    out = torch.full((b - a, hp), float("nan"), dtype=torch.float64, device=base.x.device)
    _lib.check(_lib.lib().lt_baseline_refresh_rows_fp64(base._h, a, b, out.data_ptr(), engine._stream()), "rows_fp64")
    return out.cpu().numpy()


def _ranges(n):
    """All rows of a small product; of a large one a first tile, a range across a tile boundary and the last 100 rows."""
    return [(0, n)] if n < 1000 else [(0, 64), (1000, 1100), (n - 100, n)]


def _same_bits(got, want, what):
    assert got.shape == want.shape
    bad = got != want
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} values differ from the restated bits, first at {tuple(np.argwhere(bad)[0])}: "
                           f"{got[bad][0]!r} against {want[bad][0]!r}")


# ---- the int8 split ---------------------------------------------------------------------------------------------------------------
# (256, 256, 64): the smallest admitted, exact tiles, one slice.  (257, 257, 192): one live row in the last tile, rows of odd stride
# (AV = 1), a slice of one step holding one live column, a half-filled column block.  (319, 258, 128): AV = 2.  (301, 544, 256): three
# slices.  (301, 1400, 64): six -- the slab sum's unrolled group of four plus a remainder.  (5441, 544, 256): 9 steps per slice, the
# exponent scan's second group of 8 holds one.  (16449, 288, 256): more than 512 tiles, one slice of 9 steps.
@pytest.mark.parametrize("n,f,h", R.SHAPES)
def test_int8_rows_are_the_restated_bits(gpu, n, f, h):
    """The rows as formed, behind a refresh with changed weights, and behind a second refresh: the restated bits each time."""
    cs = R.case(n, f, h)
    with knobs(**I8):
        base, par = _baseline(cs, gpu)
        for a, b in _ranges(n):
            got = _rows(base, a, b)
            assert got.shape[1] == h        # (H % 64 == 0 on this route: no pad columns)
            _same_bits(got, R.restate_product(cs.x[a:b], cs.w["W1"], n), f"rows [{a}, {b})")
        par[0].mul_(0.3)       # smaller weights: an exponent word left over from the old ones would win k_i8_w_max's atomicMax
        w1 = par[0].cpu().numpy()
        for again in range(2):
            base.refresh()
            for a, b in _ranges(n)[-1:]:
                _same_bits(_rows(base, a, b), R.restate_product(cs.x[a:b], w1, n), f"refresh {again + 1}, rows [{a}, {b})")
        torch.cuda.synchronize()


@pytest.mark.parametrize("n,f,h,cuts", [(257, 257, 192, [0, 77, 130, 256, 257]), (319, 258, 128, [0, 77, 131, 201, 319])])
def test_int8_rows_formed_in_ranges_keep_their_bits(gpu, n, f, h, cuts):
    """Row ranges cut at rows that are no multiples of 64 (what a rank of a sharded refresh forms), odd first rows among them, a
    range of one row: the bits of the whole product."""
    cs = R.case(n, f, h)
    with knobs(**I8):
        base, _ = _baseline(cs, gpu)
        whole = _rows(base, 0, n)
        parts = np.concatenate([_rows(base, a, b) for a, b in zip(cuts[:-1], cuts[1:])])
        torch.cuda.synchronize()
    _same_bits(whole, R.restate_product(cs.x, cs.w["W1"]), "whole product")
    _same_bits(parts, whole, "ranges")


def _preact_check(cs, a, stored_rows, fp32):
    """The pre-activation against A_hat (stored rows) + b1 (np.longdouble: the reference adds no error of its own), each entry within
    2^-23 |z| where it is stored as fp32, plus (entries of the row + 1) 2^-53 (|A_hat| |stored| + |b1|): the textbook bound of an
    fp64 chain of that many additions."""
    av = sp.csr_matrix(_graph(cs.n)[0]).astype(np.float32).astype(np.float64)
    dense = av.toarray().astype(np.longdouble)
    b1 = cs.w["b1"].astype(np.longdouble)[None, :]
    z = (dense @ stored_rows.astype(np.longdouble) + b1).astype(np.float64)
    mag = (np.abs(dense) @ np.abs(stored_rows).astype(np.longdouble) + np.abs(b1)).astype(np.float64)
    entries = np.diff(av.indptr).reshape(-1, 1)
    bound = (entries + 1) * 2.0 ** -53 * mag + (2.0 ** -23 * np.abs(z) if fp32 else 0.0)
    pre = a["preact"].cpu().numpy()
    assert pre.dtype == (np.float32 if fp32 else np.float64)
    assert not pre[:, cs.h:].any()
    err = np.abs(pre[:, :cs.h].astype(np.float64) - z)
    print(f"pre-activation: largest error {np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max():.3g} of its bound")
    assert (err <= bound).all()


@pytest.mark.parametrize("s1_f32", [1, 0])
@pytest.mark.parametrize("n,f,h", [(257, 257, 192), (301, 1400, 64), (256, 256, 64)])
def test_int8_stored_form(gpu, n, f, h, s1_f32):
    """One `delta` call over all nodes, then the arrays as stored: int32 words and scales that equal the restated 32-bit storage
    (k_sum_slabs_f64_q; one slice: k_quant_rows_f64), with "s1_f32" = 0 the restated fp64 product; the pre-activation formed from
    them.  Again behind a refresh with SMALLER weights: where k_sum_slabs_f64_q was to clear the exponent words for the next refresh
    (i8_ew_clean), a word it left would carry the old, larger exponent into every digit."""
    cs = R.case(n, f, h)
    nodes = np.arange(n, dtype=np.int64)
    with knobs(**I8, s1_f32=s1_f32, z_on_demand=0):
        base, par = _baseline(cs, gpu)
        w1 = cs.w["W1"]
        for step in range(2):
            scores = base.influence_rows(nodes, nodes, DELTA, "delta")
            a = base.fp64_arrays()
            torch.cuda.synchronize()
            assert torch.isfinite(scores).all() and a["valid"].all() and not a["deferred_cref"] and a["cref"] is None
            want = R.restate_product(cs.x, w1)
            if s1_f32:
                assert a["product"].dtype == torch.int32 and a["scales"] is not None
                words, scales = R.restate_stored(want)
                _same_bits(a["scales"].cpu().numpy(), scales, f"scales, step {step}")
                _same_bits(a["product"].cpu().numpy(), words, f"words, step {step}")
                stored = words.astype(np.float64) * scales[:, None]
            else:
                assert a["product"].dtype == torch.float64 and a["scales"] is None
                _same_bits(a["product"].cpu().numpy(), want, f"product, step {step}")
                stored = want
            _preact_check(cs, a, stored, fp32=bool(s1_f32))
            if step == 0:
                par[0].mul_(0.3)
                w1 = par[0].cpu().numpy()
                base.refresh()
        # (the next product starts from the exponent words as the last one left them)
        _same_bits(_rows(base, 0, n), R.restate_product(cs.x, w1), "rows behind the stored form")
        _same_bits(_rows(base, 0, n), R.restate_product(cs.x, w1), "rows, once more")
        torch.cuda.synchronize()


# ---- the f64 matrix cores -----------------------------------------------------------------------------------------------------------
# The paths by fp64_big (n >= 1024 and H % 128 == 0: k_gemm_f64acc_128) and fp64_kslice, worked out from lt_fp64.hip:
#   (301, 16, 64)      k_gemm_f64acc, one slice of 16 (the rows land in the destination; k_quant_rows_f64)
#   (301, 17, 64)      two slices of 16: the second holds one column
#   (301, 100, 130)    seven slices of 16, the last of 4; Hp = 132 != H: the pad columns come from the memset, a column tail in the
#                      third column block, H % 4 != 0: the rows stay fp64
#   (257, 257, 192)    seventeen slices of 16, the last of one column; one live row in the last tile
#   (1100, 40, 128)    k_gemm_f64acc_128, one slice: two full k tiles and a tail of 8; a row tail of 76
#   (1025, 300, 128)   three slices of 112, 112, 76 (the tail path of a slice); one live row in the last tile
#   (1025, 1000, 256)  five slices of 208, the last of 168
F64_SHAPES = [(301, 16, 64), (301, 17, 64), (301, 100, 130), (257, 257, 192), (1100, 40, 128), (1025, 300, 128), (1025, 1000, 256)]


@functools.lru_cache(maxsize=None)
def _exact(n, f, h):
    cs = R.case(n, f, h, i8=False)
    x, w1 = cs.x.astype(np.longdouble), cs.w["W1"].astype(np.longdouble)
    return x @ w1, np.abs(cs.x).astype(np.float64) @ np.abs(cs.w["W1"]).astype(np.float64)


@pytest.mark.parametrize("s1_f32", [1, 0])
@pytest.mark.parametrize("n,f,h", F64_SHAPES)
def test_f64_cores_within_the_bound_of_any_summation_order(gpu, n, f, h, s1_f32):
    """The rows against the exact product (np.longdouble: 64 mantissa bits, its own error 2^-11 of the bound), entry by entry within
    (F + 64) 2^-53 |X| |W1|; pad columns zero; rows formed in ranges carry the bits of the whole product; and the stored form behind a
    `delta` call: with "s1_f32" = 0 the same fp64 rows, else words and scales that are the restated 32-bit storage of those rows
    (so every value is within half a step of its word; H % 4 != 0: the rows stay fp64 either way)."""
    cs = R.case(n, f, h, i8=False)
    exact, mag = _exact(n, f, h)
    hp = (h + 3) // 4 * 4
    nodes = np.arange(0, n, 3, dtype=np.int64)
    with knobs(**F64, s1_f32=s1_f32, z_on_demand=0):
        base, _ = _baseline(cs, gpu)
        whole = _rows(base, 0, n)
        cuts = [0, 77, 131, 256, n]
        parts = np.concatenate([_rows(base, a, b) for a, b in zip(cuts[:-1], cuts[1:])])
        base.refresh()
        base.influence_rows(nodes, nodes, DELTA, "delta")
        a = base.fp64_arrays()
        torch.cuda.synchronize()
    assert whole.shape == (n, hp) and not whole[:, h:].any()
    err = np.abs(whole[:, :h].astype(np.longdouble) - exact).astype(np.float64)
    bound = (f + 64) * 2.0 ** -53 * mag
    print(f"largest error {np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max():.3g} of the bound")
    assert (err <= bound).all()
    _same_bits(parts, whole, "ranges")
    fixed = bool(s1_f32) and h % 4 == 0
    assert (a["scales"] is not None) == fixed
    if fixed:
        words, scales = R.restate_stored(whole)
        got_w, got_s = a["product"].cpu().numpy(), a["scales"].cpu().numpy()
        _same_bits(got_s, scales, "scales")
        back = got_w.astype(np.float64) * got_s[:, None]
        assert (np.abs(back - whole) <= 0.5 * got_s[:, None] + np.spacing(np.abs(whole))).all()
        _same_bits(got_w, words, "words")
    else:
        _same_bits(a["product"].cpu().numpy(), whole, "product as stored")

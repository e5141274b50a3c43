"""The evaluation head over a row list (lt_eval_head_rows; ``engine.eval_head(..., rows=)``) against the existing head applied to
gathered copies -- code from before the list existed -- and against the float64 restatement (validate_restate.py)."""
import numpy as np
import pytest
import torch

import validate_restate as V

pytestmark = pytest.mark.gpu

N = 600
CS = [1, 2, 3, 7, 8]
MS = [1, 255, 256, 257, 513]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return int(t.view(torch.int32).cpu())


def _case(c, seed):
    """Logits [N, c], loss O(1): gaussian rows; every 5th row has tied maxima (the first must win); every 7th row has magnitude
    80 with the maximum on its own label.  Class c - 1 is absent from the labels."""
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((N, c)).astype(np.float32)
    y = rng.randint(0, max(c - 1, 1), N).astype(np.int64)
    if c > 1:
        rows = np.arange(0, N, 5)
        a, b = rng.randint(0, c, rows.size), rng.randint(0, c, rows.size)
        top = z[rows].max(axis=1) + np.float32(0.5)
        z[rows, a] = top
        z[rows, b] = top
    big = np.arange(3, N, 7)
    z[big] = np.float32(-80.0)
    z[big, y[big]] = np.float32(80.0)
    return z, y


def _lists(seed):
    """Shuffled lists of every length in MS (513 < N: no repeats), and one of 513 draws with repeats."""
    rng = np.random.RandomState(seed)
    out = {f"m{m}": rng.permutation(N)[:m].astype(np.int64) for m in MS}
    out["repeats"] = rng.randint(0, 40, 513).astype(np.int64)
    assert np.unique(out["repeats"]).size < 41
    return out


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("c", CS)
def test_list_equals_the_head_on_gathered_copies(c, pad):
    from linkteller_amd import engine
    z, y = _case(c, 10 * c + pad)
    wide = torch.full((N, c + pad), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :c] = _dev(z)
    view, yd = wide[:, :c], _dev(y)
    assert view.stride(0) == c + pad
    for name, rows in _lists(c).items():
        rd = _dev(rows)
        loss, conf = engine.eval_head(view, yd, rows=rd)
        want_loss, want_conf = engine.eval_head(view[rd].contiguous(), yd[rd])            # the head from before the list
        assert _bits(loss) == _bits(want_loss), (name, float(loss), float(want_loss))
        assert torch.equal(conf, want_conf), name
        loss_np, conf_np = engine.eval_head(view, yd, rows=rows)                          # an array, and twice: a pure function
        assert _bits(loss_np) == _bits(loss) and torch.equal(conf_np, conf)
        l64, c64 = V.head(z[rows], y[rows], np.float64)
        l32, _ = V.head(z[rows], y[rows], np.float32)
        got = float(loss.cpu())
        print(f"C={c} ldz={c + pad} {name}: dev {got:.9g} l64 {l64:.9g} |dev-l64| {abs(got - l64):.3g} |l32-l64| {abs(l32 - l64):.3g}")
        assert np.array_equal(conf.cpu().numpy().astype(np.int64), c64) and int(conf.sum()) == rows.size
        assert abs(got - l64) <= 2 * abs(l32 - l64) + 1e-5
    full_loss, full_conf = engine.eval_head(view, yd, rows=torch.arange(N))
    head_loss, head_conf = engine.eval_head(view, yd)
    assert _bits(full_loss) == _bits(head_loss) and torch.equal(full_conf, head_conf)


def _raw(z, ldz, y, n, c, rows, m, loss, conf, n_bad, ws, nbytes):
    from linkteller_amd import _lib
    return _lib.lib().lt_eval_head_rows(z.data_ptr(), ldz, y.data_ptr(), n, c, None if rows is None else rows.data_ptr(), m,
                                        loss.data_ptr(), conf.data_ptr(), None if n_bad is None else n_bad.data_ptr(),
                                        ws.data_ptr(), nbytes, None)


def test_ids_out_of_range_are_skipped_and_counted():
    from linkteller_amd import engine
    c = 7
    z, y = _case(c, 5)
    zd, yd = _dev(z), _dev(y).to(torch.int32)
    rows = np.random.RandomState(1).permutation(N)[:300].astype(np.int64)
    bad = rows.copy()
    bad[[0, 150, 299]] = [-1, N, 2 ** 30]
    good = np.delete(rows, [0, 150, 299])
    loss, conf = torch.zeros((), device="cuda"), torch.zeros((c, c), dtype=torch.int32, device="cuda")
    n_bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    assert _raw(zd, c, yd, N, c, _dev(bad.astype(np.int32)), 300, loss, conf, n_bad, ws, ws.numel()) == 0
    assert int(n_bad.cpu()) == 3
    _, want_conf = engine.eval_head(zd, yd, rows=good)
    assert torch.equal(conf, want_conf) and int(conf.sum()) == 297                       # the other cells are unchanged
    # the divisor is m: a skipped entry adds 0 to its block's tree, so the loss is the 297 row losses' sum / 300.  Bound: the head's
    # own against the restatement (2 |l32 - l64| + 1e-5), the fp32 restatement taken over the 297 rows and rescaled
    l297, l297_32 = V.head(z[good], y[good], np.float64)[0], V.head(z[good], y[good], np.float32)[0]
    l64 = l297 * 297 / 300
    got = float(loss.cpu())
    print(f"loss {got:.9g}, sum/300 in fp64 {l64:.9g}, sum/297 {l297:.9g}, |l32-l64| {abs(l297_32 - l297):.3g}")
    assert abs(got - l64) <= 2 * abs(l297_32 - l297) + 1e-5
    assert abs(l297 - l64) > 1e-3                        # the two divisors are far apart at this bound
    assert _raw(zd, c, yd, N, c, _dev(bad.astype(np.int32)), 300, loss, conf, None, ws, ws.numel()) == 0     # n_bad may be NULL
    assert torch.equal(conf, want_conf)
    assert _raw(zd, c, yd, N, c, _dev(rows.astype(np.int32)), 300, loss, conf, n_bad, ws, ws.numel()) == 0
    assert int(n_bad.cpu()) == 0                                                          # rewritten by every call
    for rows_arg in (bad, torch.from_numpy(bad), _dev(bad), _dev(bad.astype(np.int32))):
        with pytest.raises(IndexError):
            engine.eval_head(zd, yd, rows=rows_arg)
    with pytest.raises(TypeError):
        engine.eval_head(zd, yd, rows=np.array([0.0, 1.0]))


def test_bad_arguments_write_nothing():
    from linkteller_amd import _lib
    h = _lib.lib()
    c = 2
    z, y = torch.zeros((4, c), device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    rows = torch.zeros(4, dtype=torch.int32, device="cuda")
    loss, conf = torch.full((), 5.0, device="cuda"), torch.full((c, c), 9, dtype=torch.int32, device="cuda")
    n_bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    ws = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
    INVALID = -1
    assert _raw(z, c, y, 4, c, rows, 0, loss, conf, n_bad, ws, 64) == INVALID             # m <= 0
    assert _raw(z, c, y, 4, c, rows, -3, loss, conf, n_bad, ws, 64) == INVALID
    assert _raw(z, c, y, 0, c, rows, 4, loss, conf, n_bad, ws, 64) == INVALID             # n <= 0
    assert _raw(z, 9, y, 4, 9, rows, 4, loss, conf, n_bad, ws, 64) == INVALID             # C outside [1, 8]
    assert _raw(z, 0, y, 4, 0, rows, 4, loss, conf, n_bad, ws, 64) == INVALID
    assert _raw(z, 1, y, 4, c, rows, 4, loss, conf, n_bad, ws, 64) == INVALID             # ldz < C
    assert _raw(z, c, y, 4, c, None, 4, loss, conf, n_bad, ws, 64) == INVALID             # a NULL pointer
    assert h.lt_eval_head_rows(None, c, y.data_ptr(), 4, c, rows.data_ptr(), 4, loss.data_ptr(), conf.data_ptr(), None,
                               ws.data_ptr(), 64, None) == INVALID
    assert "lt_eval_head_rows" in h.lt_last_error().decode()
    assert _raw(z, c, y, 4, c, rows, 4, loss, conf, n_bad, ws, 8) == _lib.LT_ERR_WORKSPACE
    assert h.lt_eval_head_rows(z.data_ptr(), c, y.data_ptr(), 4, c, rows.data_ptr(), 4, loss.data_ptr(), conf.data_ptr(), None,
                               None, 64, None) == _lib.LT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert float(loss) == 5.0 and bool((conf == 9).all()) and int(n_bad) == 77 and bool((ws == 0xAB).all())
    # the workspace follows the list's length, not the matrix': as lt_eval_head's at n = m
    assert h.lt_eval_head_rows_workspace_bytes(4, 2) == 4 * (1 + 4) == h.lt_eval_head_workspace_bytes(4, 2)
    assert h.lt_eval_head_rows_workspace_bytes(65537, 8) == 257 * 65 * 4
    assert h.lt_eval_head_rows_workspace_bytes(0, 2) == 0 and h.lt_eval_head_rows_workspace_bytes(4, 9) == 0
    assert _raw(z, c, y, 4, c, rows, 4, loss, conf, n_bad, ws, 64) == 0                   # and the same arguments, valid, run
    assert int(n_bad.cpu()) == 0 and int(conf.sum()) == 4

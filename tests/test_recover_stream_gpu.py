"""The streaming selector (lt_top_stream_*, engine.TopPairsStream) against ``engine.top_pairs_lower`` on the assembled matrix
and against the numpy restatement of tests/test_recover_gpu.py.  Equality is exact everywhere: index bytes, score bits and the
four info words -- whatever the cut into pushes, the slack, or the compactions that fired on the way."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [2, 3, 64, 65, 257, 700]
CLASSES = ["zeros93", "ties", "signs", "allzero", "increasing", "decreasing"]


def _values(cls, total, rng):
    if cls == "zeros93":        # 93 % exact +0, distinct positives elsewhere
        v = np.zeros(total, dtype=np.float32)
        pos = rng.random_sample(total) < 0.07
        if total > 1 and not pos.any():
            pos[rng.randint(total)] = True
        k = int(pos.sum())
        v[pos] = rng.permutation(np.arange(1, k + 1)).astype(np.float32) / np.float32(8.0)
        return v
    if cls == "ties":           # four values, heavy ties everywhere
        return np.array([0.5, 1.0, 1.5, 2.0], dtype=np.float32)[rng.randint(4, size=total)]
    if cls == "signs":          # mixed signs, -0.0, subnormals, +-inf
        pool = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 3e-39, 1.5, 1.5, -2.0, 3.25, 3.25, -np.inf, np.inf], dtype=np.float32)
        prob = np.array([20, 20, 8, 8, 8, 8, 6, 6, 6, 4, 4, 1, 1], dtype=np.float64)
        return pool[rng.choice(pool.size, size=total, p=prob / prob.sum())]
    if cls == "allzero":
        return np.zeros(total, dtype=np.float32)
    ramp = np.arange(1, total + 1, dtype=np.float32)          # (total <= 244 650 < 2^24: distinct in fp32)
    return ramp if cls == "increasing" else ramp[::-1].copy()


def _ranked(M):
    n = M.shape[0]
    ii, jj = np.tril_indices(n, -1)
    flat = ii.astype(np.int64) * n + jj
    v = M[ii, jj] + np.float32(0)
    return flat, v, np.lexsort((flat, -v.astype(np.float64)))


def _expect(flat, v, order, m):
    thr = v[order[m - 1]]
    above = int((v > thr).sum())
    return np.sort(flat[order[:m]]), thr, above, m - above, int((v == thr).sum())


def _ms(cls, values, total):
    nz = int((values != 0).sum())
    ms = {1, 2, nz - 1, nz, nz + 1, total - 1, total}
    if cls == "ties":           # cuts inside the tied groups of 2.0 and of 1.5
        c2, c15 = int((values == 2.0).sum()), int((values == 1.5).sum())
        ms |= {c2 // 2, c2 + c15 // 2}
    if cls == "zeros93":
        ms |= {nz + (total - nz) // 2}
    return sorted(mm for mm in ms if 1 <= mm <= total)


def _splits(n, how):
    """Row ranges [b, e) of one pass over the n rows."""
    if how == "irregular":
        sizes, out, b, k = [3, 1, 11, 2, 29, 5, 64, 1, 17], [], 0, 0
        while b < n:
            e = min(n, b + sizes[k % len(sizes)])
            out.append((b, e))
            b, k = e, k + 1
        return out
    return [(b, min(n, b + how)) for b in range(0, n, how)]


# (row stride, rows per push, slack, columns handed over): every value of every dimension; each m of a case runs them all
CONFIGS = [("n", 1, "min", "all"), ("n+13", 7, "default", "all"), ("n", 64, "min", "tri"), ("n+13", "n", "min", "all"),
           ("n", "irregular", "min", "all"), ("n+13", 1, "default", "tri"), ("n", 7, "min", "all"), ("n+13", 64, "default", "all"),
           ("n", "n", "default", "all"), ("n+13", "irregular", "min", "tri")]


def _run(engine, dev, n, m, rows_per_push, slack, cols, sel=None):
    how = n if rows_per_push == "n" else rows_per_push
    own = sel is None
    if own:
        sel = engine.TopPairsStream(n, m, n, slack_cells=2 * (n - 1) if slack == "min" else 0)
    for b, e in _splits(n, how):
        sel.push(dev[b:e, :max(e - 1, 1)] if cols == "tri" else dev[b:e, :n], b)
    out = sel.finish()
    stats = sel.stats()
    if own:
        sel.close()
    return out, stats


def _assert_same(got, want, tag):
    assert torch.equal(got[0], want[0]), tag
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), tag
    assert torch.equal(got[2]["raw"], want[2]["raw"]), tag


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("n", NS)
def test_stream_equals_one_shot(gpu, n, cls):
    from linkteller_amd import engine
    total = n * (n - 1) // 2
    rng = np.random.RandomState(77 * n + len(cls))
    values = _values(cls, total, rng)
    ii, jj = np.tril_indices(n, -1)
    devs = {}
    for name, lds in (("n", n), ("n+13", n + 13)):      # a view into a larger buffer: +inf wherever nothing may be read
        host = np.full((n + 5, lds), np.inf, dtype=np.float32)
        host[ii, jj] = values
        devs[name] = torch.from_numpy(host).to(gpu)
    M = devs["n"][:n, :n].cpu().numpy()
    ranked = _ranked(M)
    for k, m in enumerate(_ms(cls, values, total)):
        want = engine.top_pairs_lower(devs["n"][:n, :n], m)
        exp_idx, thr, above, tied_taken, tied_total = _expect(*ranked, m)
        assert np.array_equal(want[0].cpu().numpy(), exp_idx)
        for lds, rpp, slack, cols in CONFIGS:
            tag = f"n={n} class={cls} m={m} lds={lds} rows/push={rpp} slack={slack} cols={cols}"
            got, stats = _run(engine, devs[lds], n, m, rpp, slack, cols)
            _assert_same(got, want, tag)
            raw = got[2]["raw"].cpu().numpy()
            assert got[0].shape == (m,) and np.array_equal(got[0].cpu().numpy(), exp_idx), tag
            assert np.array_equal(got[1].cpu().numpy().view(np.int32), M.reshape(-1)[exp_idx].view(np.int32)), tag
            assert int(raw[0]) == int(np.array([thr], dtype=np.float32).view(np.uint32)[0]), tag
            assert (int(raw[1]), int(raw[2]), int(raw[3])) == (above, tied_taken, tied_total), tag
            assert stats["seen"] == total and stats["held"] == m, tag


@pytest.mark.parametrize("cls", ["zeros93", "ties", "increasing", "decreasing"])
def test_every_cut_and_slack_at_one_shape(gpu, cls):
    """The full cross of rows per push x slack x row stride at n = 257 for three m; the handle is reused through reset()."""
    from linkteller_amd import engine
    n = 257
    total = n * (n - 1) // 2
    values = _values(cls, total, np.random.RandomState(5))
    ii, jj = np.tril_indices(n, -1)
    devs = {}
    for name, lds in (("n", n), ("n+13", n + 13)):
        host = np.full((n, lds), np.inf, dtype=np.float32)
        host[ii, jj] = values
        devs[name] = torch.from_numpy(host).to(gpu)
    nz = int((values != 0).sum())
    for m in sorted({2, min(nz, total) - 1, total - 1}):
        want = engine.top_pairs_lower(devs["n"][:, :n], m)
        for slack in ("min", "default"):
            sel = engine.TopPairsStream(n, m, n, slack_cells=2 * (n - 1) if slack == "min" else 0)
            for lds in ("n", "n+13"):
                for rpp in (1, 7, 64, "n", "irregular"):
                    got, _ = _run(engine, devs[lds], n, m, rpp, slack, "all", sel=sel)
                    _assert_same(got, want, f"class={cls} m={m} slack={slack} lds={lds} rows/push={rpp}")
                    sel.reset()
            sel.close()


def test_compactions_fire_where_they_must(gpu):
    from linkteller_amd import engine
    n = 257
    total = n * (n - 1) // 2
    ii, jj = np.tril_indices(n, -1)
    for cls, m in (("increasing", 100), ("zeros93", 500)):
        host = np.full((n, n), np.inf, dtype=np.float32)
        host[ii, jj] = _values(cls, total, np.random.RandomState(9))
        dev = torch.from_numpy(host).to(gpu)
        want = engine.top_pairs_lower(dev, m)
        # minimum slack: the buffers hold m + 512 entries and fire beyond m + 256.  On the increasing ramp every cell qualifies, so
        # the chain fires about once per slab: in front of first slabs of a push (between pushes) and of later ones (inside a
        # push).  The zero-heavy class appends its ~7 % positives only once a threshold stands: a handful of firings, wherever
        # the 257th new candidate happens to fall
        got, stats = _run(engine, dev, n, m, 7, "min", "all")
        _assert_same(got, want, cls)
        if cls == "increasing":
            assert stats["fired_between"] > 0 and stats["fired_inside"] > 0, stats
        assert stats["fired_between"] + stats["fired_inside"] > 0, stats
        # slabs are whole rows of at most slack / 2 = 256 cells, cut anew in every push (the short first rows share slabs)
        slabs = 0
        for b, e in _splits(n, 7):
            a = max(b, 1)
            while a < e:
                cells = 0
                while a < e and cells + a <= n - 1:
                    cells, a = cells + a, a + 1
                slabs += 1
        assert stats["slabs"] == slabs and n // 7 < slabs < n - 1
        # rows one at a time: every slab is a push's first
        got, stats = _run(engine, dev, n, m, 1, "min", "all")
        _assert_same(got, want, cls)
        assert stats["fired_between"] > 0 and stats["fired_inside"] == 0, stats
        # default slack: the whole triangle (32 896 cells) is below m + 2^21: nothing fires, whatever the values
        got, stats = _run(engine, dev, n, m, 7, "default", "all")
        _assert_same(got, want, cls)
        assert stats["fired_between"] + stats["fired_inside"] == 0, stats


def test_two_runs_identical_and_reset_takes_a_second_matrix(gpu):
    from linkteller_amd import engine
    n, m = 129, 700
    total = n * (n - 1) // 2
    ii, jj = np.tril_indices(n, -1)
    mats = []
    for seed in (1, 2):
        host = np.full((n, n), np.inf, dtype=np.float32)
        host[ii, jj] = _values("zeros93" if seed == 1 else "signs", total, np.random.RandomState(seed))
        mats.append(torch.from_numpy(host).to(gpu))
    sel = engine.TopPairsStream(n, m, 64, slack_cells=2 * (n - 1))
    a, _ = _run(engine, mats[0], n, m, 7, "min", "all", sel=sel)
    b, _ = _run(engine, mats[0], n, m, 7, "min", "all")
    _assert_same(a, b, "two runs")
    a_bytes = (a[0].cpu().numpy().tobytes(), a[1].cpu().numpy().tobytes(), a[2]["raw"].cpu().numpy().tobytes())
    sel.reset()
    c, stats = _run(engine, mats[1], n, m, 64, "min", "all", sel=sel)
    _assert_same(c, engine.top_pairs_lower(mats[1], m), "second matrix")
    assert stats["seen"] == total
    assert a_bytes == (a[0].cpu().numpy().tobytes(), a[1].cpu().numpy().tobytes(), a[2]["raw"].cpu().numpy().tobytes())
    sel.close()
    with pytest.raises(RuntimeError):
        sel.reset()                                  # a closed handle says so


def test_refusals_leave_the_handle_usable(gpu):
    from linkteller_amd import _lib, engine
    n, m = 65, 40
    total = n * (n - 1) // 2
    ii, jj = np.tril_indices(n, -1)
    host = np.full((n, n), np.inf, dtype=np.float32)
    host[ii, jj] = _values("zeros93", total, np.random.RandomState(3))
    dev = torch.from_numpy(host).to(gpu)
    err = _lib.LinkTellerHipError
    with pytest.raises(ValueError):
        engine.TopPairsStream(n, 0, 16)
    with pytest.raises(ValueError):
        engine.TopPairsStream(n, total + 1, 16)
    with pytest.raises(ValueError):
        engine.TopPairsStream(n, m, 16, slack_cells=2 * (n - 1) - 1)
    h = C.c_void_p()
    lib = _lib.lib()
    assert lib.lt_top_stream_create(n, total + 1, 16, 0, C.byref(h)) == -1 and b"outside" in lib.lt_last_error()
    assert lib.lt_top_stream_create(n, m, 16, 2 * (n - 1) - 1, C.byref(h)) == -1 and b"slack_cells" in lib.lt_last_error()
    assert lib.lt_top_stream_create(1, 1, 16, 0, C.byref(h)) == -1 and h.value is None

    sel = engine.TopPairsStream(n, m, 16, slack_cells=2 * (n - 1))
    with pytest.raises(err, match="already|pushed"):
        sel.finish()                                 # nothing pushed yet
    with pytest.raises(err, match="next row"):
        sel.push(dev[5:10, :n], 5)                   # does not start at row 0
    sel.push(dev[0:10, :n], 0)
    with pytest.raises(err, match="next row"):
        sel.push(dev[5:15, :n], 5)                   # overlaps
    with pytest.raises(err, match="next row"):
        sel.push(dev[12:20, :n], 12)                 # leaves a gap
    with pytest.raises(err, match="max_push_rows"):
        sel.push(dev[10:27, :n], 10)                 # 17 rows > 16
    with pytest.raises(ValueError):
        sel.push(dev[10:20, :18], 10)                # 18 columns, 19 are read
    assert lib.lt_top_stream_push(sel._h, dev.data_ptr(), 18, 10, 10, None) == -1 and b"lds" in lib.lt_last_error()
    with pytest.raises(err, match="pushed"):
        sel.finish()                                 # before completion
    # the handle took none of that: the rest of the rows, then the answer of the one-shot route
    for b in range(10, n, 16):
        sel.push(dev[b:min(n, b + 16), :n], b)
    with pytest.raises(err, match="next row|beyond"):
        sel.push(dev[0:1, :n], n)                    # past the last row
    got = sel.finish()
    _assert_same(got, engine.top_pairs_lower(dev, m), "after the refusals")
    with pytest.raises(err, match="finished"):
        sel.finish()
    with pytest.raises(err, match="finished"):
        sel.push(dev[0:1, :n], 0)
    sel.reset()
    got, _ = _run(engine, dev, n, m, 16, "min", "all", sel=sel)
    _assert_same(got, engine.top_pairs_lower(dev, m), "after reset")
    sel.close()


def test_device_bytes_follow_the_header_formula(gpu):
    """25600 + A(8 cap) + A(16 cap) + 4 A(4 m) + A(1024 nblk), A = round up to 256 (include/linkteller_hip.h)."""
    from linkteller_amd import engine

    def formula(n, m, slack):
        slack = slack or max(2 * (n - 1), 1 << 22)
        cap = m + slack
        r = 4
        while -(-m // (256 * r)) > 4096:
            r *= 2
        nblk = -(-m // (256 * r))
        A = lambda x: -(-x // 256) * 256
        return 25600 + A(8 * cap) + A(16 * cap) + 4 * A(4 * m) + A(1024 * nblk)

    for n, m, slack in ((65, 40, 128), (700, 1000, 0), (200_000, 1_000_000, 0), (200_000, 1_000_000, 399_998)):
        sel = engine.TopPairsStream(n, m, 1024, slack_cells=slack)      # create / destroy, nothing pushed
        assert sel.device_bytes == formula(n, m, slack), (n, m, slack)
        sel.close()
    # a whole graph of 200 000 nodes at a million pairs: ~0.14 GB at the default slack against the 160 GB of the n x n matrix
    assert formula(200_000, 1_000_000, 0) * 1000 < 200_000 ** 2 * 4

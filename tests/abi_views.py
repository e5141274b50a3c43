"""Operands as a foreign caller of the C ABI hands them over: a matrix that is a window of something larger.

include/linkteller_hip.h: "All matrices are row-major fp32 with an explicit leading dimension in elements", borrowed
``data_ptr()``s of tensors the library did not allocate.  ``strided`` places a host matrix at element offset ``off`` with row
stride ``ld`` inside a 1-D buffer whose every other word holds a recognisable bit pattern -- a quiet NaN for inputs (a pad
value that reaches arithmetic shows as NaN in the result), any sentinel for outputs -- ``pads_untouched`` compares those
words as integers afterwards, ``body`` reads the window back.  The ctypes wrappers below mirror the calls
``engine.Baseline`` / ``engine.Baseline3`` make, but take ``View``s (pointer + leading dimension) instead of contiguous
tensors, and assert in Python the alignment every operand is MEANT to have: a change of the allocator's alignment then
fails the test instead of silently turning one case into another.

A plain module (no fixtures, not a conftest); it runs on CPU tensors too (tests/test_abi_layout_cpu.py).
"""
import ctypes as C
import weakref

import numpy as np
import torch

NAN32_BITS = 0x7FC0DEAD                 # quiet NaN, payload 0x0dead
NAN64_BITS = 0x7FF80000DEADDEAD         # quiet NaN, the same idea in 64 bits
TAIL = 8                                # elements behind the last row
BASE_ALIGN = 64                         # what a fresh torch allocation is at least aligned to, host and device (bytes)

_INT = {torch.float32: torch.int32, torch.float64: torch.int64}
_NPINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def _signed(bits, itemsize):
    bits = int(bits) & ((1 << (8 * itemsize)) - 1)
    return bits - (1 << (8 * itemsize)) if bits >> (8 * itemsize - 1) else bits


def fill_bits(dtype, fill=None):
    """The bit pattern (unsigned int) a pad word of ``dtype`` holds: the NaN above, or the bits of the value ``fill``."""
    dt = np.dtype(dtype)
    if fill is None:
        return NAN32_BITS if dt == np.float32 else NAN64_BITS
    return int(np.array([fill], dtype=dt).view(_NPINT[dt])[0])


def buffer_len(rows, ld, off):
    return off + rows * ld + TAIL


def expected_align16(off, itemsize=4):
    """``ptr % 16`` of an operand placed ``off`` elements into a buffer whose base is at least 16-byte aligned."""
    return (off * itemsize) % 16


def strided(mat, ld, off=0, fill=None, device=None):
    """Host float32 / float64 ``mat`` [rows, cols] -> ``(buf, ptr)``: ``buf`` is a 1-D tensor of ``off + rows * ld + 8``
    elements on ``device`` (default cuda:0) filled with ``fill`` (default: the NaN pattern), the matrix copied in at element
    offset ``off`` with row stride ``ld``; ``ptr = buf.data_ptr() + itemsize * off``."""
    mat = np.ascontiguousarray(mat)
    assert mat.ndim == 2 and mat.dtype in (np.float32, np.float64), (mat.shape, mat.dtype)
    rows, cols = mat.shape
    assert ld >= cols and off >= 0, (ld, cols, off)
    dev = torch.device("cuda:0") if device is None else torch.device(device)
    tdt = torch.float32 if mat.dtype == np.float32 else torch.float64
    isz = mat.dtype.itemsize
    host = torch.empty(buffer_len(rows, ld, off), dtype=tdt)
    host.view(_INT[tdt]).fill_(_signed(fill_bits(mat.dtype, fill), isz))
    if rows and cols:
        torch.as_strided(host, (rows, cols), (ld, 1), off).copy_(torch.from_numpy(mat))
    buf = host.to(dev) if dev.type != "cpu" else host
    assert buf.data_ptr() % BASE_ALIGN == 0, f"allocation base {buf.data_ptr():#x} is not {BASE_ALIGN}-byte aligned"
    ptr = buf.data_ptr() + isz * off
    assert ptr % 16 == expected_align16(off, isz)
    return buf, ptr


def _pad_mask(n, rows, cols, ld, off):
    mask = np.ones(n, dtype=bool)
    if rows and cols:
        idx = off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
        mask[idx.reshape(-1)] = False
    return mask


def touched_pads(buf, rows, cols, ld, off, fill=None):
    """Element indices of ``buf`` outside the [rows, cols] window (lead-in, the pad columns between rows, the tail) whose
    BITS differ from the fill pattern.  Integer comparison: a NaN never equals a NaN by value."""
    assert buf.numel() == buffer_len(rows, ld, off), (buf.numel(), rows, ld, off)
    words = buf.detach().cpu().view(_INT[buf.dtype]).numpy()
    want = _signed(fill_bits(np.float32 if buf.dtype == torch.float32 else np.float64, fill), buf.element_size())
    return np.flatnonzero(_pad_mask(words.size, rows, cols, ld, off) & (words != want))


def pads_untouched(buf, rows, cols, ld, off, fill=None):
    return touched_pads(buf, rows, cols, ld, off, fill).size == 0


def body(buf, rows, cols, ld, off):
    """The [rows, cols] window as a contiguous host array."""
    host = buf.detach().cpu()
    return torch.as_strided(host, (rows, cols), (ld, 1), off).contiguous().numpy()


class View:
    """A matrix operand for the wrappers: the buffer, its pointer and its layout; ``off`` fixes the alignment the case is
    about (``assert_aligned`` is called by every wrapper that takes the view)."""

    def __init__(self, mat, ld=None, off=0, fill=None, device=None):
        mat = np.ascontiguousarray(mat)
        if mat.ndim == 1:
            mat = mat.reshape(1, -1)
        self.rows, self.cols = mat.shape
        self.ld = self.cols if ld is None else int(ld)
        self.off = int(off)
        self.fill = fill
        self.itemsize = mat.dtype.itemsize
        self.buf, self.ptr = strided(mat, self.ld, self.off, fill, device)

    @classmethod
    def output(cls, rows, cols, ld=None, off=0, fill=-7.0, dtype=np.float32, device=None):
        """A result buffer: every word, window included, holds the sentinel."""
        return cls(np.full((rows, cols), fill, dtype=dtype), ld, off, fill, device)

    def assert_aligned(self):
        assert self.buf.data_ptr() % BASE_ALIGN == 0
        assert self.ptr == self.buf.data_ptr() + self.itemsize * self.off
        assert self.ptr % 16 == expected_align16(self.off, self.itemsize), (hex(self.ptr), self.off)
        return self.ptr

    def body(self):
        return body(self.buf, self.rows, self.cols, self.ld, self.off)

    def touched_pads(self):
        return touched_pads(self.buf, self.rows, self.cols, self.ld, self.off, self.fill)

    def pads_untouched(self):
        return self.touched_pads().size == 0


# ---- the C ABI with (pointer, leading dimension) operands --------------------------------------------------------------
def _L():
    from linkteller_amd import _lib
    return _lib


def _stream():
    from linkteller_amd import engine
    return engine._stream()


def _nodes(nodes, dev):
    return torch.as_tensor(np.asarray(nodes, dtype=np.int32)).to(dev)


def gemm(a: View, b: View, c: View, m, n, k):
    L = _L()
    L.check(L.lib().lt_gemm_f32(a.assert_aligned(), a.ld, b.assert_aligned(), b.ld, c.assert_aligned(), c.ld, m, n, k, _stream()),
            "lt_gemm_f32")


def spmm(hg, s: View, ncols, bias, relu, out: View):
    """``bias``: a View of one row, or None."""
    L = _L()
    L.check(L.lib().lt_spmm_csr_f32(hg.handle, s.assert_aligned(), s.ld, ncols, None if bias is None else bias.assert_aligned(),
                                    int(bool(relu)), out.assert_aligned(), out.ld, _stream()), "lt_spmm_csr_f32")


def gcn2_forward(hg, x: View, f, w1: View, b1: View, h, w2: View, b2: View, c, logits: View):
    """lt_gcn2_forward; the weights are dense (W1 [F, H], W2 [H, C]: the ABI gives them no leading dimension)."""
    from linkteller_amd import engine
    L = _L()
    assert w1.ld == h and w2.ld == c
    ws = engine._workspace(L.lib().lt_gcn2_workspace_bytes(hg.n, f, h, c), x.buf.device)
    return L.lib().lt_gcn2_forward(hg.handle, x.assert_aligned(), x.ld, f, w1.assert_aligned(), b1.assert_aligned(), h,
                                   w2.assert_aligned(), b2.assert_aligned(), c, logits.assert_aligned(), logits.ld,
                                   ws.data_ptr(), ws.numel(), _stream())


class RawBaseline:
    """lt_baseline_* / lt_influence_* on Views (what ``engine.Baseline`` does with contiguous tensors)."""

    def __init__(self, hg, x: View, f, w1: View, b1: View, h, w2: View, b2: View, c):
        L = _L()
        assert w1.ld == h and w2.ld == c
        self.hg, self.n, self.f, self.h, self.c = hg, hg.n, f, h, c
        self.dev = x.buf.device
        self.keep = (x, w1, b1, w2, b2)          # borrowed by the handle
        hd = C.c_void_p()
        L.check(L.lib().lt_baseline_create(hg.handle, x.assert_aligned(), x.ld, f, w1.assert_aligned(), b1.assert_aligned(), h,
                                           w2.assert_aligned(), b2.assert_aligned(), c, _stream(), C.byref(hd)), "lt_baseline_create")
        self._h = hd
        self._finalizer = weakref.finalize(self, L.lib().lt_baseline_destroy, hd)

    def destroy(self):
        torch.cuda.synchronize()
        self._finalizer()

    def enable_fp64(self):
        L = _L()
        L.check(L.lib().lt_baseline_enable_fp64(self._h, _stream()), "lt_baseline_enable_fp64")
        return self

    def fp64_route(self):
        L = _L()
        r = C.c_int32(-1)
        L.check(L.lib().lt_baseline_fp64_route(self._h, C.byref(r)), "lt_baseline_fp64_route")
        return r.value

    def refresh(self):
        L = _L()
        L.check(L.lib().lt_baseline_refresh(self._h, _stream()), "lt_baseline_refresh")

    def logits(self):
        L = _L()
        out = torch.empty((self.n, self.c), dtype=torch.float32, device=self.dev)
        L.check(L.lib().lt_baseline_logits(self._h, out.data_ptr(), _stream()), "lt_baseline_logits")
        return out.cpu().numpy()

    def _ws(self, npb, nob, mode):
        from linkteller_amd import engine
        L = _L()
        return engine._workspace(L.lib().lt_influence_workspace_bytes(self._h, npb, nob, mode), self.dev)

    def rows(self, probes, obs, delta, mode, out: View):
        """lt_influence_rows into ``out`` ([n_probe, n_obs] window, ld = out.ld)."""
        L = _L()
        m = L.MODES[mode]
        p, o = _nodes(probes, self.dev), _nodes(obs, self.dev)
        assert (out.rows, out.cols) == (p.numel(), o.numel())
        ws = self._ws(p.numel(), o.numel(), m)
        L.check(L.lib().lt_influence_rows(self._h, p.data_ptr(), p.numel(), o.data_ptr(), o.numel(), float(delta), m,
                                          out.assert_aligned(), out.ld, ws.data_ptr(), ws.numel(), _stream()), "lt_influence_rows")
        torch.cuda.synchronize()
        return out.body()

    def rows_vec(self, probes, obs, delta, mode, out: View, vec: View):
        """lt_influence_rows_vec: ``vec`` is a [n_probe, n_obs * C] window with ld = out.ld * C (the header indexes it with ldo)."""
        L = _L()
        m = L.MODES[mode]
        p, o = _nodes(probes, self.dev), _nodes(obs, self.dev)
        assert (out.rows, out.cols) == (p.numel(), o.numel())
        assert (vec.rows, vec.cols, vec.ld) == (p.numel(), o.numel() * self.c, out.ld * self.c)
        ws = self._ws(p.numel(), o.numel(), m)
        L.check(L.lib().lt_influence_rows_vec(self._h, p.data_ptr(), p.numel(), o.data_ptr(), o.numel(), float(delta), m,
                                              out.assert_aligned(), out.ld, vec.assert_aligned(), ws.data_ptr(), ws.numel(),
                                              _stream()), "lt_influence_rows_vec")
        torch.cuda.synchronize()
        return out.body(), vec.body()

    def pairs(self, probes, pair_ptr, pair_obs, delta, mode):
        from linkteller_amd import engine
        L = _L()
        m = L.MODES[mode]
        p, o = _nodes(probes, self.dev), _nodes(pair_obs, self.dev)
        ptr = np.ascontiguousarray(pair_ptr, dtype=np.int64)
        assert ptr.size == p.numel() + 1
        out = torch.full((o.numel(),), -7.0, dtype=torch.float32, device=self.dev)
        ws = engine._workspace(L.lib().lt_influence_pairs_workspace_bytes(self._h, p.numel(), o.numel(), m), self.dev)
        L.check(L.lib().lt_influence_pairs(self._h, p.data_ptr(), p.numel(), ptr.ctypes.data, o.data_ptr(), o.numel(), float(delta),
                                           m, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "lt_influence_pairs")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def matrix_host(self, probes, obs, delta, mode, out: View, dst: torch.Tensor, ldd):
        """lt_influence_matrix_host: ``dst`` is a PINNED float64 tensor of n_probe * ldd elements (the caller pre-fills it)."""
        L = _L()
        m = L.MODES[mode]
        p, o = _nodes(probes, self.dev), _nodes(obs, self.dev)
        assert dst.is_pinned() and dst.dtype == torch.float64 and dst.numel() >= p.numel() * ldd and dst.data_ptr() % 16 == 0
        ws = self._ws(p.numel(), o.numel(), m)
        L.check(L.lib().lt_influence_matrix_host(self._h, p.data_ptr(), p.numel(), o.data_ptr(), o.numel(), float(delta), m,
                                                 out.assert_aligned(), out.ld, dst.data_ptr(), ldd, ws.data_ptr(), ws.numel(),
                                                 _stream()), "lt_influence_matrix_host")
        return out.body()

    def host_landing_stats(self):
        L = _L()
        o = (C.c_int64 * 4)()
        L.check(L.lib().lt_host_landing_stats(self._h, o), "lt_host_landing_stats")
        return [int(v) for v in o]


class RawBaseline3:
    """lt_baseline3_* / lt_influence3_rows_mode on Views."""

    def __init__(self, hg, x: View, f, w1: View, b1: View, h1, w2: View, b2: View, h2, w3: View, b3: View, c):
        L = _L()
        assert w1.ld == h1 and w2.ld == h2 and w3.ld == c
        self.hg, self.n, self.dev = hg, hg.n, x.buf.device
        self.keep = (x, w1, b1, w2, b2, w3, b3)
        hd = C.c_void_p()
        L.check(L.lib().lt_baseline3_create(hg.handle, x.assert_aligned(), x.ld, f, w1.assert_aligned(), b1.assert_aligned(), h1,
                                            w2.assert_aligned(), b2.assert_aligned(), h2, w3.assert_aligned(), b3.assert_aligned(),
                                            c, _stream(), C.byref(hd)), "lt_baseline3_create")
        self._h = hd
        self._finalizer = weakref.finalize(self, L.lib().lt_baseline3_destroy, hd)

    def destroy(self):
        torch.cuda.synchronize()
        self._finalizer()

    def enable_fp64(self):
        L = _L()
        L.check(L.lib().lt_baseline3_enable_fp64(self._h, _stream()), "lt_baseline3_enable_fp64")
        return self

    def rows(self, probes, obs, delta, mode, out: View):
        from linkteller_amd import engine
        L = _L()
        m = L.MODES[mode]
        p, o = _nodes(probes, self.dev), _nodes(obs, self.dev)
        assert (out.rows, out.cols) == (p.numel(), o.numel())
        ws = engine._workspace(L.lib().lt_influence3_workspace_bytes(self._h, p.numel(), o.numel()), self.dev)
        L.check(L.lib().lt_influence3_rows_mode(self._h, p.data_ptr(), p.numel(), o.data_ptr(), o.numel(), float(delta), m,
                                                out.assert_aligned(), out.ld, ws.data_ptr(), ws.numel(), _stream()),
                "lt_influence3_rows_mode")
        torch.cuda.synchronize()
        return out.body()

"""Host-side graph preparation and the device-resident graph handle.

Mirrors, for the hot path only, what the reference does between reading an adjacency and
handing it to the model:

* ``fetch_normalization(name)`` -- the six ``--norm`` choices of reference utils/load.py:562-627
  (``FirstOrderGCN`` = ``I + D^-1/2 A D^-1/2`` is the one BASELINE.json uses).  Computed on the
  CSR arrays in the reference's multiplication order ``(d_i * a_ij) * d_j`` and in the dtype numpy
  promotion gives the reference (float32 for a float32 adjacency), so the float32 values handed
  to the device are the reference's bit for bit.
* ``sparse_mx_to_torch_sparse_tensor`` (reference utils/load.py:552-559) -- kept for API parity;
  the product path converts to int32 CSR instead (8 B/nnz rather than the reference's 20 B/nnz
  int64 COO) and uploads it once through ``lt_graph_create``.  An adjacency that already lies on the device (what
  ``Worker`` ends with: ``adj_2.cuda()``) stays there: ``lt_graph_create_device`` builds the same tables with kernels
  (``HipGraph.from_device_csr``, ``from_torch_sparse`` on a CUDA tensor; ``LT_GRAPH_BUILD`` selects the builder).
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np
import scipy.sparse as sp

from . import _lib


# ----------------------------------------------------------------------------------------------
# normalisers (host; dtype follows numpy promotion from the input, as in the reference)
# ----------------------------------------------------------------------------------------------
def _canonical_csr(adj) -> sp.csr_matrix:
    # dtype is deliberately NOT forced: the reference's arithmetic follows numpy promotion from
    # the adjacency's dtype (float32 for the MUSAE readers, utils/load.py:456-460 -> the whole
    # normalisation runs in float32; integer for the DP-perturbed graphs -> float64).
    a = sp.csr_matrix(adj, copy=True)
    if a.dtype == np.bool_:
        a = a.astype(np.int64)
    a.sum_duplicates()
    a.sort_indices()
    return a


def _with_identity(a: sp.csr_matrix) -> sp.csr_matrix:
    out = _canonical_csr(a + sp.identity(a.shape[0], dtype=np.float64, format="csr"))  # float64 from here
    return out


def _inv_power(row_sum: np.ndarray, power: float, zero_inf: bool) -> np.ndarray:
    with np.errstate(divide="ignore"):
        d = np.power(row_sum, power)
    if zero_inf:
        d[np.isinf(d)] = 0.0
    return d


def _scale(a: sp.csr_matrix, left: np.ndarray, right=None) -> sp.csr_matrix:
    """(diag(left) @ a) @ diag(right), entry-wise in that association."""
    rows = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))
    data = left[rows] * a.data
    if right is not None:
        data = data * right[a.indices]
    return sp.csr_matrix((data, a.indices.copy(), a.indptr.copy()), shape=a.shape)


def _row_sums(a: sp.csr_matrix) -> np.ndarray:
    return np.asarray(a.sum(axis=1)).ravel()


def first_order_gcn(adj):
    """``FirstOrderGCN``: I + D^-1/2 A D^-1/2 (reference utils/load.py:572-578)."""
    a = _canonical_csr(adj)
    d = _inv_power(_row_sums(a), -0.5, True)
    return _canonical_csr(sp.identity(a.shape[0], dtype=np.float64, format="csr") + _scale(a, d, d))


def aug_normalized_adjacency(adj):
    """``AugNormAdj``: (D+I)^-1/2 (A+I) (D+I)^-1/2 (reference utils/load.py:562-569)."""
    a = _with_identity(_canonical_csr(adj))
    d = _inv_power(_row_sums(a), -0.5, True)
    return _canonical_csr(_scale(a, d, d))


def bingge_norm_adjacency(adj):
    """``BingGeNormAdj``: (D+I)^-1/2 (A+I) (D+I)^-1/2 + I (reference utils/load.py:581-588)."""
    return _canonical_csr(aug_normalized_adjacency(adj) + sp.identity(adj.shape[0], dtype=np.float64, format="csr"))


def normalized_adjacency(adj):
    """``NormAdj``: D^-1/2 A D^-1/2 (reference utils/load.py:591-597)."""
    a = _canonical_csr(adj)
    d = _inv_power(_row_sums(a), -0.5, True)
    return _canonical_csr(_scale(a, d, d))


def random_walk(adj):
    """``RWalk``: D^-1 A (reference utils/load.py:600-605; infinities are NOT zeroed there)."""
    a = _canonical_csr(adj)
    return _canonical_csr(_scale(a, _inv_power(_row_sums(a), -1.0, False)))


def aug_random_walk(adj):
    """``AugRWalk``: (D+I)^-1 (A+I) (reference utils/load.py:608-614)."""
    a = _with_identity(_canonical_csr(adj))
    return _canonical_csr(_scale(a, _inv_power(_row_sums(a), -1.0, False)))


_NORMALIZERS = {
    "FirstOrderGCN": first_order_gcn,
    "BingGeNormAdj": bingge_norm_adjacency,
    "NormAdj": normalized_adjacency,
    "AugRWalk": aug_random_walk,
    "RWalk": random_walk,
    "AugNormAdj": aug_normalized_adjacency,
}


def fetch_normalization(name: str):
    """Same lookup contract as reference utils/load.py:617-627."""
    try:
        return _NORMALIZERS[name]
    except KeyError:
        raise NotImplementedError(f"normalization {name!r} not implemented") from None


def sparse_mx_to_torch_sparse_tensor(sparse_mx):
    """scipy -> torch sparse COO, float32 values / int64 indices (reference utils/load.py:552-559)."""
    import torch
    m = sp.coo_matrix(sparse_mx).astype(np.float32)
    idx = torch.from_numpy(np.vstack((m.row, m.col)).astype(np.int64))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(m.data), torch.Size(m.shape))


# ----------------------------------------------------------------------------------------------
# the same on the device, for a 0/1 pattern that already lies there (a DP graph: dp.perturb_adj_device)
# ----------------------------------------------------------------------------------------------
def inv_power_table(name: str, n: int) -> np.ndarray:
    """float64 [n + 2]: what ``_inv_power`` gives the row sums 0 .. n + 1 under the normaliser ``name`` -- the table
    ``lt_normalize_csr`` reads instead of computing a power on the device."""
    if name not in _NORMALIZERS:
        raise NotImplementedError(f"normalization {name!r} not implemented")
    walk = name in ("RWalk", "AugRWalk")
    return _inv_power(np.arange(n + 2, dtype=np.float64), -1.0 if walk else -0.5, not walk)


def normalize_device(name: str, rowptr, col):
    """``csr_arrays(fetch_normalization(name)(a))`` for the 0/1 matrix ``a`` whose pattern is the device CSR (``rowptr`` int32
    [n + 1], ``col`` int32, CUDA tensors, columns strictly increasing): (rowptr, col, val) on the device, structure and float32
    bits equal to the host's (``lt_normalize_csr``).  Reads 32 bytes back: the nnz and the count of malformed rows."""
    import torch
    if name not in _NORMALIZERS:
        raise NotImplementedError(f"normalization {name!r} not implemented")
    _lib.require_gpu()
    for what, t in (("rowptr", rowptr), ("col", col)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1:
            raise TypeError(f"normalize_device: {what} must be a 1-D int32 CUDA tensor")
    if rowptr.numel() < 2 or rowptr.device != col.device:
        raise ValueError("normalize_device: rowptr needs n + 1 >= 2 words on the device of col")
    rowptr, col = rowptr.contiguous(), col.contiguous()
    n, nnz = rowptr.numel() - 1, col.numel()
    dev = rowptr.device
    inv_pow = torch.from_numpy(inv_power_table(name, n)).to(dev)
    capacity = nnz + n
    out_rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    out_col = torch.empty(capacity, dtype=torch.int32, device=dev)
    out_val = torch.empty(capacity, dtype=torch.float32, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    col_arg = col if nnz else col.new_zeros(1)                            # a pointer even for an empty graph
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().lt_normalize_csr(n, rowptr.data_ptr(), col_arg.data_ptr(), nnz, _lib.NORM_CODES[name], inv_pow.data_ptr(),
                                               out_rowptr.data_ptr(), out_col.data_ptr(), out_val.data_ptr(), capacity,
                                               info.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "lt_normalize_csr")
    out_nnz, bad = info[:2].tolist()
    if bad:
        raise ValueError(f"normalize_device: {bad} rows whose columns are not strictly increasing or not in [0, {n})")
    return out_rowptr, out_col[:out_nnz], out_val[:out_nnz]


def torch_sparse_from_device_csr(rowptr, col, val):
    """The sparse COO CUDA tensor ``sparse_mx_to_torch_sparse_tensor(m).cuda()`` gives for the matrix of this device CSR: int64
    indices in row-major order, float32 values, not marked coalesced.  Torch ops on the device, no kernel of ours."""
    import torch
    n = rowptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=rowptr.device), torch.diff(rowptr).to(torch.int64),
                                   output_size=int(col.numel()))
    return torch.sparse_coo_tensor(torch.stack((rows, col.to(torch.int64))), val.to(torch.float32), torch.Size((n, n)))


# ----------------------------------------------------------------------------------------------
# device graph handle
# ----------------------------------------------------------------------------------------------
def csr_arrays(mat):
    """(n, rowptr int32, col int32, val float32) of a square sparse matrix, canonical form."""
    a = sp.csr_matrix(mat)
    if a.shape[0] != a.shape[1]:
        raise ValueError(f"adjacency must be square, got {a.shape}")
    a = a.astype(np.float32)       # the reference rounds to f32 BEFORE any duplicate could be summed
    a.sum_duplicates()
    a.sort_indices()
    if a.nnz >= 2**31 - 1:
        raise ValueError("nnz does not fit int32 row pointers")
    return (a.shape[0], np.ascontiguousarray(a.indptr, dtype=np.int32),
            np.ascontiguousarray(a.indices, dtype=np.int32), np.ascontiguousarray(a.data, dtype=np.float32))


def _build_mode() -> str:
    """``LT_GRAPH_BUILD``: ``auto`` (default: inputs that lie on the device build there, host inputs on the host), ``host``
    (always ``lt_graph_create``) or ``device`` (always ``lt_graph_create_device``; host inputs are uploaded as canonical CSR)."""
    mode = os.environ.get("LT_GRAPH_BUILD", "").strip().lower() or "auto"
    if mode not in ("auto", "host", "device"):
        raise ValueError(f"LT_GRAPH_BUILD must be auto, host or device, got {mode!r}")
    return mode


class HipGraph:
    """Normalised adjacency resident in HBM as CSR (+ CSC) behind an ``lt_graph`` handle."""

    def __init__(self, mat):
        _lib.require_gpu()
        n, rowptr, col, val = csr_arrays(mat)
        if _build_mode() == "device":
            import torch
            dev = torch.device("cuda", torch.cuda.current_device())
            self._create_device(*(torch.from_numpy(a).to(dev) for a in (rowptr, col, val)))
            return
        h = C.c_void_p()
        _lib.check(_lib.lib().lt_graph_create(n, int(col.shape[0]), rowptr.ctypes.data, col.ctypes.data,
                                              val.ctypes.data, C.byref(h)), "lt_graph_create")
        import torch
        self._adopt(h, n, int(col.shape[0]), torch.cuda.current_device(), "host")      # lt_graph_create uploads to the current device

    def _adopt(self, h, n, nnz, device_index, built_on):
        self._h = h
        self.n = n
        self.nnz = nnz
        self.device_index = device_index
        self.built_on = built_on          # "host" (lt_graph_create) or "device" (lt_graph_create_device)
        self._finalizer = weakref.finalize(self, _lib.lib().lt_graph_destroy, h)

    def _create_device(self, rowptr, col, val):
        import torch
        for name, t, dt in (("rowptr", rowptr, torch.int32), ("col", col, torch.int32), ("val", val, torch.float32)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise TypeError(f"from_device_csr: {name} must be a CUDA tensor")
            if t.dtype != dt or t.dim() != 1:
                raise TypeError(f"from_device_csr: {name} must be a 1-D {dt} tensor, got {t.dtype} with {t.dim()} dimensions")
        if not (rowptr.device == col.device == val.device):
            raise ValueError("from_device_csr: rowptr, col and val lie on different devices")
        if rowptr.numel() < 1 or col.numel() != val.numel():
            raise ValueError(f"from_device_csr: rowptr of {rowptr.numel()} words, {col.numel()} columns, {val.numel()} values")
        rowptr, col, val = rowptr.contiguous(), col.contiguous(), val.contiguous()
        n, nnz = rowptr.numel() - 1, col.numel()
        h = C.c_void_p()
        with torch.cuda.device(rowptr.device):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.lib().lt_graph_create_device(n, nnz, rowptr.data_ptr(), col.data_ptr() if nnz else None,
                                                         val.data_ptr() if nnz else None, stream, C.byref(h)),
                       "lt_graph_create_device")
        self._adopt(h, n, nnz, rowptr.device.index, "device")

    @classmethod
    def from_device_csr(cls, rowptr, col, val):
        """A graph from a canonical CSR that already lies on the device: int32 ``rowptr`` [n + 1], int32 ``col`` and float32
        ``val`` [nnz] CUDA tensors, columns strictly increasing inside each row.  Read on torch's current stream, validated and
        copied by ``lt_graph_create_device``; every derived table is built on the device."""
        _lib.require_gpu()
        g = cls.__new__(cls)
        g._create_device(rowptr, col, val)
        return g

    @classmethod
    def from_device_pattern(cls, rowptr, col, norm):
        """A graph from a 0/1 pattern on the device (``dp.perturb_adj_device``): normalised there (``normalize_device``) and
        handed to ``from_device_csr``."""
        return cls.from_device_csr(*normalize_device(norm, rowptr, col))

    @property
    def handle(self):
        return self._h

    @property
    def max_row_nnz(self) -> int:
        m = C.c_int32()
        _lib.check(_lib.lib().lt_graph_info(self._h, None, None, C.byref(m)), "lt_graph_info")
        return m.value

    def table(self, name: str) -> np.ndarray:
        """One table of the graph read back through ``lt_graph_table`` (``_lib.GRAPH_TABLES``; an absent table is empty)."""
        which, dtype = _lib.GRAPH_TABLES[name]
        size = C.c_int64()
        _lib.check(_lib.lib().lt_graph_table(self._h, which, None, 0, C.byref(size)), "lt_graph_table")
        out = np.empty(size.value // np.dtype(dtype).itemsize, dtype=dtype)
        if size.value:
            _lib.check(_lib.lib().lt_graph_table(self._h, which, out.ctypes.data, out.nbytes, C.byref(size)), "lt_graph_table")
        return out

    def scalars(self) -> dict:
        return dict(zip(_lib.GRAPH_SCALARS, self.table("scalars").tolist()))

    @classmethod
    def from_torch_sparse(cls, t):
        """Accepts what the reference feeds its model: an (uncoalesced) sparse COO float tensor.  A tensor that lies on the device
        is coalesced there and handed to the device builder, unless coalescing summed duplicates: the reference rounds to
        float32 before duplicates are summed and the device's summation order is not fixed, so that case (like every CPU
        tensor, and everything under ``LT_GRAPH_BUILD=host``) takes the host route."""
        import torch
        if t.is_cuda and _build_mode() != "host":
            t = t.detach()
            if t.dim() != 2 or t.shape[0] != t.shape[1]:
                raise ValueError(f"adjacency must be square, got {tuple(t.shape)}")
            c = t.coalesce()
            if c._nnz() == t._nnz():
                if c._nnz() >= 2**31 - 1:
                    raise ValueError("nnz does not fit int32 row pointers")
                n = int(t.shape[0])
                idx = c.indices()
                rowptr = torch.zeros(n + 1, dtype=torch.int64, device=c.device)
                rowptr[1:] = torch.cumsum(torch.bincount(idx[0], minlength=n), 0)
                return cls.from_device_csr(rowptr.to(torch.int32), idx[1].to(torch.int32).contiguous(),
                                           c.values().to(torch.float32).contiguous())
        t = t.detach().cpu().coalesce()
        idx = t.indices().numpy()
        m = sp.coo_matrix((t.values().numpy().astype(np.float32), (idx[0], idx[1])), shape=tuple(t.shape))
        return cls(m)


_GRAPH_CACHE: "dict[int, tuple]" = {}


def as_hip_graph(adj) -> HipGraph:
    """HipGraph for whatever the caller holds (HipGraph / torch sparse / scipy), cached per object."""
    if isinstance(adj, HipGraph):
        return adj
    key = id(adj)
    hit = _GRAPH_CACHE.get(key)
    if hit is not None and hit[0]() is adj:
        return hit[1]
    import torch
    if isinstance(adj, torch.Tensor):
        if not adj.is_sparse:
            raise TypeError("adj must be a sparse tensor, a scipy sparse matrix or a HipGraph")
        g = HipGraph.from_torch_sparse(adj)
    else:
        g = HipGraph(adj)
    try:
        ref = weakref.ref(adj, lambda _r, k=key: _GRAPH_CACHE.pop(k, None))
        _GRAPH_CACHE[key] = (ref, g)
    except TypeError:
        pass
    return g

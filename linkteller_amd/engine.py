"""Thin torch-facing wrappers over the C ABI: torch owns device memory and streams, the kernels
are liblinkteller_hip's.  Every function enqueues on torch's current stream and never syncs."""
from __future__ import annotations

import ctypes as C
import weakref

import torch

from . import _lib
from .graph import HipGraph, as_hip_graph


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's current stream (of the current device) as the ``void *`` the C ABI takes.  The raw getter is what torch's own
    launchers use: ~0.3 us against ~3 us for building a ``torch.cuda.Stream`` object -- three of them sat in front of the first
    launch of every ``Attacker.influence_matrix()`` call (tools/api_profile.py)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise _lib.LinkTellerHipError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def _require_finite(**tensors):
    """ReLU is one ``v_max_f32`` in the kernels: a NaN pre-activation becomes 0 where torch keeps NaN (DESIGN.md
    section 3), so non-finite inputs would be hidden instead of propagated.  They are refused up front (one device
    reduction per tensor when a baseline is created, never on the per-step path)."""
    for name, t in tensors.items():
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{name} holds non-finite values (NaN / Inf): the reference would propagate them through "
                             f"every score; refusing rather than masking them")


def _workspace(nbytes: int, device) -> torch.Tensor:
    # torch's caching allocator returns >= 512-byte aligned blocks
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _pinned_f64(rows: int, cols: int) -> torch.Tensor:
    # a block of torch's pinned-memory cache: recycled when its last owner is released, so a fresh one per step allocates nothing
    return torch.empty((rows, cols), dtype=torch.float64, pin_memory=True)


def gemm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a @ b on the matrix cores in exact fp32 (reference gcn/layers.py:31 torch.mm)."""
    a, b = _f32(a, "a"), _f32(b, "b")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0]:
        raise ValueError(f"shape mismatch {tuple(a.shape)} @ {tuple(b.shape)}")
    m, k = a.shape
    n = b.shape[1]
    out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().lt_gemm_f32(a.data_ptr(), k, b.data_ptr(), n, out.data_ptr(), n, m, n, k, _stream()),
               "lt_gemm_f32")
    return out


def spmm(adj, dense: torch.Tensor, bias=None, relu: bool = False) -> torch.Tensor:
    """adj @ dense (+ bias)(relu)  (reference gcn/layers.py:32-36 torch.spmm + bias)."""
    g = as_hip_graph(adj)
    s = _f32(dense, "dense")
    if s.dim() != 2 or s.shape[0] != g.n:
        raise ValueError(f"dense must be [{g.n}, k], got {tuple(s.shape)}")
    k = s.shape[1]
    out = torch.empty((g.n, k), dtype=torch.float32, device=s.device)
    bptr = None
    if bias is not None:
        bias = _f32(bias, "bias")
        bptr = bias.data_ptr()
    _lib.check(_lib.lib().lt_spmm_csr_f32(g.handle, s.data_ptr(), k, k, bptr, int(bool(relu)),
                                          out.data_ptr(), k, _stream()), "lt_spmm_csr_f32")
    return out


def gcn2_forward(adj, x, w1, b1, w2, b2) -> torch.Tensor:
    """Logits of the 2-layer GCN in eval mode (reference gcn/models.py:19-24)."""
    g = as_hip_graph(adj)
    x, w1, b1, w2, b2 = (_f32(t, n) for t, n in ((x, "x"), (w1, "W1"), (b1, "b1"), (w2, "W2"), (b2, "b2")))
    n, f = x.shape
    h, c = w1.shape[1], w2.shape[1]
    if n != g.n or w1.shape[0] != f or w2.shape[0] != h or b1.numel() != h or b2.numel() != c:
        raise ValueError("inconsistent GCN shapes")
    if not fused_shapes(h, c):      # wider than the fused kernels: the same layers unfused (GraphConvolution.forward x 2)
        return spmm(g, gemm(spmm(g, gemm(x, w1), b1, relu=True), w2), b2)
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    nbytes = _lib.lib().lt_gcn2_workspace_bytes(n, f, h, c)
    ws = _workspace(nbytes, x.device)
    _lib.check(_lib.lib().lt_gcn2_forward(g.handle, x.data_ptr(), f, f, w1.data_ptr(), b1.data_ptr(), h,
                                          w2.data_ptr(), b2.data_ptr(), c, out.data_ptr(), c,
                                          ws.data_ptr(), ws.numel(), _stream()), "lt_gcn2_forward")
    return out


def _x_version(x):
    try:
        return x._version
    except RuntimeError:        # (an inference tensor keeps no version counter: its edits are announced by features_changed())
        return None


def _refresh_handle(owner, name, *args):
    """Every lt_baseline_refresh* call on a handle goes through here.  A refresh announces changed WEIGHTS; a baseline on the
    feature-difference route keeps lists of X built once, so changed contents of X are announced by *_features_changed first --
    which this does whenever torch's version counter of the feature tensor moved since the lists were built (an in-place edit
    followed by refresh() keeps giving what it always gave).  Writes torch does not see (a raw pointer, another library) are
    announced with ``features_changed()``."""
    v = _x_version(owner.x)
    if v != owner._x_seen:
        changed = owner._SYM["changed"]
        _lib.check(getattr(_lib.lib(), changed)(owner._h, _stream()), changed)
        owner._x_seen = v
    _lib.check(getattr(_lib.lib(), name)(owner._h, *args, _stream()), name)


def _symbols(handle, calls, rows=None):
    """The library's names of a probe handle's calls: ``handle`` prefixes the handle's own, ``calls`` the probe primitive's."""
    return {"destroy": handle + "_destroy", "changed": handle + "_features_changed", "logits": handle + "_logits",
            "rows": rows or calls + "_rows", "rows_ws": calls + "_workspace_bytes", "pairs": calls + "_pairs",
            "pairs_ws": calls + "_pairs_workspace_bytes"}


class _ProbeHandle:
    """What the probe handles ``Baseline``, ``Baseline3`` and ``Baseline2W`` share: the borrowed inputs and their checks, the
    handle with its finalizer, ``features_changed`` / ``logits``, the cached workspace, the operands of the rectangle and the
    whole of ``influence_pairs``.  A class says which symbols it calls (``_SYM``), which mode ``None`` stands for
    (``_DEFAULT_MODE``), which modes it serves (``_serves``), whether `delta` needs ``enable_fp64`` first (``_fp64`` is False
    until then; a class whose fp64 parts exist from creation sets it True) and whether its workspace depends on the mode
    (``_WS_MODE``)."""

    _SYM = None
    _DEFAULT_MODE = "delta"
    _WS_MODE = False
    _fp64 = False

    def _take(self, adj, error, **tensors):
        """The constructor's front: ``x`` and (W, b) per layer by name -> ``self.x``, ``self.w1``, ``self.b1`` ... as contiguous
        fp32 CUDA tensors, checked for consistent shapes (``ValueError(error)``), one device and finite values.  Returns the
        widths (n, F, then every layer's)."""
        self.graph: HipGraph = as_hip_graph(adj)
        held = [_f32(t, name) for name, t in tensors.items()]
        for name, t in zip(tensors, held):
            setattr(self, name.lower(), t)
        self.n, self.f = n, f = self.x.shape
        widths, ok = [n, f], n == self.graph.n
        for w, b in zip(held[1::2], held[2::2]):
            ok = ok and w.shape[0] == widths[-1] and b.numel() == w.shape[1]
            widths.append(w.shape[1])
        if not ok:
            raise ValueError(error)
        if self.graph.device_index != self.x.device.index:
            raise ValueError(f"the graph lives on cuda:{self.graph.device_index}, the features on {self.x.device}")
        _require_finite(**{"features" if name == "x" else name: t for name, t in zip(tensors, held)})
        self._layers = [a for w, b in zip(held[1::2], held[2::2]) for a in (w.data_ptr(), b.data_ptr(), w.shape[1])]
        return widths

    def _open(self, create):
        """lt_*_create over what ``_take`` holds: the handle, its finalizer, the features' version, the workspace cache."""
        h = C.c_void_p()
        _lib.check(getattr(_lib.lib(), create)(self.graph.handle, self.x.data_ptr(), self.f, self.f, *self._layers, _stream(),
                                               C.byref(h)), create)
        self._h = h
        self._x_seen = _x_version(self.x)       # the features' version the baseline's difference lists (if any) were built from
        self._finalizer = weakref.finalize(self, getattr(_lib.lib(), self._SYM["destroy"]), h)
        self._ws = {}

    @property
    def handle(self):
        return self._h

    def features_changed(self):
        """The contents of the feature tensor changed in a way torch's version counter does not show (a write through the raw
        pointer, by another library): the difference lists of the feature route are built again (lt_baseline_features_changed
        and its twins; may synchronise) and everything ``refresh()`` marks stale is stale.  In-place torch edits need no call:
        ``refresh()`` sees the version counter."""
        changed = self._SYM["changed"]
        _lib.check(getattr(_lib.lib(), changed)(self._h, _stream()), changed)
        self._x_seen = _x_version(self.x)
        return self

    def logits(self) -> torch.Tensor:
        out = torch.empty((self.n, self.c), dtype=torch.float32, device=self.x.device)
        _lib.check(getattr(_lib.lib(), self._SYM["logits"])(self._h, out.data_ptr(), _stream()), self._SYM["logits"])
        return out

    def _serves(self, m):
        """Raise ``NotImplementedError`` for a mode the handle does not serve (before the node lists are touched)."""

    def _mode(self, mode) -> int:
        m = _lib.MODES[mode or self._DEFAULT_MODE] if isinstance(mode, str) or mode is None else int(mode)
        self._serves(m)
        return m

    def _workspace(self, key, need):
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = _workspace(need, self.x.device)
            self._ws = {key: ws}   # keep only the latest: sizes repeat across steps
        return ws

    def _operands(self, m, probe_nodes, listed_nodes, out, ptr=None):
        """What a rows call, or with the offsets ``ptr`` a pairs call, hands the library: the two node lists (``_as_nodes``), ``out``
        allocated or validated, the fp64 parts for `delta`, the cached workspace by the call's own query."""
        dev = self.x.device
        probes = _as_nodes(probe_nodes, self.n, dev, "probe_nodes")
        listed = _as_nodes(listed_nodes, self.n, dev, "observe_nodes" if ptr is None else "pair_obs")
        npb, nls = probes.numel(), listed.numel()
        if ptr is not None and ptr.size != npb + 1:
            raise ValueError(f"pair_ptr must hold n_probe + 1 = {npb + 1} offsets, got {ptr.size}")
        shape = (npb, nls) if ptr is None else (nls,)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        elif out.shape != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out must be a contiguous float32 {'[n_probe, n_obs]' if ptr is None else '[n_pairs]'} tensor on the "
                             "baseline's device")
        if m == _lib.MODE_DELTA and not self._fp64:
            # kink test on an fp64-accumulated pre-activation (one-off cost, kept fresh by refresh())
            self.enable_fp64()
        extra = (m,) if self._WS_MODE else ()
        key = ((npb, nls) if ptr is None else ("pairs", npb, nls)) + extra
        query = getattr(_lib.lib(), self._SYM["rows_ws" if ptr is None else "pairs_ws"])
        return probes, listed, out, self._workspace(key, query(self._h, npb, nls, *extra))   # (host arithmetic; depends on the knobs too)

    def _rows(self, probe_nodes, observe_nodes, delta, mode, out, name=None, host=None):
        """The rectangle by the handle's rows call, or by ``name``, a call that takes a float64 matrix ``host`` behind ``out``."""
        m = self._mode(mode)
        probes, obs, out, ws = self._operands(m, probe_nodes, observe_nodes, out)
        npb, nob = out.shape
        name = name or self._SYM["rows"]
        dst = () if host is None else (host.data_ptr(), max(nob, 1))
        _lib.check(getattr(_lib.lib(), name)(self._h, probes.data_ptr(), npb, obs.data_ptr(), nob, float(delta), m, out.data_ptr(),
                                             nob, *dst, ws.data_ptr(), ws.numel(), _stream()), name)
        return out

    def influence_pairs(self, probe_nodes, pair_ptr, pair_obs, delta: float, mode="delta", out=None) -> torch.Tensor:
        """[n_pairs] fp32 on the device: the scores of a LIST of pairs grouped by probe (lt_influence_pairs, lt_influence3_pairs,
        lt_influence2w_pairs).  Probe i = ``probe_nodes[i]`` owns ``pair_obs[pair_ptr[i]:pair_ptr[i + 1]]`` (``group_pairs`` builds
        the three from two id arrays) and ``out[k]`` is what ``influence_rows`` writes at (that probe, ``pair_obs[k]``) for the
        same mode, bit for bit -- without the rectangle: the output and the workspace are sized by the list.  ``pair_ptr`` is a
        HOST array of n_probe + 1 int64 offsets (validated by the library before anything is launched); the node lists follow
        ``influence_rows`` (int32 CUDA tensors are checked on the device: ``engine.node_check()`` after synchronising).  Modes as
        in ``influence_rows``."""
        import numpy as np
        m = self._mode(mode)
        if isinstance(pair_ptr, torch.Tensor):
            pair_ptr = pair_ptr.cpu().numpy()
        ptr = np.ascontiguousarray(np.asarray(pair_ptr).reshape(-1), dtype=np.int64)
        probes, obs, out, ws = self._operands(m, probe_nodes, pair_obs, out, ptr)
        pairs = self._SYM["pairs"]
        _lib.check(getattr(_lib.lib(), pairs)(self._h, probes.data_ptr(), probes.numel(), ptr.ctypes.data, obs.data_ptr(),
                                              obs.numel(), float(delta), m, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                   pairs)
        return out


class Baseline(_ProbeHandle):
    """Unperturbed forward state (S1, Z1, S2, logits) for the probe loop; see lt_baseline_create."""

    _SYM = _symbols("lt_baseline", "lt_influence")
    _DEFAULT_MODE = "full"
    _WS_MODE = True

    def __init__(self, adj, x, w1, b1, w2, b2):
        _, _, self.h, self.c = self._take(adj, "inconsistent GCN shapes", x=x, W1=w1, b1=b1, W2=w2, b2=b2)
        self._open("lt_baseline_create")
        self._host_scratch = {}
        self._fp64 = False
        self._shard = None          # (row_begin, row_end, per) while the sharded refresh of the fp32 product is on
        self._s1_full = None        # torch-owned S1 storage once attached (kept alive for the handle's lifetime)
        self._send = None
        self._shard64 = None        # the same for the fp64 product of `delta` (lt_baseline_refresh_rows_fp64)
        self._s1d_full = None
        self._send64 = None

    def refresh(self, mode=None):
        """The borrowed inputs changed: everything derived from them is recomputed by the next call that reads it.
        ``mode`` (the mode of the calls that follow, when known) lets a multi-GPU run move only what that mode reads:
        with ``shard_refresh`` on, `full` / `sparse` compute this rank's rows of the fp32 X W1 and all-gather S1; `delta`
        with the fp64 pre-activation does the same for the fp64 product (``shard_refresh_fp64``) and touches nothing
        fp32.  Without a mode both sharded products (if enabled) are refreshed."""
        m = None if mode is None else (_lib.MODES[mode] if isinstance(mode, str) else int(mode))
        only64 = m == _lib.MODE_DELTA and self._fp64
        only32 = m is not None and not only64
        from . import dist as lt_dist
        if self._shard is not None and not only64:
            b, e, _ = self._shard
            _refresh_handle(self, "lt_baseline_refresh_rows", b, e, self._send.data_ptr())
            lt_dist.all_gather_into(self._s1_full, self._send)
        else:
            _refresh_handle(self, "lt_baseline_refresh")
        if self._shard64 is not None and not only32:
            b, e, _ = self._shard64
            _refresh_handle(self, "lt_baseline_refresh_rows_fp64", b, e, self._send64.data_ptr())
            lt_dist.all_gather_into(self._s1d_full, self._send64)

    def enable_fp64(self):
        """The fp64-accumulated pre-activation `delta` evaluates its ReLU kink test on (lt_baseline_enable_fp64):
        allocates S1d / Z1d (2 * n * Hp * 8 bytes -- 8.6 GB at n = 2 M, H = 256) and computes them once."""
        if not self._fp64:
            _lib.check(_lib.lib().lt_baseline_enable_fp64(self._h, _stream()), "lt_baseline_enable_fp64")
            self._x_seen = _x_version(self.x)       # (the difference lists were built from these features)
            self._fp64 = True
        return self

    def feature_list_entries(self) -> int:
        """Entries of the difference lists the baseline keeps for the feature route, -1 when it keeps none."""
        r = C.c_int64(-1)
        _lib.check(_lib.lib().lt_baseline_feature_list_entries(self._h, C.byref(r)), "lt_baseline_feature_list_entries")
        return r.value

    def fp64_route(self) -> int:
        """1: the fp64 product comes from the feature rows' differences to a reference row (one pass over X; sharding it
        buys nothing), 0: it runs on the f64 matrix cores, -1: fp64 not enabled."""
        r = C.c_int32(-1)
        _lib.check(_lib.lib().lt_baseline_fp64_route(self._h, C.byref(r)), "lt_baseline_fp64_route")
        return r.value

    def fp64_arrays(self) -> dict:
        """The fp64 product rows and the pre-activation as the last refresh stored them (lt_baseline_fp64_arrays; read after a
        `delta` call): {"product": int32 fixed point [n, Hp] + "scales" [n] float64, or float64 [n, Hp] with scales None;
        "preact": float32 or float64 [n, Hp]; "valid": bool [n], the rows of preact that are formed; "deferred_cref": bool;
        "cref": float64 [Hp], the reference vector's product m W1 on the feature-difference route, else None}.
        Not on the aggregate-first route."""
        dev, n, hp = self.x.device, self.n, (self.h + 3) // 4 * 4
        prod = torch.empty(max(n * hp, 1), dtype=torch.float64, device=dev)
        pre = torch.empty(max(n * hp, 1), dtype=torch.float64, device=dev)
        scales = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        state = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        cref = torch.empty(hp, dtype=torch.float64, device=dev)
        forms = (C.c_int32 * 5)()
        _lib.check(_lib.lib().lt_baseline_fp64_arrays(self._h, prod.data_ptr(), scales.data_ptr(), cref.data_ptr(), pre.data_ptr(),
                                                      state.data_ptr(), forms, _stream()), "lt_baseline_fp64_arrays")
        if forms[0]:
            product, sc = prod.view(torch.int32)[:n * hp].view(n, hp).clone(), scales[:n].clone()
        else:
            product, sc = prod[:n * hp].view(n, hp), None
        preact = pre.view(torch.float32)[:n * hp].view(n, hp).clone() if forms[1] else pre[:n * hp].view(n, hp)
        valid = torch.ones(n, dtype=torch.bool, device=dev) if forms[2] else state[:n] == 1
        return {"product": product, "scales": sc, "preact": preact, "valid": valid, "deferred_cref": bool(forms[3]),
                "cref": cref if forms[4] else None}

    # ---- the on-demand pre-activation by row list (fp64_route() == 2): hub rows shared between ranks, dist.share_hub_rows ----
    def reached_rows(self, probe_nodes, min_entries: int) -> torch.Tensor:
        """Sorted int32 device list of the rows of >= min_entries entries that the probes reach in one hop (lt_graph_reached_rows;
        one host sync for the count: call once per node list, not per step)."""
        dev = self.x.device
        probes = _as_nodes(probe_nodes, self.n, dev, "probe_nodes")
        flags = torch.empty(max(self.n, 1), dtype=torch.int32, device=dev)
        rows = torch.empty(max(self.n, 1), dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().lt_graph_reached_rows(self.graph.handle, probes.data_ptr(), probes.numel(), int(min_entries),
                                                    flags.data_ptr(), rows.data_ptr(), count.data_ptr(), _stream()),
                   "lt_graph_reached_rows")
        return torch.sort(rows[: int(count.item())]).values.contiguous()

    def form_rows_fp64(self, rows: torch.Tensor):
        self.enable_fp64()
        _lib.check(_lib.lib().lt_baseline_form_rows_fp64(self._h, rows.data_ptr(), rows.numel(), _stream()), "lt_baseline_form_rows_fp64")

    def gather_rows_fp64(self, rows: torch.Tensor, dst: torch.Tensor):
        _lib.check(_lib.lib().lt_baseline_gather_rows_fp64(self._h, rows.data_ptr(), rows.numel(), dst.data_ptr(), _stream()),
                   "lt_baseline_gather_rows_fp64")

    def scatter_rows_fp64(self, rows: torch.Tensor, src: torch.Tensor):
        _lib.check(_lib.lib().lt_baseline_scatter_rows_fp64(self._h, rows.data_ptr(), rows.numel(), src.data_ptr(), _stream()),
                   "lt_baseline_scatter_rows_fp64")

    def shard_refresh_fp64(self, enable=True):
        """Multi-GPU: shard the fp64 product X W1 of `delta` over the ranks (rows of k_gemm_f64acc_128 + one all-gather
        of S1d) instead of recomputing it on every rank.  Bits are those of the replicated product."""
        from . import dist as lt_dist
        rank, world = lt_dist.world()
        if not enable or not lt_dist.collectives_on():
            if self._shard64 is not None:
                _lib.check(_lib.lib().lt_baseline_attach_s1d(self._h, None, 0, _stream()), "lt_baseline_attach_s1d")
                torch.cuda.current_stream().synchronize()
                self._s1d_full = self._send64 = None
            self._shard64 = None
            return self
        self.enable_fp64()
        b, e, per = lt_dist.shard_bounds(self.n, rank, world)
        hp = (self.h + 3) // 4 * 4
        if self._s1d_full is None or self._s1d_full.shape[0] != world * per:
            s1d = torch.zeros((world * per, hp), dtype=torch.float64, device=self.x.device)
            _lib.check(_lib.lib().lt_baseline_attach_s1d(self._h, s1d.data_ptr(), hp, _stream()), "lt_baseline_attach_s1d")
            self._s1d_full = s1d
            self._send64 = torch.zeros((per, hp), dtype=torch.float64, device=self.x.device)
        self._shard64 = (b, e, per)
        return self

    def shard_refresh(self, enable=True):
        """Multi-GPU: shard the loop-invariant X W1 over the ranks of the initialised process group
        instead of replicating it.  S1 moves to a torch-owned [world * ceil(n / world), Hp] tensor (the all-gather's
        output) that the library reads in place.  Bits are those of the replicated product."""
        from . import dist as lt_dist
        rank, world = lt_dist.world()
        if not enable or not lt_dist.collectives_on():
            self._shard = None
            return self
        b, e, per = lt_dist.shard_bounds(self.n, rank, world)
        hp = (self.h + 3) // 4 * 4
        if self._s1_full is None or self._s1_full.shape[0] != world * per:
            s1_full = torch.zeros((world * per, hp), dtype=torch.float32, device=self.x.device)
            _lib.check(_lib.lib().lt_baseline_attach_s1(self._h, s1_full.data_ptr(), hp, _stream()), "lt_baseline_attach_s1")
            torch.cuda.current_stream().synchronize()        # the previous storage may be released now
            self._s1_full = s1_full
            self._send = torch.zeros((per, hp), dtype=torch.float32, device=self.x.device)
        self._shard = (b, e, per)
        return self

    def influence_rows(self, probe_nodes, observe_nodes, delta: float, mode="full", out=None, host=None,
                       wait=False) -> torch.Tensor:
        """[n_probe, n_obs] fp32 on the device: ||(f(X + delta e_v x_v^T) - f(X))[u]||_2 / delta.  ``host``: a pinned (or
        device) float64 [n_probe, n_obs] tensor that receives the same matrix widened (valid once the stream has drained;
        with ``wait``, a PINNED HOST tensor that holds it when the call returns: lt_influence_matrix_host).
        Node lists given as int32 CUDA tensors are checked on the device: call ``engine.node_check()`` after synchronising
        (see ``_as_nodes``)."""
        if host is None:
            return self._rows(probe_nodes, observe_nodes, delta, mode, out)
        # lt_influence_matrix_host (``wait``): the same call, and the stream wait; on the fused `delta` route the matrix's zeros
        # are written here on the host while the GPU computes, and only the touched values cross PCIe.  lt_influence_rows_f64:
        # the float64 matrix is written as part of the same call (the fused `delta` route's blocks export their own rows; other
        # routes end with the export launch)
        return self._rows(probe_nodes, observe_nodes, delta, mode, out, "lt_influence_matrix_host" if wait else "lt_influence_rows_f64",
                          host)

    def influence_matrix_host(self, probe_nodes, observe_nodes, delta: float, mode="delta", refresh=False):
        """[n_probe, n_obs] float64 on the HOST (the reference's ``influence_val``, attacker.py:216-229) by ONE library call
        that returns with the matrix in pinned host memory (a block of torch's pinned-memory cache, owned by the returned
        array; lt_influence_matrix_host), then the device-side node-id check (IndexError, as the reference raises).  On the
        fused `delta` route the host zero-fills the matrix while the GPU computes and only the touched values cross PCIe,
        packed; other routes write whole rows without an export launch of their own where the route allows.  ``refresh``:
        mark the loop-invariant baseline stale first (``refresh(mode)``) -- the call then recomputes it.
        A baseline without a sharded refresh does all of that -- refresh, rows, wait, node check -- in ONE library call
        (lt_influence_step_host): the node lists are converted once, the cached workspace is passed as it is (the library says
        when it is too small: one retry) and the IndexError comes from that call's own return code.  A sharded refresh runs
        collectives, so such a baseline keeps the separate calls; a call with an empty list is its refresh and nothing else."""
        dev = self.x.device
        probes = _as_nodes(probe_nodes, self.n, dev, "probe_nodes")
        obs = _as_nodes(observe_nodes, self.n, dev, "observe_nodes")
        npb, nob = probes.numel(), obs.numel()
        host = _pinned_f64(npb, nob)
        key = ("scratch", npb, nob)
        out = self._host_scratch.get(key)
        if out is None:
            out = torch.empty((npb, nob), dtype=torch.float32, device=dev)
            self._host_scratch = {key: out}
        if self._shard is not None or self._shard64 is not None or not (npb and nob):      # (an empty list: the refresh, no rows call)
            if refresh:
                self.refresh(mode)
            if npb and nob:
                self.influence_rows(probes, obs, delta, mode, out=out, host=host, wait=True)
                node_check()
            return host.numpy()
        m = _lib.MODES[mode] if isinstance(mode, str) else int(mode)
        if m == _lib.MODE_DELTA and not self._fp64:
            self.enable_fp64()
        if refresh:
            # (what _refresh_handle does in front of every refresh: in-place torch edits of X are announced first)
            v = _x_version(self.x)
            if v != self._x_seen:
                _lib.check(_lib.lib().lt_baseline_features_changed(self._h, _stream()), "lt_baseline_features_changed")
                self._x_seen = v
        flags = (_lib.STEP_REFRESH | _lib.STEP_DST_PINNED) if refresh else _lib.STEP_DST_PINNED
        step = _lib.lib().lt_influence_step_host
        ws = next(iter(self._ws.values()), None)
        if ws is None:
            ws = self._step_workspace(npb, nob, m, dev)
        args = (self._h, probes.data_ptr(), npb, obs.data_ptr(), nob, float(delta), m, out.data_ptr(), nob, host.data_ptr(),
                max(nob, 1))
        rc = step(*args, ws.data_ptr(), ws.numel(), _stream(), flags, None, None)
        if rc == _lib.LT_ERR_WORKSPACE:      # (refused before anything was enqueued or marked stale: ask, regrow, call again -- once)
            ws = self._step_workspace(npb, nob, m, dev)
            rc = step(*args, ws.data_ptr(), ws.numel(), _stream(), flags, None, None)
        if rc:
            _lib.check(rc, "lt_influence_step_host")
        return host.numpy()

    def _step_workspace(self, npb, nob, m, dev):
        ws = _workspace(_lib.lib().lt_influence_workspace_bytes(self._h, npb, nob, m), dev)
        self._ws = {(npb, nob, m): ws}
        return ws

    def host_landing_stats(self) -> dict:
        """The packed ``influence_matrix_host`` calls on this baseline so far (lt_host_landing_stats): how many walked the index
        run ahead of its values (``early``, the ``export_early`` look) / did not (``late``), the nanoseconds the host spent placing
        (``post_ns``: behind the stream wait, or, for a polled call, from the zero-fill's end to the complete matrix), and the
        index words an ``export_early`` = 2 look saw differently from the finished run (``mismatch``).  And, of those calls
        (lt_host_landing_stats2): how many placed their values as they landed, by look (``polled``, the ``host_poll`` path), how
        many of these ran out of stall budget and fell back to the stream wait (``fallback``), the stalled looks (``looks``) and
        the entries whose first look found them not yet there (``late_entries``)."""
        o = (C.c_int64 * 4)()
        _lib.check(_lib.lib().lt_host_landing_stats(self._h, o), "lt_host_landing_stats")
        p = (C.c_int64 * 4)()
        _lib.check(_lib.lib().lt_host_landing_stats2(self._h, p), "lt_host_landing_stats2")
        return {"early": int(o[0]), "late": int(o[1]), "post_ns": int(o[2]), "mismatch": int(o[3]),
                "polled": int(p[0]), "fallback": int(p[1]), "looks": int(p[2]), "late_entries": int(p[3])}

    def influence_rows_vec(self, probes: torch.Tensor, obs: torch.Tensor, delta: float, m: int, out: torch.Tensor,
                           vec: torch.Tensor) -> torch.Tensor:
        """lt_influence_rows_vec (a slice of a wide model, ``WideBaseline``): the norms into ``out`` and the pairs' unscaled
        difference vectors into ``vec`` ([n_probe, n_obs, C] dense in the storage of ``vec``).  Device int32 node tensors."""
        if m == _lib.MODE_DELTA and not self._fp64:
            self.enable_fp64()
        npb, nob = probes.numel(), obs.numel()
        if vec.numel() < npb * nob * self.c or vec.dtype != torch.float32 or not vec.is_contiguous():
            raise ValueError("vec must be a contiguous float32 tensor of at least n_probe * n_obs * C elements")
        ws = self._workspace((npb, nob, m), _lib.lib().lt_influence_workspace_bytes(self._h, npb, nob, m))
        _lib.check(_lib.lib().lt_influence_rows_vec(self._h, probes.data_ptr(), npb, obs.data_ptr(), nob, float(delta), m,
                                                    out.data_ptr(), nob, vec.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                   "lt_influence_rows_vec")
        return vec


class WideBaseline:
    """The probe primitive for 2-layer models wider than one pass of the fused kernels (hidden width > 256 or more than 8
    classes; the reference has no such limit: gcn/layers.py:14-36, main.py:30 --hidden).  Same interface as ``Baseline``.

    A perturbation reaches the logits as a SUM over the hidden units, so the model is served slice by slice: for every slice
    s of <= 256 hidden units and every slice t of <= 8 classes a ``Baseline`` on (W1[:, s], b1[s], W2[s, t], b2[t]) whose
    ``lt_influence_rows_vec`` call yields the pairs' difference vectors, and per class slice one ``lt_wide_combine`` that adds
    the hidden slices' vectors in slice order, divides by delta and accumulates the squared norm over the classes in class
    order (include/linkteller_hip.h).  All three modes: `sparse` (= `full`: per slice the fp32 finite difference of the
    slice's own forward, exact zeros outside the 2-hop set) and `delta` (the exact propagation, fp64 kink test per slice).
    ~5 launches per (s, t) per matrix, independent of the number of probes (round 3 looped ~5 launches per PROBE and had
    no `delta`).  The fp32 product X W1[:, s] is formed once per hidden slice and shared by its class slices (round 6); the
    fp64 parts of `delta` are per (s, t)."""

    supports_sharding = False       # dist.choose_baseline_sharding: replicated on every rank, no timing loop
    VEC_BUDGET_BYTES = 256 << 20    # difference vectors of one probe chunk, all hidden slices together

    def __init__(self, adj, x, w1, b1, w2, b2):
        self.graph: HipGraph = as_hip_graph(adj)
        self.x, self.w1, self.b1, self.w2, self.b2 = (
            _f32(t, n) for t, n in ((x, "x"), (w1, "W1"), (b1, "b1"), (w2, "W2"), (b2, "b2")))
        n, f = self.x.shape
        self.n, self.f, self.h, self.c = n, f, self.w1.shape[1], self.w2.shape[1]
        if n != self.graph.n or self.w1.shape[0] != f or self.w2.shape[0] != self.h or self.b1.numel() != self.h or self.b2.numel() != self.c:
            raise ValueError("inconsistent GCN shapes")
        if self.graph.device_index != self.x.device.index:
            raise ValueError(f"the graph lives on cuda:{self.graph.device_index}, the features on {self.x.device}")
        _require_finite(features=self.x, W1=self.w1, b1=self.b1, W2=self.w2, b2=self.b2)
        self.h_slices = [(s0, min(s0 + 256, self.h)) for s0 in range(0, self.h, 256)]
        self.c_slices = [(t0, min(t0 + 8, self.c)) for t0 in range(0, self.c, 8)]
        if len(self.h_slices) > 32:
            raise NotImplementedError(f"hidden width {self.h}: more than 32 slices of 256 (lt_wide_combine)")
        self._subs = None           # [(s, t)] -> (Baseline, (W1 slice, b1 slice, W2 slice, b2 slice)); built on first use
        self._logits = None
        self._fp64 = False
        self._buf = {}

    def _build(self):
        if self._subs is not None:
            return
        subs = {}
        for si, (s0, s1) in enumerate(self.h_slices):
            for ti, (t0, t1) in enumerate(self.c_slices):
                parts = (self.w1[:, s0:s1].contiguous(), self.b1[s0:s1].contiguous(),
                         self.w2[s0:s1, t0:t1].contiguous(), self.b2[t0:t1].contiguous())
                subs[(si, ti)] = (Baseline(self.graph, self.x, *parts), parts)
        self._subs = subs
        # ONE product X W1[:, s] per hidden slice, shared by the slice's class slices (a 121-class model has 16 of them): every
        # (s, t) baseline reads S1 from the slice's torch-owned storage (lt_baseline_attach_s1), the first class slice's
        # baseline forms it there (lt_baseline_refresh_rows over all rows), the others are told it is current
        self._s1 = {}
        for si, (s0, s1) in enumerate(self.h_slices):
            hp = (s1 - s0 + 3) // 4 * 4
            t = torch.zeros((self.n, hp), dtype=torch.float32, device=self.x.device)
            self._s1[si] = t
            for ti in range(len(self.c_slices)):
                sub = subs[(si, ti)][0]
                # (marked current first: attaching copies the baseline's own S1 over, and none has been formed yet)
                _refresh_handle(sub, "lt_baseline_refresh_rows", 0, 0, t.data_ptr())
                _lib.check(_lib.lib().lt_baseline_attach_s1(sub._h, t.data_ptr(), hp, _stream()), "lt_baseline_attach_s1")
                sub._s1_full = t
        self._share_products()

    def _share_products(self):
        for si in range(len(self.h_slices)):
            t = self._s1[si]
            for ti in range(len(self.c_slices)):
                sub = self._subs[(si, ti)][0]
                _refresh_handle(sub, "lt_baseline_refresh_rows", 0, self.n if ti == 0 else 0, t.data_ptr())

    def refresh(self, mode=None):
        """The borrowed inputs changed: the slices are re-cut from them, everything derived is recomputed on next use."""
        self._logits = None
        if self._subs is None:
            return
        for (si, ti), (sub, (w1s, b1s, w2s, b2s)) in self._subs.items():
            (s0, s1), (t0, t1) = self.h_slices[si], self.c_slices[ti]
            w1s.copy_(self.w1[:, s0:s1]); b1s.copy_(self.b1[s0:s1])
            w2s.copy_(self.w2[s0:s1, t0:t1]); b2s.copy_(self.b2[t0:t1])
        m = _lib.MODES[mode] if isinstance(mode, str) else mode
        if m == _lib.MODE_DELTA and all(sub._fp64 for sub, _ in self._subs.values()):
            # `delta` reads the fp64 pre-activation only: no fp32 X W1[:, s] at all (75 us per hidden slice at twitch size, half of a
            # 0.34 ms build with H = 512) -- every slice is marked stale, and an fp32 reader that comes later recomputes lazily
            for sub, _ in self._subs.values():
                _refresh_handle(sub, "lt_baseline_refresh")
        else:
            self._share_products()      # (marks every slice's layers and fp64 parts stale as lt_baseline_refresh does)

    def features_changed(self):
        """``Baseline.features_changed`` for every slice's baseline, then ``refresh()``."""
        if self._subs is not None:
            for sub, _ in self._subs.values():
                sub.features_changed()
        self.refresh()
        return self

    def shard_refresh(self, enable=True):
        return self

    shard_refresh_fp64 = shard_refresh

    def enable_fp64(self):
        self._fp64 = True
        return self

    def fp64_route(self) -> int:
        return -1

    def logits(self) -> torch.Tensor:
        """GraphConvolution.forward x 2 on the unfused HIP layers (gcn/layers.py:30-36: any width)."""
        if self._logits is None:
            h1 = spmm(self.graph, gemm(self.x, self.w1), self.b1, relu=True)
            self._logits = spmm(self.graph, gemm(h1, self.w2), self.b2)
        return self._logits.clone()

    def influence_rows(self, probe_nodes, observe_nodes, delta: float, mode="delta", out=None) -> torch.Tensor:
        m = _lib.MODES[mode or "delta"] if isinstance(mode, str) or mode is None else int(mode)
        if m == _lib.MODE_FULL:
            m = _lib.MODE_SPARSE            # the same quantity, bit for bit (lt_influence_rows_vec has no FULL form)
        dev = self.x.device
        probes = _as_nodes(probe_nodes, self.n, dev, "probe_nodes")
        obs = _as_nodes(observe_nodes, self.n, dev, "observe_nodes")
        npb, nob = probes.numel(), obs.numel()
        if out is None:
            out = torch.empty((npb, nob), dtype=torch.float32, device=dev)
        elif out.shape != (npb, nob) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 [n_probe, n_obs] tensor")
        if npb == 0 or nob == 0:
            return out
        self._build()
        n_s = len(self.h_slices)
        # probes in chunks: the slices' difference vectors ([chunk, n_obs, 8] fp32 per hidden slice) stay within a fixed budget
        # (unchunked they took n_slices x n_probe x n_obs x 32 bytes -- 16 GB at 4096^2 pairs and 32 slices)
        chunk = max(1, min(npb, self.VEC_BUDGET_BYTES // (n_s * nob * 8 * 4)))
        key = (chunk, nob)
        if self._buf.get("key") != key:
            self._buf = {"key": key, "norm": torch.empty((chunk, nob), dtype=torch.float32, device=dev),
                         "vec": [torch.empty((chunk, nob, 8), dtype=torch.float32, device=dev) for _ in self.h_slices]}
        ptrs = (C.c_void_p * n_s)()
        for p0 in range(0, npb, chunk):
            pc = probes[p0:p0 + chunk]
            nb = pc.numel()
            orow = out[p0:p0 + nb]
            for ti, (t0, t1) in enumerate(self.c_slices):
                ct = t1 - t0
                for si in range(n_s):
                    sub = self._subs[(si, ti)][0]
                    if m == _lib.MODE_DELTA:
                        sub.enable_fp64()
                    vec = self._buf["vec"][si]          # used as [nb, nob, ct] dense
                    sub.influence_rows_vec(pc, obs, delta, m, self._buf["norm"], vec)
                    ptrs[si] = vec.data_ptr()
                _lib.check(_lib.lib().lt_wide_combine(ptrs, n_s, nb * nob, ct, float(delta), orow.data_ptr(), int(ti == 0),
                                                      int(ti == len(self.c_slices) - 1), _stream()), "lt_wide_combine")
        return out


class _ValidationMixin:
    """Per-epoch validation of a GPU trainer (lt_gcn*_trainer_attach_validation / _run_validated / _val_state / _restore_best /
    _val_logits): after every optimiser step the held-out graph is forwarded with dropout off, the evaluation head leaves the
    mean loss and the C x C confusion counts, the early-stopping state (EarlyStopping with delta = 0, kept in device memory)
    takes the loss, and with ``keep_best`` a predicated launch copies the parameters when the epoch improved -- all enqueued
    behind the epoch, no host round trip.  ``_PREFIX`` names the C entry points."""

    _PREFIX = ""
    _val = None
    _WIDE = False     # GCN2Trainer / GCN3Trainer(head="wide"): val_counts are [C, 3] = (tp, fp, fn) per class instead of the C x C confusion

    def _count_cols(self):
        return 3 if self._WIDE else self.c

    def _call(self, name, *args):
        fn = f"{self._PREFIX}_{name}"
        _lib.check(getattr(_lib.lib(), fn)(self._h, *args), fn)

    def attach_validation(self, adj2, x2, labels2, keep_best=False, patience=0, rows=None):
        """Attach the held-out graph (reference: ``features_2``, ``adj_2``, ``labels_2``); once per trainer.  ``keep_best``: keep a
        snapshot of the parameters of the best validation loss (``restore_best``).  ``patience`` > 0: stop ``run_validated``
        after that many epochs without improvement; 0: never stop.  ``rows`` (a tensor or an array of node ids of the held-out
        graph, any order, repeats count): the head scores these rows only (the reference's ``idx_val`` of a dataset with one
        graph and a split of its nodes, gcn_trainer.py:183-196); an id outside [0, n2) raises ``IndexError``."""
        if self._val is not None:
            raise ValueError("validation is already attached to this trainer")
        if int(patience) < 0:
            raise ValueError(f"patience must be >= 0, got {patience}")
        g2: HipGraph = as_hip_graph(adj2)
        x2 = _f32(x2, "x2")
        if x2.dim() != 2 or x2.shape[1] != self.f:
            raise ValueError(f"x2 must be [n2, {self.f}], got {tuple(x2.shape)}")
        if x2.shape[0] != g2.n:
            raise ValueError(f"x2 has {x2.shape[0]} rows, the validation graph {g2.n} nodes")
        if g2.device_index != self.x.device.index or x2.device != self.x.device:
            raise ValueError(f"the trainer lives on {self.x.device}: the validation graph is on cuda:{g2.device_index}, "
                             f"x2 on {x2.device}")
        _require_finite(features_2=x2)
        labels2 = self._prepare_labels(labels2, g2.n, "labels2")
        if self._WIDE:
            if rows is not None:
                rows = _as_rows(rows, g2.n, self.x.device, "rows")
                if rows.numel() == 0:
                    raise ValueError("rows is empty: a validation loss over no row is undefined")
            self._call("attach_validation_wide", g2.handle, x2.data_ptr(), x2.shape[1], x2.shape[0], labels2.data_ptr(),
                       labels2.shape[1] if labels2.dim() == 2 else 0, int(bool(keep_best)), int(patience),
                       None if rows is None else rows.data_ptr(), 0 if rows is None else rows.numel(), _stream())
        elif rows is None:
            self._call("attach_validation", g2.handle, x2.data_ptr(), x2.shape[1], x2.shape[0], labels2.data_ptr(),
                       int(bool(keep_best)), int(patience), _stream())
        else:
            rows = _as_rows(rows, g2.n, self.x.device, "rows")
            if rows.numel() == 0:
                raise ValueError("rows is empty: a validation loss over no row is undefined")
            self._call("attach_validation_rows", g2.handle, x2.data_ptr(), x2.shape[1], x2.shape[0], labels2.data_ptr(),
                       int(bool(keep_best)), int(patience), rows.data_ptr(), rows.numel(), _stream())
        self._val = (g2, x2, labels2, rows)       # borrowed by the library: kept alive here
        self.n2, self.keep_best, self.patience = g2.n, bool(keep_best), int(patience)

    def _require_val(self):
        if self._val is None:
            raise ValueError("no validation attached: call attach_validation() first")

    def run_validated_async(self, epochs: int):
        """Enqueue ``epochs`` validated epochs without syncing; returns the device tensors (record [epochs, 2], val_loss
        [epochs], val_counts [epochs, C, C]; [epochs, C, 3] = (tp, fp, fn) per class with the wide head)."""
        self._require_val()
        k, dev = max(int(epochs), 0), self.x.device
        record = torch.empty((k, 2), dtype=torch.float32, device=dev)
        val_loss = torch.empty((k,), dtype=torch.float32, device=dev)
        val_counts = torch.empty((k, self.c, self._count_cols()), dtype=torch.int32, device=dev)
        self._call("run_validated", int(epochs), record.data_ptr(), val_loss.data_ptr(), val_counts.data_ptr(), _stream())
        for p in self.params:
            torch.autograd.graph.increment_version(p)
        return record, val_loss, val_counts

    def run_validated(self, epochs: int, chunk=None) -> dict:
        """Run up to ``epochs`` validated epochs.  Returns a dict of CPU arrays ``loss``, ``correct`` (the train record),
        ``val_loss`` [k] float32 and ``val_counts`` [k, C, C] int32 (row = true class, column = predicted; the trace is the
        correct count), and the ints ``best_epoch`` and ``stop_epoch`` (0-based, counted since the trainer was created;
        ``stop_epoch`` is -1 when the run did not stop).  With ``patience`` > 0 the epochs are enqueued ``chunk`` at a time
        (default: the patience, the fewest epochs after which a stop is possible) and the 32-byte state is read after each
        chunk; the run ends at a stop and the arrays are cut behind the stop epoch.  Epochs of a chunk behind the stop have
        run (they moved the live parameters) but neither state nor snapshot: the result does not depend on ``chunk``."""
        self._require_val()
        epochs = max(int(epochs), 0)
        if self.patience > 0:
            chunk = self.patience if chunk is None else int(chunk)
            if chunk <= 0:
                raise ValueError(f"chunk must be positive, got {chunk}")
        else:
            chunk = max(epochs, 1)
        first, parts, done = self.epoch, [], 0
        state = self.val_state()
        while done < epochs and state["stop_epoch"] < 0:
            k = min(chunk, epochs - done)
            parts.append(self.run_validated_async(k))
            done += k
            state = self.val_state()
        keep = done if state["stop_epoch"] < 0 else min(done, state["stop_epoch"] + 1 - first)
        cat = (lambda i, shape, dt: torch.cat([p[i] for p in parts])[:keep].cpu().numpy() if parts
               else torch.empty(shape, dtype=dt).numpy())
        rec = cat(0, (0, 2), torch.float32)
        return {"loss": rec[:, 0].copy(), "correct": rec[:, 1].astype("int64"), "val_loss": cat(1, (0,), torch.float32),
                "val_counts": cat(2, (0, self.c, self._count_cols()), torch.int32), "best_epoch": state["best_epoch"],
                "stop_epoch": state["stop_epoch"]}

    def val_state(self) -> dict:
        """The early-stopping state (synchronises): ``best_loss`` (float; ``best_loss_bits`` its fp32 bits), ``best_epoch``,
        ``counter``, ``stop_epoch`` (-1 while running), ``improved``, ``seen``."""
        self._require_val()
        words = (C.c_int32 * 8)()
        self._call("val_state", words, _stream())
        w = [int(v) for v in words]
        import struct
        return {"best_loss": struct.unpack("<f", struct.pack("<i", w[0]))[0], "best_loss_bits": w[0] & 0xffffffff,
                "best_epoch": w[1], "counter": w[2], "stop_epoch": w[3], "improved": w[4], "seen": w[5]}

    def restore_best(self):
        """Copy the snapshot of the best epoch into the live parameters (needs ``keep_best``)."""
        self._require_val()
        if not self.keep_best:
            raise ValueError("restore_best() needs attach_validation(..., keep_best=True)")
        self._call("restore_best", _stream())
        for p in self.params:
            torch.autograd.graph.increment_version(p)

    def val_logits(self) -> torch.Tensor:
        """The last validated epoch's logits on the held-out graph [n2, C] (eval mode, after that epoch's update)."""
        self._require_val()
        out = torch.empty((self.n2, self.c), dtype=torch.float32, device=self.x.device)
        self._call("val_logits", out.data_ptr(), self.c, _stream())
        return out


def eval_head(logits: torch.Tensor, labels: torch.Tensor, rows=None):
    """Mean cross-entropy (device float32 scalar tensor) and confusion matrix (int32 [C, C], row = true class, column = first
    argmax) of ``logits`` [n, C] -- a strided view with unit column stride is read in place -- against ``labels``
    (lt_eval_head).  Enqueue-only.  With ``rows`` (a tensor or an array of row ids, any order, repeats count) only the listed
    rows are scored: ``F.cross_entropy(logits[rows], labels[rows])`` without the gathered copies (lt_eval_head_rows); the ids
    are checked first (a synchronisation when they live on the device) and one outside [0, n) raises ``IndexError``."""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2):
        raise ValueError("logits must be a 2-d float32 device tensor")
    n, c = logits.shape
    if n and (logits.stride(1) != 1 or logits.stride(0) < c):
        logits = logits.contiguous()
    labels = labels.reshape(-1).to(device=logits.device, dtype=torch.int32).contiguous()
    if labels.numel() != n:
        raise ValueError(f"labels: {labels.numel()} entries for {n} rows")
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    conf = torch.empty((c, c), dtype=torch.int32, device=logits.device)
    if rows is not None:
        rows = _as_rows(rows, n, logits.device, "rows")
        m = rows.numel()
        ws = _workspace(_lib.lib().lt_eval_head_rows_workspace_bytes(m, c), logits.device)
        _lib.check(_lib.lib().lt_eval_head_rows(logits.data_ptr(), logits.stride(0) if n else c, labels.data_ptr(), n, c,
                                                rows.data_ptr(), m, loss.data_ptr(), conf.data_ptr(), None, ws.data_ptr(),
                                                ws.numel(), _stream()), "lt_eval_head_rows")
        return loss, conf
    ws = _workspace(_lib.lib().lt_eval_head_workspace_bytes(n, c), logits.device)
    _lib.check(_lib.lib().lt_eval_head(logits.data_ptr(), logits.stride(0) if n else c, labels.data_ptr(), n, c, loss.data_ptr(),
                                       conf.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "lt_eval_head")
    return loss, conf


def f1_from_confusion(conf):
    """(micro, macro, weighted) F1 in float64 from C x C integer counts (row = true class, column = predicted class), with the
    conventions of ``sklearn.metrics.f1_score`` on the labels present (reference gcn_trainer.py:354-383 calls it three times): a
    class with no true and no predicted member is left out of the macro mean, a zero division gives 0, the weights are the
    supports."""
    import numpy as np
    k = conf.detach().cpu().numpy() if isinstance(conf, torch.Tensor) else np.asarray(conf)
    if k.ndim != 2 or k.shape[0] != k.shape[1]:
        raise ValueError(f"conf must be [C, C], got {k.shape}")
    k = k.astype(np.int64)
    tp, true, pred = np.diag(k), k.sum(axis=1), k.sum(axis=0)
    total = int(k.sum())
    micro = float(tp.sum()) / total if total else 0.0      # single label: micro F1 = accuracy (sum fp = sum fn)
    den = true + pred                                       # F1_c = 2 tp / (2 tp + fp + fn) = 2 tp / (true + pred)
    f1 = np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)
    present = den > 0
    macro = float(f1[present].mean()) if present.any() else 0.0
    weighted = float((f1 * true).sum() / total) if total else 0.0
    return micro, macro, weighted


def eval_head_wide(output: torch.Tensor, labels: torch.Tensor, rows=None, loss="ce"):
    """Loss (device float32 scalar tensor) and counts (int32 [C, 3] = (tp, fp, fn) per class) of ``output`` [n, C], C <= 256
    (lt_eval_head_wide).  ``loss="ce"``: ``labels`` [n], mean cross-entropy, prediction = first argmax; ``loss="bce"``:
    ``labels`` [n, C] of 0 / 1, mean binary cross-entropy with logits over all elements, predicted positive iff the logit
    is > 0.  ``rows``: only the listed rows, repeats counting (an id outside [0, n) raises ``IndexError``).  Enqueue-only."""
    if not (isinstance(output, torch.Tensor) and output.is_cuda and output.dtype == torch.float32 and output.dim() == 2):
        raise ValueError("output must be a 2-d float32 device tensor")
    if loss not in GCN2Trainer._LOSSES:
        raise ValueError(f"loss must be 'ce' or 'bce', got {loss!r}")
    n, c = output.shape
    if n and (output.stride(1) != 1 or output.stride(0) < c):
        output = output.contiguous()
    if not isinstance(labels, torch.Tensor):
        labels = torch.as_tensor(labels)
    if loss == "bce":
        if labels.dim() != 2 or labels.shape[0] != n or labels.shape[1] != c:
            raise ValueError(f"labels must be [{n}, {c}] for loss='bce', got {tuple(labels.shape)}")
        labels = labels.to(device=output.device)
        if labels.dtype != torch.uint8 or labels.stride(1) != 1 or labels.stride(0) < c:
            labels = labels.to(torch.uint8).contiguous()
        ldy = labels.stride(0)
    else:
        labels = labels.reshape(-1).to(device=output.device, dtype=torch.int32).contiguous()
        if labels.numel() != n:
            raise ValueError(f"labels: {labels.numel()} entries for {n} rows")
        ldy = 0
    out_loss = torch.empty((), dtype=torch.float32, device=output.device)
    counts = torch.empty((c, 3), dtype=torch.int32, device=output.device)
    m = 0
    if rows is not None:
        rows = _as_rows(rows, n, output.device, "rows")
        m = rows.numel()
    ws = _workspace(_lib.lib().lt_eval_head_wide_workspace_bytes(m if rows is not None else n, c), output.device)
    _lib.check(_lib.lib().lt_eval_head_wide(output.data_ptr(), output.stride(0) if n else c, labels.data_ptr(), ldy, n, c,
                                            GCN2Trainer._LOSSES[loss], None if rows is None else rows.data_ptr(), m,
                                            out_loss.data_ptr(), counts.data_ptr(), None, ws.data_ptr(), ws.numel(), _stream()),
               "lt_eval_head_wide")
    return out_loss, counts


def f1_from_counts(counts, present_only=False):
    """(micro, macro, weighted) F1 as Python floats from integer counts [C, 3] = (tp, fp, fn) per class, single- or
    multi-label, with ``sklearn.metrics.f1_score``'s arithmetic over all C classes: per class 2 tp / (2 tp + fp + fn), 0 where
    that denominator is 0; macro their mean; weighted by the supports tp + fn (0 when there is none); micro from the summed
    counts.  ``present_only``: the macro mean leaves out the classes that are neither a label nor a prediction, as
    ``f1_score`` does on single-label inputs when it is not told the class list (reference gcn_trainer.py:246-252)."""
    import numpy as np
    k = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    if k.ndim != 2 or k.shape[1] != 3:
        raise ValueError(f"counts must be [C, 3], got {k.shape}")
    k = k.astype(np.int64)
    tp, fp, fn = k[:, 0], k[:, 1], k[:, 2]
    den = 2 * tp + fp + fn
    f1 = np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)
    support = tp + fn
    den_all = int(den.sum())
    micro = 2.0 * int(tp.sum()) / den_all if den_all else 0.0
    in_mean = f1[den > 0] if present_only else f1
    macro = float(in_mean.mean()) if in_mean.size else 0.0
    weighted = float((f1 * support).sum() / support.sum()) if support.sum() else 0.0
    return float(micro), macro, weighted


class EarlyStopState:
    """The early-stopping state block on its own (lt_early_stop_reset / lt_early_stop_update): 8 int32 words of device memory."""

    def __init__(self, patience: int, device="cuda"):
        if int(patience) < 0:
            raise ValueError(f"patience must be >= 0, got {patience}")
        self.patience = int(patience)
        self.words = torch.empty(8, dtype=torch.int32, device=device)
        _lib.check(_lib.lib().lt_early_stop_reset(self.words.data_ptr(), _stream()), "lt_early_stop_reset")

    def update(self, loss: torch.Tensor, epoch: int):
        """Apply one epoch's loss (a float32 device tensor of one element); enqueue-only."""
        if not (loss.is_cuda and loss.dtype == torch.float32 and loss.numel() == 1):
            raise ValueError("loss must be a float32 device tensor of one element")
        _lib.check(_lib.lib().lt_early_stop_update(loss.data_ptr(), self.patience, int(epoch), self.words.data_ptr(), _stream()),
                   "lt_early_stop_update")

    def read(self):
        """The 8 words as a CPU int32 array (synchronises)."""
        return self.words.cpu().numpy()


class _GCNTrainer(_ValidationMixin):
    """What ``GCN2Trainer`` and ``GCN3Trainer`` share: the constructor's checks, driven by the class's parameter names, and the
    accessors, which reach the C entry points through ``_PREFIX``.  The parameters are updated IN PLACE (their version counters
    are bumped after every ``run``); the trainer owns the Adam moments.  Dropout is a Philox4x32-10 mask keyed by ``seed``, the
    epoch counter and the hidden layer (include/linkteller_hip.h), so it can be rebuilt exactly; it is not torch's generator.
    Limits: hidden widths <= 256, classes <= 8 (``head="wide"``: <= 256)."""

    _NAMES = ()       # the parameter tensors in model order; each becomes the attribute of its lower-case name
    _MODEL = ""       # the model's name in the shape error
    _LOSSES = {"ce": 0, "bce": 1}      # LT_LOSS_CE, LT_LOSS_BCE
    head, loss = "narrow", "ce"

    def _set_head(self, head, loss):
        """The ``head`` / ``loss`` arguments of both trainers, checked before anything touches the device."""
        if head not in ("narrow", "wide"):
            raise ValueError(f"head must be 'narrow' or 'wide', got {head!r}")
        if loss not in self._LOSSES:
            raise ValueError(f"loss must be 'ce' or 'bce', got {loss!r}")
        if head == "narrow" and loss != "ce":
            raise ValueError("the narrow head has the cross-entropy loss only: pass head='wide' for loss='bce'")
        self._WIDE, self.head, self.loss = head == "wide", head, loss

    def __init__(self, adj, x, labels, params, *, lr, weight_decay, dropout, seed, train_rows=None):
        if not 0.0 <= float(dropout) <= 1.0:      # F.dropout's message
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout}")
        self.graph: HipGraph = as_hip_graph(adj)
        self.x = _f32(x, "x")
        self.params = [_f32(t, n) for t, n in zip(params, self._NAMES)]
        for t, src in zip(self.params, params):
            if t.data_ptr() != src.data_ptr():
                raise ValueError("the parameters are updated in place: pass contiguous float32 device tensors")
        for name, t in zip(self._NAMES, self.params):
            setattr(self, name.lower(), t)
        n, f = self.x.shape
        dims = [f] + [w.shape[1] for w in self.params[0::2]]      # layer l maps dims[l] to dims[l + 1] columns
        self.n, self.f, self.c = n, f, dims[-1]
        if n != self.graph.n or any(w.shape != (dims[l], dims[l + 1]) or b.shape != (dims[l + 1],)
                                    for l, (w, b) in enumerate(zip(self.params[0::2], self.params[1::2]))):
            raise ValueError(f"inconsistent {self._MODEL} shapes")
        if self.graph.device_index != self.x.device.index:
            raise ValueError(f"the graph lives on cuda:{self.graph.device_index}, the features on {self.x.device}")
        _require_finite(features=self.x, **dict(zip(self._NAMES, self.params)))
        self.labels = self._prepare_labels(labels, n, "labels")
        h = C.c_void_p()
        fn, label_args = self._create_call()
        _lib.check(getattr(_lib.lib(), fn)(self.graph.handle, self.x.data_ptr(), f, f, *label_args, *dims[1:],
                                           *[t.data_ptr() for t in self.params], float(lr), float(weight_decay),
                                           float(dropout), int(seed) & (2**64 - 1), _stream(), C.byref(h)), fn)
        self._h = h
        self._finalizer = weakref.finalize(self, getattr(_lib.lib(), f"{self._PREFIX}_destroy"), h)
        self.n_train = n
        if train_rows is not None:
            self.set_train_rows(train_rows)

    def set_train_rows(self, rows):
        """Train on the listed rows only (lt_gcn*_trainer_set_train_rows; the reference's transductive loss,
        ``model(features, adj)[idx_train]``, gcn_trainer.py:150-156): the whole graph is forwarded, the loss is the mean over
        the listed rows, every other row's gradient of the logits is zero, and ``run``'s second value and ``counts()`` count
        the listed rows.  ``rows``: a 1-d list, array or tensor of any integer dtype, distinct ids in [0, n), any order; ``None``
        restores all rows.  Checked here, before the library is called: ``IndexError`` for ids outside the graph, ``ValueError``
        for repeated ids, a float dtype, another dimension or an empty list; the trainer is then as it was.  May be called
        between runs, before or after ``attach_validation``; validation does not see the list.  Waits for the stream."""
        if rows is None:
            self._call("set_train_rows", None, 0, _stream())
            self.n_train = self.n
            return
        t = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(rows)
        if t.numel() == 0:      # (before the dtype: an empty Python list arrives as float32)
            raise ValueError("train_rows is empty: a loss over no row is undefined (None trains on all rows)")
        if t.dtype.is_floating_point or t.dtype == torch.bool or t.is_complex():
            raise ValueError(f"train_rows must hold integer ids, got {t.dtype}")
        if t.dim() != 1:
            raise ValueError(f"train_rows must be 1-d, got {tuple(t.shape)}")
        t = t.detach().to(device="cpu", dtype=torch.int64)
        outside = int(((t < 0) | (t >= self.n)).sum())
        if outside:
            raise IndexError(f"train_rows: {outside} ids outside the graph [0, {self.n})")
        repeated = t.numel() - int(torch.unique(t).numel())
        if repeated:
            raise ValueError(f"train_rows: {repeated} ids repeat an earlier one")
        host = t.to(torch.int32).contiguous()      # the library copies it before the call returns
        self._call("set_train_rows", host.data_ptr(), host.numel(), _stream())
        self.n_train = host.numel()

    def _prepare_labels(self, labels, n, name):
        """One class id per node as the int32 device tensor the library borrows; for the wide head with ``loss="bce"`` the
        [n, C] matrix of 0 / 1 as uint8."""
        if not isinstance(labels, torch.Tensor):
            labels = torch.as_tensor(labels)
        if self._WIDE and self.loss == "bce":
            if labels.dim() != 2 or tuple(labels.shape) != (n, self.c):
                raise ValueError(f"{name} must be [{n}, {self.c}] for loss='bce', got {tuple(labels.shape)}")
            if labels.is_floating_point() or labels.is_complex():
                raise ValueError(f"{name} must have an integer or bool dtype, got {labels.dtype}")
            if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) > 1):
                raise ValueError(f"{name} must hold 0 / 1")
            return labels.to(device=self.x.device, dtype=torch.uint8).contiguous()
        labels = labels.reshape(-1)
        if labels.numel() != n:
            raise ValueError(f"{name}: {labels.numel()} entries for {n} nodes")
        if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= self.c):
            raise ValueError(f"{name} outside [0, {self.c})")
        return labels.to(device=self.x.device, dtype=torch.int32).contiguous()

    def _create_call(self):
        """The create entry point's name and its arguments between ``F`` and the widths."""
        if self._WIDE:
            return f"{self._PREFIX}_create_wide", (self.labels.data_ptr(), self.c, self._LOSSES[self.loss])
        return f"{self._PREFIX}_create", (self.labels.data_ptr(),)

    def counts(self) -> torch.Tensor:
        """The last epoch's int32 [C, 3] = (tp, fp, fn) per class on the training rows (wide head only)."""
        if not self._WIDE:
            raise ValueError("counts() needs head='wide'")
        out = torch.empty((self.c, 3), dtype=torch.int32, device=self.x.device)
        self._call("counts", out.data_ptr(), _stream())
        return out

    @property
    def epoch(self) -> int:
        e = C.c_int64()
        self._call("epoch", C.byref(e))
        return e.value

    def run_async(self, epochs: int) -> torch.Tensor:
        """Enqueue ``epochs`` epochs; returns the device record [epochs, 2] (mean loss, correct count) without syncing."""
        record = torch.empty((max(int(epochs), 0), 2), dtype=torch.float32, device=self.x.device)
        self._call("run", int(epochs), record.data_ptr(), _stream())
        for p in self.params:
            torch.autograd.graph.increment_version(p)
        return record

    def run(self, epochs: int):
        """Run ``epochs`` epochs; returns (loss [epochs] float32, correct [epochs] int64) as CPU arrays (one read at the end);
        with ``train_rows`` set both are over the listed rows."""
        rec = self.run_async(epochs).cpu().numpy()
        return rec[:, 0].copy(), rec[:, 1].astype("int64")

    def grads(self):
        """The last epoch's gradients (before weight decay), one per parameter in the constructor's order."""
        out = [torch.empty_like(p) for p in self.params]
        self._call("grads", *[t.data_ptr() for t in out], _stream())
        return tuple(out)

    def logits(self) -> torch.Tensor:
        """The last epoch's train-mode logits (dropout applied, before that epoch's update)."""
        out = torch.empty((self.n, self.c), dtype=torch.float32, device=self.x.device)
        self._call("logits", out.data_ptr(), self.c, _stream())
        return out


class GCN2Trainer(_GCNTrainer):
    """Training of the 2-layer GCN on the GPU (lt_gcn2_trainer_*): one epoch is the reference's ``train_one_epoch`` on a
    transfer dataset (gcn_trainer.py:144-170) -- forward with dropout, mean cross-entropy, backward, ``optim.Adam`` with
    weight decay -- as ~15 stream-ordered launches on torch's current stream and no host synchronisation.  ``w1, b1, w2, b2``
    are updated in place.  Validation every epoch, best-model snapshot and early stopping: ``attach_validation`` /
    ``run_validated`` (_ValidationMixin)."""

    _PREFIX, _NAMES, _MODEL = "lt_gcn2_trainer", ("W1", "b1", "W2", "b2"), "GCN"

    def __init__(self, adj, x, labels, w1, b1, w2, b2, *, lr, weight_decay, dropout, seed, head="narrow", loss="ce",
                 train_rows=None):
        """``train_rows``: ``set_train_rows`` at creation (``n_train`` = their number, or n).
        ``head="wide"`` (lt_gcn2_trainer_create_wide): up to 256 classes, the class layer as matrix products and the wide loss
        head; ``loss="ce"`` takes ``labels`` [n] (mean cross-entropy), ``loss="bce"`` takes ``labels`` [n, C] of 0 / 1 in any
        integer or bool dtype (mean binary cross-entropy with logits over all n C elements; kept as uint8 on the device).
        ``run`` then returns (loss, sum over the classes of tp): the correct count for ce.  ``head="narrow"`` (default) is the
        fused class layer for at most 8 classes with cross-entropy."""
        self._set_head(head, loss)
        super().__init__(adj, x, labels, (w1, b1, w2, b2), lr=lr, weight_decay=weight_decay, dropout=dropout, seed=seed,
                         train_rows=train_rows)
        self.h = self.w1.shape[1]

    def hidden(self) -> torch.Tensor:
        """The last epoch's hidden activations after ReLU and dropout, H1d [n, H]."""
        out = torch.empty((self.n, self.h), dtype=torch.float32, device=self.x.device)
        self._call("hidden", out.data_ptr(), self.h, _stream())
        return out


class GCN3Trainer(_GCNTrainer):
    """Training of the 3-layer GCN3 on the GPU (lt_gcn3_trainer_*): the epoch of ``GCN2Trainer`` behind one more hidden layer
    -- two hidden layers with independent Philox masks (the counter's layer word), the backward through the middle layer on
    the matrix cores, one Adam launch over the six tensors.  ``w1 .. b3`` are updated in place.  Validation as for
    ``GCN2Trainer`` (_ValidationMixin)."""

    _PREFIX, _NAMES, _MODEL = "lt_gcn3_trainer", ("W1", "b1", "W2", "b2", "W3", "b3"), "GCN3"

    def __init__(self, adj, x, labels, w1, b1, w2, b2, w3, b3, *, lr, weight_decay, dropout, seed, head="narrow", loss="ce",
                 train_rows=None):
        """``train_rows``, ``head`` and ``loss`` as for ``GCN2Trainer``: ``head="wide"`` (lt_gcn3_trainer_create_wide) puts the
        wide class layer and loss head, up to 256 classes with ``loss="ce"`` or ``"bce"``, behind the two hidden layers; both
        heads draw the same two dropout masks from one seed.  ``counts()`` and the [C, 3] ``val_counts`` follow."""
        self._set_head(head, loss)
        super().__init__(adj, x, labels, (w1, b1, w2, b2, w3, b3), lr=lr, weight_decay=weight_decay, dropout=dropout, seed=seed,
                         train_rows=train_rows)
        self.h1, self.h2 = self.w1.shape[1], self.w2.shape[1]

    def hidden(self, layer: int) -> torch.Tensor:
        """The last epoch's hidden activations after ReLU and dropout: layer 1 -> H1d [n, H1], layer 2 -> H2d [n, H2]."""
        if layer not in (1, 2):
            raise ValueError(f"layer must be 1 or 2, got {layer}")
        width = self.h1 if layer == 1 else self.h2
        out = torch.empty((self.n, width), dtype=torch.float32, device=self.x.device)
        _lib.check(_lib.lib().lt_gcn3_trainer_hidden(self._h, int(layer), out.data_ptr(), width, _stream()),
                   "lt_gcn3_trainer_hidden")
        return out


def fused_shapes(h: int, c: int) -> bool:
    """What lt_baseline_create / lt_influence_rows are built for (one pass of the row kernels, fused layer-2 epilogue)."""
    return h <= 256 and c <= 8


def baseline_for(adj, x, w1, b1, w2, b2):
    """``Baseline`` (the fused probe primitive) when the layer widths allow it, else ``WideBaseline``."""
    return (Baseline if fused_shapes(w1.shape[1], w2.shape[1]) else WideBaseline)(adj, x, w1, b1, w2, b2)


class Baseline3(_ProbeHandle):
    """Unperturbed forward state of the 3-layer model (reference gcn/models.py:28-46) + its probe primitive
    (lt_baseline3_create / lt_influence3_rows): the reference's fp32 finite difference, evaluated on the rows a
    probe reaches in 1 / 2 / 3 hops.  More than 8 classes (up to 256) make a WIDE handle (lt_baseline3_create_wide,
    ``wide = True``): it serves ``mode="delta"`` alone, the fp32 finite difference of such a model is the attacker's loop."""

    NARROW_MAX_C = 8
    _SYM = _symbols("lt_baseline3", "lt_influence3", rows="lt_influence3_rows_mode")
    _DEFAULT_MODE = "sparse"

    def __init__(self, adj, x, w1, b1, w2, b2, w3, b3):
        _, _, self.h1, self.h2, self.c = self._take(adj, "inconsistent GCN3 shapes", x=x, W1=w1, b1=b1, W2=w2, b2=b2, W3=w3, b3=b3)
        self.wide = self.c > self.NARROW_MAX_C
        self._open("lt_baseline3_create_wide" if self.wide else "lt_baseline3_create")
        self._fp64 = False

    def refresh(self):
        _refresh_handle(self, "lt_baseline3_refresh")

    def enable_fp64(self):
        """fp64 pre-activations of the first two layers for the exact (`delta`) propagation (lt_baseline3_enable_fp64)."""
        if not self._fp64:
            _lib.check(_lib.lib().lt_baseline3_enable_fp64(self._h, _stream()), "lt_baseline3_enable_fp64")
            self._x_seen = _x_version(self.x)
            self._fp64 = True
        return self

    def _serves(self, m):
        if self.wide and m != _lib.MODE_DELTA:
            raise NotImplementedError(f"a GCN3 with {self.c} classes is served in mode 'delta' only (lt_baseline3_create_wide); "
                                      "its fp32 finite difference is Attacker._rows_generic")

    def influence_rows(self, probe_nodes, observe_nodes, delta: float, mode="sparse", out=None) -> torch.Tensor:
        """`sparse` (= `full`): the reference's fp32 finite difference on the rows a probe reaches in 1 / 2 / 3 hops;
        `delta`: the perturbation propagated exactly through the three layers (lt_influence3_rows_mode).  A wide handle
        serves ``delta`` alone."""
        return self._rows(probe_nodes, observe_nodes, delta, mode, out)


def wide_class_shapes(h: int, c: int) -> bool:
    """What ``Baseline2W`` is for: a 2-layer model whose hidden layer fits one pass of the row kernels and whose class layer
    does not fit the fused epilogue (reddit's 41 classes, ppi's 121 labels) but fits one lane group (lt_baseline2w_create)."""
    return h <= 256 and 9 <= c <= 256


class Baseline2W(_ProbeHandle):
    """The probe primitive of a 2-layer model with up to 256 classes as ONE handle (lt_baseline2w_create; H <= 256): `delta`
    alone -- the wide GCN3 chain with one level removed, one MFMA product over a probe chunk's items and a lane group across
    the class columns per (probe, observed) cell -- as a rectangle (``influence_rows``) and as a pair list
    (``influence_pairs``, the rectangle's bits).  `sparse` / `full` raise ``NotImplementedError``: the fp32 finite difference
    of these shapes is ``WideBaseline``'s.  The fp64 parts belong to the handle from creation (``enable_fp64`` is a no-op)."""

    supports_sharding = False       # dist.choose_baseline_sharding: replicated on every rank, no timing loop
    _SYM = _symbols("lt_baseline2w", "lt_influence2w")
    _fp64 = True

    def __init__(self, adj, x, w1, b1, w2, b2):
        _, _, self.h, self.c = self._take(adj, "inconsistent GCN shapes", x=x, W1=w1, b1=b1, W2=w2, b2=b2)
        self._open("lt_baseline2w_create")

    def refresh(self, mode=None):
        """The borrowed inputs changed: everything derived from them is re-formed by the next call that reads it."""
        _refresh_handle(self, "lt_baseline2w_refresh")

    def enable_fp64(self):
        return self

    def fp64_route(self) -> int:
        return -1

    def shard_refresh(self, enable=True):
        return self

    shard_refresh_fp64 = shard_refresh

    def _serves(self, m):
        if m != _lib.MODE_DELTA:
            raise NotImplementedError(f"a 2-layer model with {self.c} classes is served through this handle in mode 'delta' only "
                                      "(lt_baseline2w_create); its fp32 finite difference is engine.WideBaseline")

    def influence_rows(self, probe_nodes, observe_nodes, delta: float, mode="delta", out=None) -> torch.Tensor:
        """[n_probe, n_obs] fp32 on the device (lt_influence2w_rows): the perturbation propagated exactly through the two layers."""
        return self._rows(probe_nodes, observe_nodes, delta, mode, out)


def group_pairs(probe, observed):
    """Two equal-length id arrays in any order -> ``(probe_nodes, pair_ptr, pair_obs, order)``, the grouped layout of
    ``Baseline.influence_pairs`` (pure numpy, host only).  ``probe_nodes``: the distinct probes ascending (int32);
    ``pair_ptr``: int64 [len(probe_nodes) + 1]; ``pair_obs = observed[order]`` (int32), where ``order`` is the STABLE sort of the
    pairs by probe -- the pairs of one probe keep their input order, duplicates are kept.  Scores come back grouped; in input
    order they are ``scores = np.empty(len(order)); scores[order] = out``."""
    import numpy as np
    probe = np.asarray(probe, dtype=np.int64).reshape(-1)
    observed = np.asarray(observed, dtype=np.int64).reshape(-1)
    if probe.shape != observed.shape:
        raise ValueError(f"probe and observed differ in length: {probe.size} / {observed.size}")
    order = np.argsort(probe, kind="stable")
    nodes, counts = np.unique(probe, return_counts=True)
    pair_ptr = np.zeros(nodes.size + 1, dtype=np.int64)
    np.cumsum(counts, out=pair_ptr[1:])
    return nodes.astype(np.int32), pair_ptr, observed[order].astype(np.int32), order


def group_pairs_device(probe: torch.Tensor, observed: torch.Tensor, n: int = None):
    """``group_pairs`` on the device (lt_group_pairs): two equal-length int32 CUDA tensors of node ids -> ``(probe_nodes, pair_ptr,
    pair_obs, order)`` as CUDA tensors, equal to the host function's arrays element for element (``probe_nodes`` int32,
    ``pair_ptr`` int64, ``pair_obs`` int32, ``order`` int32: the stable sort of the pairs by probe).  ``n``: the ids lie in
    [0, n) (default: 2^31 - 1, four digit passes; the graph's node count saves passes).  The number of groups is the one word that
    comes to the host (one wait) to cut ``probe_nodes`` and ``pair_ptr``; ids outside [0, n) raise ``IndexError`` there.
    ``Baseline.influence_pairs`` takes the result as it is (its ``pair_ptr`` is copied to the host there)."""
    for t, name in ((probe, "probe"), (observed, "observed")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise _lib.LinkTellerHipError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
        if t.dtype != torch.int32 or t.dim() != 1:
            raise TypeError(f"{name} must be a 1-d int32 tensor, got {t.dtype} {tuple(t.shape)}")
    if probe.shape != observed.shape or probe.device != observed.device:
        raise ValueError(f"probe and observed differ in length or device: {probe.numel()} / {observed.numel()}")
    probe, observed = probe.contiguous(), observed.contiguous()
    m, dev = int(probe.numel()), probe.device
    if m < 1:
        raise ValueError("group_pairs_device: no pairs")
    n = (1 << 31) - 1 if n is None else int(n)
    need = _lib.lib().lt_group_pairs_workspace_bytes(m)
    if need == 0:
        raise ValueError(f"group_pairs_device: {m} pairs are outside what the library serves")
    ws = _workspace(need, dev)
    nodes = torch.empty(m, dtype=torch.int32, device=dev)
    ptr = torch.empty(m + 1, dtype=torch.int64, device=dev)
    obs = torch.empty(m, dtype=torch.int32, device=dev)
    order = torch.empty(m, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().lt_group_pairs(n, probe.data_ptr(), observed.data_ptr(), m, nodes.data_ptr(), ptr.data_ptr(),
                                             obs.data_ptr(), order.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                   "lt_group_pairs")
    groups, outside = [int(v) for v in info[:2].tolist()]
    if outside:
        raise IndexError(f"group_pairs_device: {outside} node ids outside [0, {n})")
    return nodes[:groups], ptr[:groups + 1], obs, order


_select_ws = {}      # top_pairs_lower's workspace: only the latest (device, size) is kept, sizes repeat across calls


def top_pairs_lower(scores: torch.Tensor, m: int):
    """The ``m`` highest-scoring cells (i, j), j < i, of an n x n fp32 score matrix on the device (lt_top_pairs_lower; the
    reference's ``np.argpartition(pred, -n_pos)[-n_pos:]``, attack_stats_all.py:106-116) -> ``(idx, score, info)``:
    ``idx`` int64 [m], the flat indices ``i * n + j`` in ascending order; ``score`` fp32 [m], the stored values at them;
    ``info``: ``threshold_bits`` (bit pattern of the m-th value), ``above``, ``tied_taken``, ``tied_total`` as 0-d int64 device
    tensors and all four as ``raw`` -- nothing is brought to the host here.  Cells are ranked by value descending, then flat index
    ascending (-0.0 as +0.0): a tied threshold -- the zeros of an influence matrix -- is cut at the same cells on every call.
    ``scores`` may be a view with a row stride > n (last-dimension stride 1); nothing outside the strict lower triangle is read."""
    if not isinstance(scores, torch.Tensor):
        raise TypeError("scores must be a torch.Tensor")
    if not scores.is_cuda:
        raise _lib.LinkTellerHipError(f"scores must live on the GPU (got {scores.device}); there is no CPU path")
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise TypeError(f"scores must be a square 2-d float32 tensor, got {scores.dtype} {tuple(scores.shape)}")
    n = int(scores.shape[0])
    if n > 1 and scores.stride(1) != 1:
        raise ValueError("scores must have last-dimension stride 1 (rows may be strided)")
    m = int(m)
    total = n * (n - 1) // 2
    if n < 2 or not 1 <= m <= total:
        raise ValueError(f"m={m} outside [1, {total}] for n={n}")
    lds = int(scores.stride(0))
    if lds < n:
        raise ValueError(f"row stride {lds} smaller than n={n}")
    dev = scores.device
    idx = torch.empty(m, dtype=torch.int64, device=dev)
    val = torch.empty(m, dtype=torch.float32, device=dev)
    raw = torch.empty(4, dtype=torch.int64, device=dev)
    need = _lib.lib().lt_top_pairs_workspace_bytes(n, m)
    key = (dev, need)
    ws = _select_ws.get(key)
    if ws is None:
        ws = _workspace(need, dev)
        _select_ws.clear()
        _select_ws[key] = ws
    _lib.check(_lib.lib().lt_top_pairs_lower(scores.data_ptr(), lds, n, m, idx.data_ptr(), val.data_ptr(), raw.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream()), "lt_top_pairs_lower")
    info = {"threshold_bits": raw[0], "above": raw[1], "tied_taken": raw[2], "tied_total": raw[3], "raw": raw}
    return idx, val, info


class TopPairsStream:
    """``top_pairs_lower`` over rows that arrive in chunks (lt_top_stream_*): the n x n matrix is never formed, the handle keeps
    O(m + slack) device state.  ``push(rows, row_begin)`` takes rows [row_begin, row_begin + rows.shape[0]) -- fp32 CUDA, last
    stride 1, at least ``row_begin + rows.shape[0] - 1`` columns; only columns 0 .. i - 1 of row i are read -- contiguously and in
    ascending order from row 0, at most ``max_rows`` a call.  ``finish()`` returns the ``(idx, score, info)`` of
    ``top_pairs_lower`` on the assembled matrix, byte for byte, whatever the cut into pushes or ``slack_cells`` (0 = default; at
    least 2 (n - 1)).  ``reset()`` readies the handle for another matrix of the same (n, m).  Nothing synchronises but the
    constructor.  ``device_bytes``: what the handle allocated (the formula stands in include/linkteller_hip.h)."""

    def __init__(self, n: int, m: int, max_rows: int, slack_cells: int = 0, device=None):
        n, m, max_rows, slack_cells = int(n), int(m), int(max_rows), int(slack_cells)
        total = n * (n - 1) // 2
        if n < 2 or not 1 <= m <= total:
            raise ValueError(f"m={m} outside [1, {total}] for n={n}")
        if max_rows < 1:
            raise ValueError(f"max_rows={max_rows} < 1")
        if slack_cells != 0 and slack_cells < 2 * (n - 1):
            raise ValueError(f"slack_cells={slack_cells} below the minimum 2 (n - 1) = {2 * (n - 1)} (0 = default)")
        _lib.require_gpu()
        self.n, self.m, self.max_rows = n, m, max_rows
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._h = None
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().lt_top_stream_create(n, m, max_rows, slack_cells, C.byref(h)), "lt_top_stream_create")
        self._h = h
        nbytes = C.c_size_t()
        _lib.check(_lib.lib().lt_top_stream_bytes(self._h, C.byref(nbytes)), "lt_top_stream_bytes")
        self.device_bytes = int(nbytes.value)

    def _handle(self):
        if self._h is None:
            raise _lib.LinkTellerHipError("TopPairsStream: the handle was closed")
        return self._h

    def push(self, rows: torch.Tensor, row_begin: int):
        if not isinstance(rows, torch.Tensor):
            raise TypeError("rows must be a torch.Tensor")
        if not rows.is_cuda:
            raise _lib.LinkTellerHipError(f"rows must live on the GPU (got {rows.device}); there is no CPU path")
        if rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[0] < 1:
            raise TypeError(f"rows must be a 2-d float32 tensor of at least one row, got {rows.dtype} {tuple(rows.shape)}")
        if rows.shape[1] > 1 and rows.stride(1) != 1:
            raise ValueError("rows must have last-dimension stride 1 (rows may be strided)")
        k, row_begin = int(rows.shape[0]), int(row_begin)
        if rows.shape[1] < row_begin + k - 1:
            raise ValueError(f"rows has {int(rows.shape[1])} columns, rows [{row_begin}, {row_begin + k}) need {row_begin + k - 1}")
        lds = int(rows.stride(0)) if k > 1 else max(int(rows.stride(0)), int(rows.shape[1]))
        if lds < row_begin + k - 1:
            raise ValueError(f"row stride {lds} smaller than the {row_begin + k - 1} columns read")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().lt_top_stream_push(self._handle(), rows.data_ptr(), lds, row_begin, k, _stream()), "lt_top_stream_push")

    def finish(self):
        idx = torch.empty(self.m, dtype=torch.int64, device=self.device)
        val = torch.empty(self.m, dtype=torch.float32, device=self.device)
        raw = torch.empty(4, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().lt_top_stream_finish(self._handle(), idx.data_ptr(), val.data_ptr(), raw.data_ptr(), _stream()),
                       "lt_top_stream_finish")
        info = {"threshold_bits": raw[0], "above": raw[1], "tied_taken": raw[2], "tied_total": raw[3], "raw": raw}
        return idx, val, info

    def reset(self):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().lt_top_stream_reset(self._handle(), _stream()), "lt_top_stream_reset")

    def stats(self) -> dict:
        """The handle's counters (one copy of 16 words, one wait): ``held``, ``seen`` cells, compactions that fired in front of
        the first slab of a push (``fired_between``) and of a later one (``fired_inside``), ``slabs``, ``tied_dropped``."""
        raw = torch.empty(16, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().lt_top_stream_stats(self._handle(), raw.data_ptr(), _stream()), "lt_top_stream_stats")
        w = [int(v) for v in raw.cpu().tolist()]
        return {"held": w[w[2] & 1], "seen": w[8], "fired_between": w[9], "fired_inside": w[10], "slabs": w[11],
                "threshold_set": bool(w[6]), "tied_dropped": w[7]}

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            _lib.lib().lt_top_stream_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pairs_present(csr, u, v) -> torch.Tensor:
    """uint8 CUDA tensor [len(u)]: 1 iff column ``v[k]`` is stored in row ``u[k]`` of the device pattern ``csr``
    (``sampling.device_pattern_csr``; lt_pairs_present: a binary search per pair).  ``u``, ``v``: integer CUDA tensors of equal
    length.  An id outside [0, n) raises ``IndexError`` (the call's own info word, read here: one wait); the node-id flag of the
    probe primitives is not touched."""
    rowptr, col = csr[0], csr[1]
    for name, t in (("u", u), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise _lib.LinkTellerHipError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
        if t.dtype.is_floating_point or t.dtype == torch.bool or t.is_complex() or t.dim() != 1:
            raise TypeError(f"{name} must be a 1-d tensor of integer ids, got {t.dtype} {tuple(t.shape)}")
    if u.numel() != v.numel():
        raise ValueError(f"u and v differ in length: {u.numel()} and {v.numel()}")
    _lib.require_gpu()
    dev = rowptr.device
    n = int(rowptr.numel()) - 1
    lim = torch.iinfo(torch.int32)

    def _ids(t):      # ids beyond int32 are out of range whatever n is: keep them out of range through the narrowing
        return t.contiguous() if t.dtype == torch.int32 else t.clamp(min=-1, max=lim.max).to(torch.int32)
    u32, v32 = _ids(u), _ids(v)
    out = torch.empty(u32.numel(), dtype=torch.uint8, device=dev)
    info = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().lt_pairs_present(n, rowptr.data_ptr(), col.data_ptr(), u32.data_ptr(), v32.data_ptr(), u32.numel(),
                                               out.data_ptr(), info.data_ptr(), _stream()), "lt_pairs_present")
    bad = int(info.item())
    if bad:
        raise IndexError(f"pairs_present: {bad} pairs name a node outside [0, {n})")
    return out


_curve_ws = {}       # score_curve's workspace: only the latest (device, size) is kept, sizes repeat across calls


class ScoreCurve:
    """What ``score_curve`` enqueued, still on the device: ``thresholds`` (fp32), ``tps``, ``fps`` (int64), each of capacity
    n_items with entries [0, D) written, and ``raw`` -- the eight summary words of lt_score_curve (include/linkteller_hip.h)."""

    def __init__(self, thresholds, tps, fps, raw, n_items):
        self.thresholds, self.tps, self.fps, self.raw, self.n_items = thresholds, tps, fps, raw, n_items
        self._host = None

    def _words(self):
        if self._host is None:
            self._host = [int(v) for v in self.raw.cpu().tolist()]      # ONE copy of 8 words, one wait
        return self._host

    def summary(self) -> dict:
        """``{"n_thresholds", "n_pos", "n_neg", "auc", "ap"}`` after one copy of 8 words and one wait (cached).  ``auc`` is
        ``auc2 / (2 P N)``, a true division of Python ints -- NaN when one class is missing (the counts are still right; sklearn's
        ``roc_auc_score`` raises there); ``ap`` is 0.0 without positives.  Raises ``IndexError`` when an index lay outside the
        scores, ``ValueError`` when a listed score was NaN / Inf (as sklearn does) or a label was neither 0 nor 1."""
        import struct
        w = self._words()
        if w[6]:
            raise IndexError(f"score_curve: {w[6]} of {self.n_items} indices outside the scores")
        if w[5]:
            raise ValueError(f"score_curve: {w[5]} of {self.n_items} scores are NaN or infinite")
        if w[7]:
            raise ValueError(f"score_curve: {w[7]} of {self.n_items} labels are neither 0 nor 1")
        d, p, n, auc2 = w[0], w[1], w[2], w[3]
        return {"n_thresholds": d, "n_pos": p, "n_neg": n, "auc": auc2 / (2 * p * n) if p and n else float("nan"),
                "ap": struct.unpack("<d", struct.pack("<q", w[4]))[0]}

    def counts(self):
        """``(thresholds, tps, fps)`` as numpy arrays of the D written entries (one more copy of each array's head)."""
        d = self.summary()["n_thresholds"]
        return self.thresholds[:d].cpu().numpy(), self.tps[:d].cpu().numpy(), self.fps[:d].cpu().numpy()


def score_curve(scores: torch.Tensor, labels: torch.Tensor, index: torch.Tensor = None) -> ScoreCurve:
    """The counts table behind the attack's ROC / PR curves, AUC and AP on the device (lt_score_curve; the reference's three
    sklearn calls of attacker.py:378-389).  Item k has label ``labels[k]`` (uint8, 0 / 1) and score ``scores.view(-1)[k]`` -- or,
    with ``index`` (int64), the STORAGE element ``index[k]`` of ``scores``, counted from its first element: a strided matrix
    is addressed as ``i * scores.stride(0) + j``, elements may repeat, what is not listed is not read.  ``scores``: float32 CUDA
    tensor with last-dimension stride 1 (without an index: contiguous).  Nothing is brought to the host here; the returned
    ``ScoreCurve`` does that on request.  Enqueues on the current stream and does not synchronise."""
    for t, name in ((scores, "scores"), (labels, "labels")) + (((index, "index"),) if index is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise _lib.LinkTellerHipError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
    if scores.dtype != torch.float32 or scores.dim() < 1:
        raise TypeError(f"scores must be a float32 tensor of at least one dimension, got {scores.dtype} {tuple(scores.shape)}")
    if labels.dtype != torch.uint8 or labels.dim() != 1 or not labels.is_contiguous():
        raise TypeError(f"labels must be a contiguous 1-d uint8 tensor, got {labels.dtype} {tuple(labels.shape)}")
    if scores.numel() and scores.stride(-1) != 1 and scores.shape[-1] > 1:
        raise ValueError("scores must have last-dimension stride 1 (rows may be strided)")
    n_items = int(labels.numel())
    if n_items < 1:
        raise ValueError("score_curve: no items")
    dev = scores.device
    if labels.device != dev or (index is not None and index.device != dev):
        raise ValueError("scores, labels and index must live on one device")
    if index is not None:
        if index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous() or index.numel() != n_items:
            raise TypeError(f"index must be a contiguous int64 tensor of {n_items} entries, got {index.dtype} {tuple(index.shape)}")
        # the extent of the view in storage elements, from its first element
        n_scores = 1 + sum((s - 1) * st for s, st in zip(scores.shape, scores.stride())) if scores.numel() else 0
    else:
        if not scores.is_contiguous():
            raise ValueError("scores must be contiguous when no index is given")
        n_scores = int(scores.numel())
        if n_scores < n_items:
            raise ValueError(f"{n_scores} scores for {n_items} labels")
    if n_scores < 1:
        raise ValueError("score_curve: scores holds no element")
    thresholds = torch.empty(n_items, dtype=torch.float32, device=dev)
    tps = torch.empty(n_items, dtype=torch.int64, device=dev)
    fps = torch.empty(n_items, dtype=torch.int64, device=dev)
    raw = torch.empty(8, dtype=torch.int64, device=dev)
    need = _lib.lib().lt_score_curve_workspace_bytes(n_items)
    key = (dev, need)
    ws = _curve_ws.get(key)
    if ws is None:
        ws = _workspace(need, dev)
        _curve_ws.clear()
        _curve_ws[key] = ws
    _lib.check(_lib.lib().lt_score_curve(scores.data_ptr(), n_scores, index.data_ptr() if index is not None else None,
                                         labels.data_ptr(), n_items, thresholds.data_ptr(), tps.data_ptr(), fps.data_ptr(),
                                         raw.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "lt_score_curve")
    return ScoreCurve(thresholds, tps, fps, raw, n_items)


_corr_ws = {}        # corr_square / corr_pairs' workspace: one per device, the largest size asked for so far


class CorrInfo:
    """The four info words of lt_corr_square / lt_corr_pairs, still on the device (``raw``, int64 [4]: [0] zero-norm rows / pairs,
    [1] node ids outside [0, n)).  ``check()`` brings them over -- one copy of four words, the caller's wait -- and raises."""

    def __init__(self, raw, what, n):
        self.raw, self.what, self.n = raw, what, n
        self._host = None

    def check(self, nan_ok: bool = True) -> dict:
        """``{"zero_norm", "bad_ids"}``.  ``IndexError`` when a node id lay outside [0, n) (its cells are NaN); ``ValueError`` when
        ``nan_ok`` is false and a zero-norm row made cells NaN (with ``nan_ok`` the NaNs stand, as in the reference's 0 / 0)."""
        if self._host is None:
            self._host = [int(v) for v in self.raw.cpu().tolist()]
        zero, bad = self._host[0], self._host[1]
        if bad:
            raise IndexError(f"{self.what}: {bad} node ids outside [0, {self.n})")
        if zero and not nan_ok:
            raise ValueError(f"{self.what}: {zero} zero-norm rows / pairs (a centred vector is zero): their scores are NaN")
        return {"zero_norm": zero, "bad_ids": bad}


def _corr_operands(vectors, lists, what):
    if not isinstance(vectors, torch.Tensor):
        raise TypeError("vectors must be a torch.Tensor")
    if not vectors.is_cuda:
        raise _lib.LinkTellerHipError(f"vectors must live on the GPU (got {vectors.device}); there is no CPU path")
    if vectors.dtype != torch.float32 or vectors.dim() != 2:
        raise TypeError(f"vectors must be a 2-d float32 tensor, got {vectors.dtype} {tuple(vectors.shape)}")
    n, d = int(vectors.shape[0]), int(vectors.shape[1])
    if n < 1 or d < 1:
        raise ValueError(f"{what}: vectors of shape {tuple(vectors.shape)} hold no element")
    if d > 1 and vectors.stride(1) != 1:
        raise ValueError("vectors must have last-dimension stride 1 (rows may be strided)")
    ldv = int(vectors.stride(0)) if n > 1 else d
    if ldv < d:
        raise ValueError(f"row stride {ldv} smaller than the {d} columns")
    out = []
    for name, t in lists:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise _lib.LinkTellerHipError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
        if t.dtype != torch.int32 or t.dim() != 1:
            raise TypeError(f"{name} must be a 1-d int32 tensor, got {t.dtype} {tuple(t.shape)}")
        if t.device != vectors.device:
            raise ValueError(f"vectors and {name} must live on one device")
        out.append(t.contiguous())
    return n, d, ldv, out


def _corr_workspace(n, d, k, m, dev):
    need = _lib.lib().lt_corr_workspace_bytes(n, d, k, m)
    if need == 0:
        raise ValueError(f"corr: n={n}, D={d}, k={k}, pairs={m} are outside what the library serves")
    ws = _corr_ws.get(dev)
    if ws is None or ws.numel() < need:      # (one per device, grown to the largest need: alternating calls and sizes reallocate nothing)
        ws = _corr_ws[dev] = _workspace(need, dev)
    return ws


def corr_square(vectors: torch.Tensor, nodes: torch.Tensor):
    """The baseline attacks' correlation square on the device (lt_corr_square; the reference's ``d @ d.T / nrm / nrm``,
    attacker.py:305-313) -> ``(out, info)``: ``out`` fp32 [k, k], ``out[i, j]`` the correlation of rows ``nodes[i]`` and ``nodes[j]``
    of ``vectors`` ([n, D] float32 CUDA, rows may be strided) centred by the column mean over the k listed rows; symmetric bit for
    bit; fp64 arithmetic, one rounding.  ``nodes``: int32 CUDA.  Nothing is brought to the host here: ``info.check()`` (a
    ``CorrInfo``) does that after the caller's wait and raises ``IndexError`` for ids outside [0, n)."""
    n, d, ldv, (nodes,) = _corr_operands(vectors, (("nodes", nodes),), "corr_square")
    k, dev = int(nodes.numel()), vectors.device
    out = torch.empty((k, k), dtype=torch.float32, device=dev)
    raw = torch.zeros(4, dtype=torch.int64, device=dev)
    if k:
        ws = _corr_workspace(n, d, k, 0, dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().lt_corr_square(vectors.data_ptr(), ldv, n, d, nodes.data_ptr(), k, out.data_ptr(), k, raw.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _stream()), "lt_corr_square")
    return out, CorrInfo(raw, "corr_square", n)


def corr_pairs(vectors: torch.Tensor, u: torch.Tensor, v: torch.Tensor):
    """The baseline attacks' correlation of listed pairs on the device (lt_corr_pairs; attacker.py:337-375) -> ``(out, info)``:
    ``out`` fp32 [m], ``out[p]`` the correlation of rows ``u[p]`` and ``v[p]`` of ``vectors`` centred by the column mean over ALL
    n rows (``u[p] == v[p]`` is allowed).  Otherwise as ``corr_square``."""
    n, d, ldv, (u, v) = _corr_operands(vectors, (("u", u), ("v", v)), "corr_pairs")
    if u.shape != v.shape:
        raise ValueError(f"u and v differ in length: {u.numel()} / {v.numel()}")
    m, dev = int(u.numel()), vectors.device
    out = torch.empty(m, dtype=torch.float32, device=dev)
    raw = torch.zeros(4, dtype=torch.int64, device=dev)
    if m:
        ws = _corr_workspace(n, d, 0, m, dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().lt_corr_pairs(vectors.data_ptr(), ldv, n, d, u.data_ptr(), v.data_ptr(), m, out.data_ptr(),
                                                raw.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "lt_corr_pairs")
    return out, CorrInfo(raw, "corr_pairs", n)


class CorrRows:
    """``corr_square``'s square a band of rows at a time (lt_corr_rows_prepare / lt_corr_rows): the k x k matrix is never formed.
    The constructor enqueues the mean and the norms of the k listed rows into a workspace of its own and leaves ``info`` (a
    ``CorrInfo``): ``info.check(nan_ok=False)`` -- one copy of four words -- tells about NaN rows before any row is formed.
    ``rows(row_begin, n_rows, n_cols=None)`` returns fp32 [n_rows, k] on the device whose columns [0, n_cols) (default: all k) hold
    ``corr_square``'s cells bit for bit, whatever the cut into bands; columns at or right of ``n_cols`` hold whatever an earlier
    call left.  The buffer is REUSED by the next call.  ``vectors`` / ``nodes`` as for ``corr_square``; both are kept alive and
    must not be written while the handle is in use.  At most ``max_rows`` rows a call (``.max_rows``: clipped to k and to the 4 194 240 rows one
    library call takes).  ``device_bytes``: workspace plus buffer."""

    def __init__(self, vectors: torch.Tensor, nodes: torch.Tensor, max_rows: int):
        n, d, ldv, (nodes,) = _corr_operands(vectors, (("nodes", nodes),), "CorrRows")
        max_rows = int(max_rows)
        if max_rows < 1:
            raise ValueError(f"max_rows={max_rows} < 1")
        k, dev = int(nodes.numel()), vectors.device
        if k < 1:
            raise ValueError("CorrRows: no node listed")
        self.n, self.d, self.ldv, self.k, self.device = n, d, ldv, k, dev
        self.max_rows = min(max_rows, k, 65535 * 64)      # (one launch's grid: 65 535 row blocks of 64)
        self._vectors, self._nodes = vectors, nodes
        need = _lib.lib().lt_corr_rows_workspace_bytes(n, d, k, self.max_rows)
        if need == 0:
            raise ValueError(f"CorrRows: n={n}, D={d}, k={k}, max_rows={self.max_rows} are outside what the library serves")
        self._ws = _workspace(need, dev)
        self._out = torch.empty((self.max_rows, k), dtype=torch.float32, device=dev)
        self.device_bytes = int(self._ws.numel()) * self._ws.element_size() + int(self._out.numel()) * 4
        raw = torch.zeros(4, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().lt_corr_rows_prepare(vectors.data_ptr(), ldv, n, d, nodes.data_ptr(), k, raw.data_ptr(),
                                                       self._ws.data_ptr(), self._ws.numel(), _stream()), "lt_corr_rows_prepare")
        self.info = CorrInfo(raw, "CorrRows", n)

    def rows(self, row_begin: int, n_rows: int, n_cols: int = None) -> torch.Tensor:
        row_begin, n_rows = int(row_begin), int(n_rows)
        n_cols = self.k if n_cols is None else int(n_cols)
        if row_begin < 0 or n_rows < 0 or row_begin + n_rows > self.k:
            raise ValueError(f"rows [{row_begin}, {row_begin + n_rows}) outside the {self.k} listed")
        if n_rows > self.max_rows:
            raise ValueError(f"{n_rows} rows a call, the handle was made for {self.max_rows}")
        if not 0 <= n_cols <= self.k:
            raise ValueError(f"n_cols={n_cols} outside [0, {self.k}]")
        out = self._out[:n_rows, :self.k]
        if n_rows == 0 or n_cols == 0:
            return out
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().lt_corr_rows(self._vectors.data_ptr(), self.ldv, self.n, self.d, self._nodes.data_ptr(), self.k,
                                               row_begin, n_rows, n_cols, out.data_ptr(), int(self._out.stride(0)),
                                               self._ws.data_ptr(), self._ws.numel(), _stream()), "lt_corr_rows")
        return out


def export_rows_f64(rows: torch.Tensor):
    """The finished rows as a float64 numpy array on the host (the reference's ``influence_val = np.zeros(...)`` filled by
    n_test**2 ``.item()`` round trips, attacker.py:216-229) -- ONE launch that widens on the device and writes straight into
    pinned host memory over PCIe (lt_export_rows_f64), one wait.  The array owns a block of torch's pinned-memory cache
    (recycled when the array is released: a fresh result per call costs no allocation).  Ends with the device-side node-id
    check of everything the stream has run (IndexError, as the reference raises)."""
    if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_cuda:
        raise TypeError("rows must be a 2-d float32 CUDA tensor")
    r, c = rows.shape
    host = torch.empty((r, c), dtype=torch.float64, pin_memory=True)
    if rows.stride(1) != 1:
        rows = rows.contiguous()
    stream = torch.cuda.current_stream(rows.device)
    _lib.check(_lib.lib().lt_export_rows_f64(rows.data_ptr(), rows.stride(0) if r > 1 else max(c, 1), r, c, host.data_ptr(), max(c, 1),
                                             C.c_void_p(stream.cuda_stream)), "lt_export_rows_f64")
    stream.synchronize()
    node_check()
    return host.numpy()


def node_check():
    """Raise IndexError when a probe / observed list of a COMPLETED call held a node id outside [0, n) (lt_node_check: the
    lists are device memory, so the kernels check them; call after synchronising)."""
    _lib.check(_lib.lib().lt_node_check(None, None), "lt_node_check")


def _as_rows(rows, n, device, name) -> torch.Tensor:
    """Row list (tensor or array, any integer dtype) -> contiguous int32 tensor on ``device``; every id is checked here, an id
    outside [0, n) raises ``IndexError`` as indexing does in the reference."""
    t = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(rows)
    if t.dtype.is_floating_point or t.dtype == torch.bool or t.is_complex():
        raise TypeError(f"{name} must hold integer ids, got {t.dtype}")
    t = t.reshape(-1)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
        raise IndexError(f"{name} out of range [0, {n})")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _as_nodes(nodes, n, device, name) -> torch.Tensor:
    """Node list -> int32 device tensor.  Host lists are range-checked here (IndexError, as the reference's indexing raises).  An
    int32 CUDA tensor is taken as it is -- no copy, no host round trip -- and its ids are checked by the KERNELS of the call that
    reads it: an id outside [0, n) is replaced by node 0 there and raises a flag the caller collects with ``engine.node_check()``
    AFTER synchronising (``influence_matrix_host`` / ``export_rows_f64`` do).  The flag is one per process (two words of mapped host
    memory): a caller that never collects it gets LT_ERR_INDEX from the NEXT probe call of any baseline instead."""
    if isinstance(nodes, torch.Tensor) and nodes.is_cuda and nodes.dtype == torch.int32:
        return nodes.contiguous()          # fast path: the ids are checked on the device (lt_node_check / LT_ERR_INDEX)
    t = torch.as_tensor(nodes).to(torch.int64).reshape(-1).cpu()
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
        raise IndexError(f"{name} out of range [0, {n})")
    return t.to(torch.int32).to(device)


def torch_epoch_orders(n: int, n_epochs: int) -> torch.Tensor:
    """int64 [n_epochs, n]: the row orders ``DataLoader(dataset of n rows, shuffle=True)`` walks in its next ``n_epochs``
    epochs under torch's global CPU generator, which it advances exactly as those epochs would: per epoch the loader's
    iterator first draws its base seed, then its ``RandomSampler`` draws the seed of the epoch's permutation."""
    from torch.utils.data import RandomSampler
    sampler = RandomSampler(range(int(n)))
    out = torch.empty((max(int(n_epochs), 0), int(n)), dtype=torch.int64)
    for e in range(out.shape[0]):
        torch.empty((), dtype=torch.int64).random_()      # _BaseDataLoaderIter's base seed
        out[e] = torch.tensor(list(sampler), dtype=torch.int64)
    return out


def _mlp_params(params, depth, f):
    """The parameter tensors of an MLP baseline, checked: (W1 [F, H], b1 [H], W2 [H, C], b2 [C]) or (W [F, C], b [C])."""
    if depth not in (1, 2):
        raise ValueError(f"depth must be 1 or 2, got {depth!r}")
    names = ("W1", "b1", "W2", "b2") if depth == 2 else ("W", "b")
    if len(params) != len(names):
        raise ValueError(f"depth {depth} takes the parameters {names}, got {len(params)} tensors")
    ps = [_f32(t, n) for t, n in zip(params, names)]
    dims = [f] + [w.shape[1] if w.dim() == 2 else -1 for w in ps[0::2]]
    if any(w.dim() != 2 or tuple(w.shape) != (dims[l], dims[l + 1]) or tuple(b.shape) != (dims[l + 1],)
           for l, (w, b) in enumerate(zip(ps[0::2], ps[1::2]))):
        raise ValueError("inconsistent MLP shapes")
    return ps, names, dims


class MLPTrainer:
    """Minibatch training of the feature-only baselines on the GPU (lt_mlp_trainer_*): the reference's ``MLPTrainer`` loop
    (mlp_trainer.py) over ``SingleHiddenLayerMLP`` (``depth=2``: parameters w1, b1, w2, b2) or ``OneLayerMLP`` (``depth=1``:
    w, b), in the project's [in, out] layout.  One epoch is ``ceil(n / batch_size)`` Adam steps over the epoch's row order; a
    whole ``run`` is enqueued by one library call.  The parameters are updated IN PLACE; the trainer owns the Adam moments.
    Dropout and the default shuffle are Philox4x32-10 streams keyed by ``seed`` (include/linkteller_hip.h), not torch's
    generator.  Limits: hidden width <= 256, classes <= 256."""

    _LOSSES = {"ce": 0, "bce": 1}

    def __init__(self, x, labels, *params, depth, batch_size, lr, weight_decay, dropout=0.0, seed=0, loss="ce"):
        if loss not in self._LOSSES:
            raise ValueError(f"loss must be 'ce' or 'bce', got {loss!r}")
        if not 0.0 <= float(dropout) <= 1.0:
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout}")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be at least 1, got {batch_size}")
        self.x = _f32(x, "x")
        n, f = self.x.shape
        self.params, self._names, dims = _mlp_params(params, depth, f)
        for t, src in zip(self.params, params):
            if t.data_ptr() != src.data_ptr():
                raise ValueError("the parameters are updated in place: pass contiguous float32 device tensors")
        self.n, self.f, self.c, self.depth, self.loss = n, f, dims[-1], int(depth), loss
        self.h = dims[1] if depth == 2 else 0
        self.batch_size = int(batch_size)
        self.steps_per_epoch = -(-n // self.batch_size)
        _require_finite(features=self.x, **dict(zip(self._names, self.params)))
        if not isinstance(labels, torch.Tensor):
            labels = torch.as_tensor(labels)
        if loss == "bce":
            if tuple(labels.shape) != (n, self.c):
                raise ValueError(f"labels must be [{n}, {self.c}] for loss='bce', got {tuple(labels.shape)}")
            if labels.is_floating_point() or labels.is_complex():
                raise ValueError(f"labels must have an integer or bool dtype, got {labels.dtype}")
            if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) > 1):
                raise ValueError("labels must hold 0 / 1")
            self.labels = labels.to(device=self.x.device, dtype=torch.uint8).contiguous()
        else:
            labels = labels.reshape(-1)
            if labels.numel() != n:
                raise ValueError(f"labels: {labels.numel()} entries for {n} rows")
            if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= self.c):
                raise ValueError(f"labels outside [0, {self.c})")
            self.labels = labels.to(device=self.x.device, dtype=torch.int32).contiguous()
        ptrs = [t.data_ptr() for t in self.params] + [None] * (4 - len(self.params))
        h = C.c_void_p()
        _lib.check(_lib.lib().lt_mlp_trainer_create(self.x.data_ptr(), f, n, f, self.labels.data_ptr(), self.c,
                                                    self._LOSSES[loss], self.depth, self.h, self.c, *ptrs, self.batch_size,
                                                    float(lr), float(weight_decay), float(dropout), int(seed) & (2**64 - 1),
                                                    _stream(), C.byref(h)), "lt_mlp_trainer_create")
        self._h = h
        self._finalizer = weakref.finalize(self, _lib.lib().lt_mlp_trainer_destroy, h)

    def _order(self, epochs, order):
        """``order`` of ``run`` as the int32 device tensor [epochs, n] the library reads (None: the Philox shuffle)."""
        if order is None:
            return None
        if isinstance(order, str):
            if order != "torch":
                raise ValueError(f"order must be None, a tensor or 'torch', got {order!r}")
            order = torch_epoch_orders(self.n, epochs)
        t = order if isinstance(order, torch.Tensor) else torch.as_tensor(order)
        if t.dtype.is_floating_point or t.dtype == torch.bool or t.is_complex():
            raise TypeError(f"order must hold integer row ids, got {t.dtype}")
        if tuple(t.shape) != (epochs, self.n):
            raise ValueError(f"order must be [{epochs}, {self.n}], got {tuple(t.shape)}")
        if t.is_cuda and t.dtype == torch.int32:
            return t.contiguous()      # ids checked on the device (engine.node_check)
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= self.n):
            raise IndexError(f"order out of range [0, {self.n})")
        return t.to(device=self.x.device, dtype=torch.int32).contiguous()

    def run_async(self, epochs: int, order=None) -> torch.Tensor:
        """Enqueue ``epochs`` epochs; returns the device record [epochs * steps_per_epoch, 2] (loss, tp count) without syncing."""
        epochs = max(int(epochs), 0)
        dev_order = self._order(epochs, order)
        record = torch.empty((epochs * self.steps_per_epoch, 2), dtype=torch.float32, device=self.x.device)
        _lib.check(_lib.lib().lt_mlp_trainer_run(self._h, epochs, None if dev_order is None else dev_order.data_ptr(),
                                                 record.data_ptr(), _stream()), "lt_mlp_trainer_run")
        if dev_order is not None:
            dev_order.record_stream(torch.cuda.current_stream())
        for p in self.params:
            torch.autograd.graph.increment_version(p)
        return record

    def run(self, epochs: int, order=None):
        """Run ``epochs`` epochs; returns (loss [steps] float32, count [steps] int64) per optimiser step as CPU arrays (one
        read at the end).  ``order``: None -- the documented Philox shuffle; an integer tensor [epochs, n] of row ids, one
        permutation per epoch; ``"torch"`` -- each epoch's permutation drawn on the host as ``DataLoader(shuffle=True)`` draws
        it under torch's global seed (``torch_epoch_orders``) and uploaded before the run: the reference's batch composition."""
        rec = self.run_async(epochs, order).cpu().numpy()
        return rec[:, 0].copy(), rec[:, 1].astype("int64")

    def step_async(self, rows) -> torch.Tensor:
        """Enqueue ONE optimiser step over the batch ``rows`` (at most ``min(batch_size, n)`` row ids): the step ``run`` takes
        for that batch, bit for bit.  Returns the device record [2] (loss, tp count) without syncing."""
        r = _as_nodes(rows, self.n, self.x.device, "rows")
        record = torch.empty((2,), dtype=torch.float32, device=self.x.device)
        _lib.check(_lib.lib().lt_mlp_trainer_step(self._h, r.data_ptr(), int(r.numel()), record.data_ptr(), _stream()),
                   "lt_mlp_trainer_step")
        r.record_stream(torch.cuda.current_stream())
        for p in self.params:
            torch.autograd.graph.increment_version(p)
        return record

    def _counts(self):
        s, e, b = C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(_lib.lib().lt_mlp_trainer_counts(self._h, C.byref(s), C.byref(e), C.byref(b)), "lt_mlp_trainer_counts")
        return s.value, e.value, b.value

    @property
    def step(self) -> int:
        return self._counts()[0]

    @property
    def epoch(self) -> int:
        return self._counts()[1]

    def grads(self):
        """The last step's gradients (before weight decay), one per parameter in the constructor's order."""
        out = [torch.empty_like(p) for p in self.params]
        ptrs = [t.data_ptr() for t in out] + [None] * (4 - len(out))
        _lib.check(_lib.lib().lt_mlp_trainer_grads(self._h, *ptrs, _stream()), "lt_mlp_trainer_grads")
        return tuple(out)

    def logits(self) -> torch.Tensor:
        """The last step's train-mode logits [rows of that batch, C], rows in batch order (before that step's update)."""
        out = torch.empty((self._counts()[2], self.c), dtype=torch.float32, device=self.x.device)
        _lib.check(_lib.lib().lt_mlp_trainer_logits(self._h, out.data_ptr(), self.c, _stream()), "lt_mlp_trainer_logits")
        return out

    def last_order(self) -> torch.Tensor:
        """The row order of the last epoch run under the Philox shuffle, int32 [n]."""
        out = torch.empty((self.n,), dtype=torch.int32, device=self.x.device)
        _lib.check(_lib.lib().lt_mlp_trainer_order(self._h, out.data_ptr(), _stream()), "lt_mlp_trainer_order")
        return out


def mlp_forward(x, *params, depth, rows=None) -> torch.Tensor:
    """Eval-mode logits of an MLP baseline (lt_mlp_forward) for all rows of ``x`` or the listed ones: [rows, C] float32."""
    x = _f32(x, "x")
    n, f = x.shape
    ps, _, dims = _mlp_params(params, depth, f)
    r = None if rows is None else _as_nodes(rows, n, x.device, "rows")
    m = n if r is None else int(r.numel())
    c, h = dims[-1], dims[1] if depth == 2 else 0
    out = torch.empty((m, c), dtype=torch.float32, device=x.device)
    if m == 0:
        return out
    lib = _lib.lib()
    ws = _workspace(lib.lt_mlp_forward_workspace_bytes(m, f, depth, h, c), x.device)
    ptrs = [t.data_ptr() for t in ps] + [None] * (4 - len(ps))
    _lib.check(lib.lt_mlp_forward(x.data_ptr(), f, n, f, depth, h, c, *ptrs, None if r is None else r.data_ptr(), m,
                                  out.data_ptr(), c, ws.data_ptr(), ws.numel(), _stream()), "lt_mlp_forward")
    return out

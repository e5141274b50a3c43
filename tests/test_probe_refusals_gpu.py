"""The three pair-list entry points (lt_influence_pairs, lt_influence3_pairs, lt_influence2w_pairs) refuse a bad offset list the same
way -- one host check serves them (lt_pairs_check, lt_internal.h): LT_ERR_INVALID, "pair_ptr" in lt_last_error(), nothing launched,
so a NaN-filled ``out`` stays as it was.  One tiny graph (`loops` of wide2_shape_cases / gcn3_shape_cases), mode `delta`."""
import numpy as np
import pytest
import torch

import test_probe_bits_gpu as P
from linkteller_amd import _lib, engine, graph

pytestmark = pytest.mark.gpu

LT_ERR_INVALID = -1
ENTRY = {"b2": ("lt_influence_pairs", "lt_influence_pairs_workspace_bytes"),
         "b3": ("lt_influence3_pairs", "lt_influence3_pairs_workspace_bytes"),
         "b2w33": ("lt_influence2w_pairs", "lt_influence2w_pairs_workspace_bytes")}


def _bad_lists(ptr):
    first, down, last = ptr.copy(), ptr.copy(), ptr.copy()
    first[0] = 1
    down[4] = down[3] - 1
    last[-1] += 1
    return {"first offset not 0": first, "a decrease": down, "last offset != n_pairs": last, "NULL with n_pairs > 0": None}


@pytest.mark.parametrize("handle", list(ENTRY))
def test_a_bad_offset_list_is_refused_before_anything_runs(gpu, handle):
    cls, _, _ = P.HANDLES[handle]
    a_hat, x, params, probes, _, (ptr, pobs) = P._inputs(handle, "loops")
    dev = [torch.from_numpy(np.ascontiguousarray(p)).to(gpu) for p in params]
    base = getattr(engine, cls)(graph.HipGraph(a_hat), torch.from_numpy(x).to(gpu), *dev)
    base.enable_fp64()
    lib, (call, query) = _lib.lib(), ENTRY[handle]
    pt, ot = torch.from_numpy(probes).to(gpu), torch.from_numpy(pobs).to(gpu)
    n_p, n_m = len(probes), len(pobs)
    extra = (_lib.MODE_DELTA,) if handle == "b2" else ()
    ws = engine._workspace(getattr(lib, query)(base._h, n_p, n_m, *extra), gpu)
    out = torch.full((n_m,), float("nan"), dtype=torch.float32, device=gpu)

    def raw(p):
        host = None if p is None else np.ascontiguousarray(p, dtype=np.int64)
        rc = getattr(lib, call)(base._h, pt.data_ptr(), n_p, None if host is None else host.ctypes.data, ot.data_ptr(), n_m, 1e-4,
                                _lib.MODE_DELTA, out.data_ptr(), ws.data_ptr(), ws.numel(), engine._stream())
        return rc, lib.lt_last_error().decode()
    for what, bad in _bad_lists(ptr).items():
        rc, msg = raw(bad)
        assert rc == LT_ERR_INVALID and "pair_ptr" in msg and msg.startswith(call), (what, rc, msg)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), what
    rc, msg = raw(ptr)                      # the good list, through the same closure
    assert rc == 0, msg
    torch.cuda.synchronize()
    engine.node_check()
    assert bool(torch.isfinite(out).all())

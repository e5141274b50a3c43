"""lt_graph_create_device / lt_graph_table without a GPU: the symbols are bound, arguments are checked before any device call,
and there is no fallback: without a device the Python route fails loudly."""
import ctypes as C
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lt():
    from linkteller_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_symbols_are_bound(lt):
    h = lt.lib()
    for name in ("lt_graph_create_device", "lt_graph_table"):
        assert name in lt.SIGNATURES and getattr(h, name).argtypes == lt.SIGNATURES[name][1]
    assert h.lt_abi_version() == 5
    ids = sorted(v[0] for v in lt.GRAPH_TABLES.values())
    assert ids == list(range(len(ids))) and lt.GRAPH_TABLES["scalars"][0] == len(ids) - 1
    src = open(os.path.join(os.path.dirname(os.path.dirname(lt.LIB_PATH)), "include", "linkteller_hip.h")).read()
    for name, (which, _) in lt.GRAPH_TABLES.items():
        assert f"LT_TABLE_{name.upper()} = {which}," in src
    assert f"LT_TABLE_COUNT = {len(ids)}" in src and f"#define LT_TABLE_SCALAR_COUNT {len(lt.GRAPH_SCALARS)}" in src


def test_arguments_are_checked_before_any_device_call(lt):
    h = lt.lib()
    out = C.c_void_p(1)
    rp = np.zeros(3, dtype=np.int32)
    assert h.lt_graph_create_device(2, 0, rp.ctypes.data, None, None, None, None) == -1 and b"out is NULL" in h.lt_last_error()
    assert h.lt_graph_create_device(-1, 0, rp.ctypes.data, None, None, None, C.byref(out)) == -1 and b"negative" in h.lt_last_error()
    assert out.value is None
    assert h.lt_graph_create_device(2, -3, rp.ctypes.data, None, None, None, C.byref(out)) == -1 and b"negative" in h.lt_last_error()
    assert h.lt_graph_create_device(2, 2 ** 31 - 1, rp.ctypes.data, rp.ctypes.data, rp.ctypes.data, None, C.byref(out)) == -1
    assert b"int32" in h.lt_last_error()
    assert h.lt_graph_create_device(2, 0, None, None, None, None, C.byref(out)) == -1 and b"rowptr is NULL" in h.lt_last_error()
    assert h.lt_graph_create_device(2, 2, rp.ctypes.data, None, rp.ctypes.data, None, C.byref(out)) == -1 and b"col/val" in h.lt_last_error()
    assert h.lt_graph_create_device(2, 2, rp.ctypes.data, rp.ctypes.data, None, None, C.byref(out)) == -1 and b"col/val" in h.lt_last_error()
    size = C.c_int64(-1)
    assert h.lt_graph_table(None, 0, None, 0, C.byref(size)) == -1 and b"graph is NULL" in h.lt_last_error()
    assert h.lt_graph_table(None, 99, None, 0, None) == -1


def test_no_device_means_loud_failure(lt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from linkteller_amd import graph
    rowptr = torch.zeros(3, dtype=torch.int32)
    empty_i, empty_f = torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float32)
    with pytest.raises(lt.LinkTellerHipError):
        graph.HipGraph.from_device_csr(rowptr, empty_i, empty_f)
    import scipy.sparse as sp
    os.environ["LT_GRAPH_BUILD"] = "device"
    try:
        with pytest.raises(lt.LinkTellerHipError):
            graph.HipGraph(sp.identity(4, format="csr"))
    finally:
        del os.environ["LT_GRAPH_BUILD"]

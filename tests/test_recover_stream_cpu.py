"""The streaming edge recovery without a GPU: the command line's --recover-chunk / --recover-nodes, the argument checks of
engine.TopPairsStream / engine.pairs_present and of lt_top_stream_create that come before any device call, and the header /
binding of every new entry point."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

NEW_SYMBOLS = ["lt_top_stream_create", "lt_top_stream_bytes", "lt_top_stream_push", "lt_top_stream_finish", "lt_top_stream_reset",
               "lt_top_stream_stats", "lt_top_stream_destroy", "lt_pairs_present"]


@pytest.fixture(scope="module")
def lt():
    from linkteller_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_new_symbols_declared_bound_and_exported(lt):
    from conftest import REPO
    header = open(os.path.join(REPO, "include", "linkteller_hip.h")).read()
    h = lt.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in lt.SIGNATURES, name
        assert getattr(h, name).argtypes == lt.SIGNATURES[name][1]
    assert "typedef struct lt_top_stream lt_top_stream;" in header
    assert lt.ABI_VERSION == 5 and "#define LT_ABI_VERSION 5" in header


def test_create_refusals_before_any_allocation(lt):
    h = lt.lib()
    out = C.c_void_p()
    call = lambda n, m, rows, slack: h.lt_top_stream_create(n, m, rows, slack, C.byref(out))
    assert call(1, 1, 4, 0) == -1 and b"n >= 2" in h.lt_last_error()
    assert call(65, 0, 4, 0) == -1 and b"outside" in h.lt_last_error()
    assert call(65, 2081, 4, 0) == -1 and b"[1, 2080]" in h.lt_last_error()
    assert call(65, 10, 0, 0) == -1 and b"max_push_rows" in h.lt_last_error()
    assert call(65, 10, 4, 127) == -1 and b"slack_cells" in h.lt_last_error()
    assert call(65, 10, 4, -5) == -1 and b"slack_cells" in h.lt_last_error()
    assert call(200000, (1 << 30) + 1, 4, 0) == -1 and b"beyond" in h.lt_last_error()
    assert h.lt_top_stream_create(65, 10, 4, 0, None) == -1 and b"NULL" in h.lt_last_error()
    assert out.value is None
    # a NULL handle is refused everywhere, destroy takes it
    nbytes = C.c_size_t()
    assert h.lt_top_stream_bytes(None, C.byref(nbytes)) == -1
    assert h.lt_top_stream_push(None, None, 8, 0, 1, None) == -1 and b"NULL" in h.lt_last_error()
    assert h.lt_top_stream_finish(None, None, None, None, None) == -1
    assert h.lt_top_stream_reset(None, None) == -1 and h.lt_top_stream_stats(None, None, None) == -1
    assert h.lt_top_stream_destroy(None) == 0
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    assert h.lt_pairs_present(0, p, p, p, p, 4, p, p, None) == -1
    assert h.lt_pairs_present(8, None, p, p, p, 4, p, p, None) == -1 and b"NULL" in h.lt_last_error()
    assert h.lt_pairs_present(8, p, p, p, p, -1, p, p, None) == -1 and b"m=" in h.lt_last_error()


def test_engine_checks_come_before_the_library(monkeypatch):
    from linkteller_amd import _lib, engine

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "require_gpu", boom)
    for n, m, rows, slack in ((1, 1, 4, 0), (65, 0, 4, 0), (65, 2081, 4, 0), (65, 10, 4, 127)):
        with pytest.raises(ValueError):
            engine.TopPairsStream(n, m, rows, slack_cells=slack)
    with pytest.raises(ValueError, match="max_rows"):
        engine.TopPairsStream(65, 10, 0)
    sel = engine.TopPairsStream.__new__(engine.TopPairsStream)       # push looks at its argument before its handle
    with pytest.raises(TypeError):
        sel.push(np.zeros((4, 8), dtype=np.float32), 0)
    with pytest.raises(_lib.LinkTellerHipError, match="GPU"):
        sel.push(torch.zeros(4, 8), 0)
    csr = (torch.zeros(9, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0)
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(TypeError):
        engine.pairs_present(csr, [0, 1], ids)
    with pytest.raises(_lib.LinkTellerHipError, match="GPU"):
        engine.pairs_present(csr, ids, ids)
    sel._h = None
    sel.close()                                                       # nothing to free


def test_cli_stream_flags_defaults_and_passes():
    from linkteller_amd import main as lt_main
    a = lt_main.get_arguments([])
    assert a.recover_chunk == 0 and a.recover_nodes == "sample"
    lt_main.check_recover_stream(a)
    a = lt_main.get_arguments("--attack --attack-mode efficient --sample-type unbalanced --recover --recover-chunk 64 "
                              "--recover-nodes all".split())
    assert a.recover_chunk == 64 and a.recover_nodes == "all"
    lt_main.check_recover(a)
    lt_main.check_recover_stream(a)
    with pytest.raises(SystemExit):
        lt_main.get_arguments(["--recover-nodes", "some"])


@pytest.mark.parametrize("argv, exc", [
    ("--test --attack --attack-mode efficient --sample-type unbalanced --recover-chunk 64", NotImplementedError),
    ("--test --attack --attack-mode efficient --sample-type unbalanced --recover-nodes all", NotImplementedError),
    ("--test --attack --attack-mode efficient --sample-type unbalanced --recover --recover-chunk -3", ValueError),
    ("--test --attack --attack-mode baseline --baseline-scores device --sample-type unbalanced --recover --recover-chunk 8",
     NotImplementedError),
    ("--test --attack --attack-mode baseline --baseline-scores device --sample-type unbalanced --recover --recover-nodes all",
     NotImplementedError),
])
def test_cli_stream_flags_refused_before_a_worker_is_built(argv, exc, monkeypatch):
    from linkteller_amd import main as lt_main, worker

    def boom(*a, **k):
        raise AssertionError("a Worker was built")
    monkeypatch.setattr(worker, "Worker", boom)
    monkeypatch.setattr(lt_main, "init_distributed", boom)
    with pytest.raises(exc, match="--recover"):
        lt_main.main(argv.split())

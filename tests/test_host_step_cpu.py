"""lt_influence_step_host without a device: the header, the binding, and -- with the library call mocked -- how often
Baseline.influence_matrix_host calls it."""
import os
import re
import types

import pytest
import torch

from conftest import REPO
from linkteller_amd import _lib, engine


def _header():
    return open(os.path.join(REPO, "include", "linkteller_hip.h")).read()


def test_header_declares_the_entry_and_its_flags():
    src = _header()
    assert re.search(r"^#define LT_STEP_REFRESH 1$", src, flags=re.M)
    assert re.search(r"^#define LT_STEP_DST_PINNED 2$", src, flags=re.M)
    assert (_lib.STEP_REFRESH, _lib.STEP_DST_PINNED) == (1, 2)
    assert re.search(r"^int lt_influence_step_host\(", src, flags=re.M)
    assert re.search(r"^#define LT_ABI_VERSION 5\b", src, flags=re.M) and _lib.ABI_VERSION == 5
    assert _lib.lib().lt_abi_version() == 5
    assert int(re.search(r"LT_ERR_WORKSPACE = (-\d+)", src).group(1)) == _lib.LT_ERR_WORKSPACE


def _declared_args(name):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
    return [a.strip() for a in args.split(",")]


def test_binding_has_the_header_argument_count():
    step, host = _declared_args("lt_influence_step_host"), _declared_args("lt_influence_matrix_host")
    assert step[:len(host)] == host, "the arguments of lt_influence_matrix_host come first"
    assert [a.split()[-1].lstrip("*") for a in step[len(host):]] == ["flags", "bad_probe", "bad_observe"]
    res, args = _lib.SIGNATURES["lt_influence_step_host"]
    assert len(args) == len(step) == 17
    assert args[:14] == _lib.SIGNATURES["lt_influence_matrix_host"][1]
    assert hasattr(_lib.lib(), "lt_influence_step_host")


def test_entry_checks_its_arguments_without_a_device():
    import ctypes as C
    h = _lib.lib()
    bp, bo = C.c_int32(5), C.c_int32(5)
    assert h.lt_influence_step_host(None, None, 1, None, 1, 1e-4, 2, None, 1, None, 1, None, 0, None, 3, C.byref(bp), C.byref(bo)) == -1
    assert (bp.value, bo.value) == (0, 0)
    assert h.lt_influence_step_host(None, None, 1, None, 1, 1e-4, 2, None, 1, None, 1, None, 0, None, 8, None, None) == -1
    assert b"unknown flags" in h.lt_last_error()


class _FakeLib:
    """Stands for the loaded library: records the calls of the entries a host-landed step may use."""

    def __init__(self, step_returns):
        self.calls = []
        self._step_returns = list(step_returns)

    def lt_influence_step_host(self, *a):
        self.calls.append(("lt_influence_step_host", a))
        return self._step_returns.pop(0)

    def lt_influence_matrix_host(self, *a):
        self.calls.append(("lt_influence_matrix_host", a))
        return 0

    def lt_influence_workspace_bytes(self, *a):
        self.calls.append(("lt_influence_workspace_bytes", a))
        return 4096

    def lt_baseline_refresh(self, *a):
        self.calls.append(("lt_baseline_refresh", a))
        return 0

    def lt_baseline_refresh_rows_fp64(self, *a):
        self.calls.append(("lt_baseline_refresh_rows_fp64", a))
        return 0

    def lt_node_check(self, *a):
        self.calls.append(("lt_node_check", a))
        return 0

    def lt_last_error(self):
        return b"mock"

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def mocked(monkeypatch):
    """A Baseline that never saw a device, over a fake library: (baseline, install(step_returns) -> fake)."""
    base = object.__new__(engine.Baseline)
    base.x = torch.zeros((10, 4))
    base.n, base._h = 10, 1234
    base._x_seen = engine._x_version(base.x)
    base._ws, base._host_scratch, base._fp64 = {}, {}, True
    base._shard = base._shard64 = None
    base._send64 = torch.zeros(1, dtype=torch.float64)
    base._s1d_full = torch.zeros(1, dtype=torch.float64)
    monkeypatch.setattr(engine, "_stream", lambda: None)
    monkeypatch.setattr(engine, "_pinned_f64", lambda r, c: torch.zeros((r, c), dtype=torch.float64))
    from linkteller_amd import dist
    monkeypatch.setattr(dist, "all_gather_into", lambda *a, **k: None)

    def install(step_returns):
        fake = _FakeLib(step_returns)
        monkeypatch.setattr(_lib, "lib", lambda: fake)
        return fake
    return base, install


PROBES, OBS = [1, 2, 3], [4, 5, 6, 7]


def test_one_library_call_per_step(mocked):
    base, install = mocked
    fake = install([0, 0, 0])
    m = base.influence_matrix_host(PROBES, OBS, 1e-4, "delta", refresh=True)
    assert m.shape == (3, 4) and m.dtype.name == "float64"
    assert fake.names() == ["lt_influence_workspace_bytes", "lt_influence_step_host"]      # (the first step sizes the workspace)
    for refresh, flags in ((True, 3), (False, 2)):
        fake.calls.clear()
        base.influence_matrix_host(PROBES, OBS, 1e-4, "delta", refresh=refresh)
        assert fake.names() == ["lt_influence_step_host"]
        a = fake.calls[0][1]
        assert len(a) == 17 and a[0] == 1234 and (a[2], a[4], a[6]) == (3, 4, 2) and a[14] == flags
        assert a[12] == next(iter(base._ws.values())).numel() == 4096


def test_exactly_one_retry_when_the_workspace_is_too_small(mocked):
    base, install = mocked
    fake = install([0, _lib.LT_ERR_WORKSPACE, 0])
    base.influence_matrix_host(PROBES, OBS, 1e-4, "delta", refresh=True)
    fake.calls.clear()
    base.influence_matrix_host(PROBES, OBS, 1e-4, "delta", refresh=True)
    assert fake.names() == ["lt_influence_step_host", "lt_influence_workspace_bytes", "lt_influence_step_host"]
    # refused twice: the error, not a loop
    fake = install([_lib.LT_ERR_WORKSPACE, _lib.LT_ERR_WORKSPACE, 0])
    with pytest.raises(_lib.LinkTellerHipError):
        base.influence_matrix_host(PROBES, OBS, 1e-4, "delta", refresh=True)
    assert fake.names().count("lt_influence_step_host") == 2


def test_index_error_comes_from_the_call_itself(mocked):
    base, install = mocked
    fake = install([_lib.LT_ERR_INDEX])
    with pytest.raises(IndexError):
        base.influence_matrix_host(PROBES, OBS, 1e-4, "delta", refresh=True)
    assert "lt_node_check" not in fake.names()


def test_sharded_refresh_keeps_the_separate_calls(mocked):
    base, install = mocked
    fake = install([])
    base._shard64 = (0, 5, 5)
    base.influence_matrix_host(PROBES, OBS, 1e-4, "delta", refresh=True)
    assert fake.names() == ["lt_baseline_refresh", "lt_baseline_refresh_rows_fp64", "lt_influence_workspace_bytes",
                            "lt_influence_matrix_host", "lt_node_check"]

"""engine._ProbeHandle, the base of ``Baseline``, ``Baseline3`` and ``Baseline2W``, as far as it goes without a GPU: on objects made
with ``object.__new__`` over a recording fake library (the stub style of test_wide2_handle_cpu.py / test_host_step_cpu.py)."""
import pytest
import torch

from linkteller_amd import _lib, engine

CLASSES = {engine.Baseline: "lt_baseline", engine.Baseline3: "lt_baseline3", engine.Baseline2W: "lt_baseline2w"}


class _Recorder:
    """every symbol exists, returns 0 and is recorded by name"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append(name)
            return 0
        return call


@pytest.fixture
def fake(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    monkeypatch.setattr(engine, "_stream", lambda: None)
    return lib


@pytest.mark.parametrize("cls", list(CLASSES), ids=lambda c: c.__name__)
def test_refresh_announces_changed_features_through_the_class_own_symbol(fake, cls):
    prefix = CLASSES[cls]
    base = object.__new__(cls)
    base.x, base._h = torch.zeros((4, 3)), 1234
    base._x_seen = engine._x_version(base.x)
    base._shard = base._shard64 = None
    base.refresh()
    assert fake.calls == [prefix + "_refresh"]                        # the version has not moved: no announcement
    base.x[0, 0] = 1.0                                                # an in-place edit moves torch's version counter
    base.refresh()
    assert fake.calls[1:] == [prefix + "_features_changed", prefix + "_refresh"]
    base.refresh()
    assert fake.calls[3:] == [prefix + "_refresh"]                    # announced once
    assert base.features_changed() is base and fake.calls[4:] == [prefix + "_features_changed"]


@pytest.mark.parametrize("short", ["b1", "b2"])
def test_baseline_refuses_a_short_bias_before_any_library_call(fake, monkeypatch, short):
    n, f, h, c = 6, 5, 4, 3
    monkeypatch.setattr(engine, "as_hip_graph", lambda adj: adj)
    monkeypatch.setattr(engine, "_f32", lambda t, name: t)              # (the tensors are CPU ones: the check under test is the shapes')
    sizes = {"b1": h, "b2": c}
    sizes[short] -= 1
    graph = type("G", (), {"n": n, "device_index": None, "handle": 1})()
    with pytest.raises(ValueError, match="inconsistent GCN shapes"):
        engine.Baseline(graph, torch.zeros((n, f)), torch.zeros((f, h)), torch.zeros(sizes["b1"]), torch.zeros((h, c)),
                        torch.zeros(sizes["b2"]))
    assert fake.calls == []

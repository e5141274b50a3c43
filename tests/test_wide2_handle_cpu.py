"""The one-handle route of the wide 2-layer attack (lt_baseline2w_*, lt_influence2w_*; engine.Baseline2W) as far as it goes without a
GPU: the declarations and bindings, the ABI's host-side refusals, ``engine.wide_class_shapes`` and the attacker's two routing
decisions (``Attacker.baseline`` and ``Attacker._pair_route``) on stub objects."""
import ctypes as C
import os
import re
import types

import pytest

from linkteller_amd import engine

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "linkteller_hip.h")
NAMES = ("lt_baseline2w_create", "lt_baseline2w_refresh", "lt_baseline2w_features_changed", "lt_baseline2w_destroy",
         "lt_baseline2w_logits", "lt_influence2w_workspace_bytes", "lt_influence2w_rows", "lt_influence2w_pairs_workspace_bytes",
         "lt_influence2w_pairs")
LT_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lt():
    from linkteller_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_names_declared_bound_and_refused_for_a_null_handle(lt):
    with open(HEADER) as f:
        text = f.read()
    assert "typedef struct lt_baseline2w lt_baseline2w;" in text
    h = lt.lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in lt.SIGNATURES and hasattr(h, name), name
    assert h.lt_abi_version() == 5 and lt.ABI_VERSION == 5
    assert h.lt_influence2w_workspace_bytes(None, 10, 10) == 0
    assert h.lt_influence2w_pairs_workspace_bytes(None, 10, 100) == 0
    ptr = (C.c_int64 * 2)(0, 1)
    assert h.lt_influence2w_rows(None, None, 1, None, 1, 1e-4, 2, None, 1, None, 0, None) == LT_ERR_INVALID
    assert b"baseline" in h.lt_last_error()
    assert h.lt_influence2w_pairs(None, None, 1, ptr, None, 1, 1e-4, 2, None, None, 0, None) == LT_ERR_INVALID
    assert b"baseline" in h.lt_last_error()
    assert h.lt_baseline2w_logits(None, None, None) == LT_ERR_INVALID
    assert h.lt_baseline2w_refresh(None, None) == LT_ERR_INVALID
    assert h.lt_baseline2w_features_changed(None, None) == LT_ERR_INVALID


@pytest.mark.parametrize("h, c, want", [(256, 9, True), (256, 8, False), (257, 9, False), (16, 256, True), (16, 257, False)])
def test_wide_class_shapes(h, c, want):
    assert engine.wide_class_shapes(h, c) is want


def test_baseline2w_is_its_own_class():
    assert not issubclass(engine.Baseline2W, engine.WideBaseline) and not issubclass(engine.Baseline2W, engine.Baseline)
    assert engine.Baseline2W.supports_sharding is False
    b = object.__new__(engine.Baseline2W)
    b.c = 41
    assert b.enable_fp64() is b and b.fp64_route() == -1 and b.shard_refresh() is b and b.shard_refresh_fp64(False) is b
    for mode in ("sparse", "full"):
        with pytest.raises(NotImplementedError):
            b.influence_rows([0], [0], 1e-4, mode)
        with pytest.raises(NotImplementedError):
            b.influence_pairs([0], [0, 1], [0], 1e-4, mode)


# ---- Attacker._pair_route ------------------------------------------------------------------------------------------------------------
def _stub(kind, cuda=True, env_mode=None, base2=None):
    """An Attacker whose model walk, features and baselines are stubs: ``_pair_route`` reads nothing else."""
    from linkteller_amd.attacker import Attacker
    atk = object.__new__(Attacker)
    atk.args = types.SimpleNamespace(influence=1e-4, influence_mode=env_mode)
    atk.features = types.SimpleNamespace(is_cuda=cuda)
    atk._walk = lambda: (kind, {})
    atk.baseline3 = lambda sd=None: None
    atk.seen = []
    atk.baseline = lambda mode=None, sd=None: (atk.seen.append(mode), base2)[1]
    return atk


@pytest.mark.parametrize("mode", ["delta", "sparse", "full"])
def test_pair_route_hands_back_a_baseline2w(mode, monkeypatch):
    monkeypatch.delenv("LT_INFLUENCE_MODE", raising=False)
    two = object.__new__(engine.Baseline2W)
    atk = _stub("gcn2", base2=two)
    assert atk._pair_route(mode) is two and atk.seen == [mode]          # whatever baseline() built for that mode
    assert _stub("gcn2", env_mode=mode, base2=two)._pair_route() is two
    assert _stub("gcn2", base2=object.__new__(engine.WideBaseline))._pair_route(mode) is None
    assert _stub("gcn2", cuda=False, base2=two)._pair_route(mode) is None


# ---- Attacker.baseline ---------------------------------------------------------------------------------------------------------------
class _T:
    """what baseline() reads of a parameter tensor"""

    def __init__(self, *shape):
        self.shape, self.device, self._version = shape, "dev", 0

    def data_ptr(self):
        return id(self)

    def to(self, dev):
        return self


class _Made:
    def __init__(self, kind):
        self.kind, self.refreshed = kind, []

    def refresh(self, mode=None):
        self.refreshed.append(mode)


def _chooser(monkeypatch, h, c, env_mode=None):
    """An Attacker whose ``baseline()`` runs for real on stub tensors, with the two constructors replaced by recorders."""
    from linkteller_amd import attacker as A
    made = []
    monkeypatch.setattr(engine, "Baseline2W", lambda *a: (made.append("2w"), _Made("2w"))[1])
    monkeypatch.setattr(engine, "baseline_for", lambda *a: (made.append("for"), _Made("for"))[1])
    monkeypatch.setattr(A.lt_dist, "choose_baseline_sharding", lambda base, mode=None: False)
    monkeypatch.setattr(A.lt_dist, "collectives_on", lambda: False)
    atk = object.__new__(A.Attacker)
    atk.args = types.SimpleNamespace(influence=1e-4, influence_mode=env_mode)
    atk.features = types.SimpleNamespace(device="dev", data_ptr=lambda: 1234)
    atk.adj = object()
    atk._baseline = atk._baseline_key = None
    params = [_T(32, h), _T(h), _T(h, c), _T(c)]
    atk._params = lambda sd=None: params
    return atk, made


def test_baseline_picks_the_handle_for_delta_with_wide_class_shapes_alone(monkeypatch):
    monkeypatch.delenv("LT_INFLUENCE_MODE", raising=False)
    monkeypatch.setenv("LT_WIDE2", "handle")
    sd = {}
    atk, made = _chooser(monkeypatch, 64, 121)
    assert atk.baseline("delta", sd).kind == "2w" and made == ["2w"]
    assert atk.baseline(None, sd).kind == "2w" and made == ["2w"]             # (`delta` is the default mode; cached, refreshed)
    assert atk._baseline.refreshed == ["delta"]
    # a switch of the mode on the same model rebuilds, through the fast path's check too, and back
    assert atk.baseline("sparse", sd).kind == "for" and made == ["2w", "for"]
    assert atk.baseline("full", sd).kind == "for" and made == ["2w", "for"]
    assert atk.baseline("delta", sd).kind == "2w" and made == ["2w", "for", "2w"]
    assert atk.baseline("delta").kind == "2w" and made == ["2w", "for", "2w"]     # (without a state_dict: the full key)
    for h, c in ((64, 8), (257, 41), (64, 257), (16, 1)):
        atk, made = _chooser(monkeypatch, h, c)
        assert atk.baseline("delta", sd).kind == "for" and made == ["for"], (h, c)
    for h, c in ((256, 9), (16, 256)):
        atk, made = _chooser(monkeypatch, h, c)
        assert atk.baseline("delta", sd).kind == "2w", (h, c)


def test_the_switches_keep_the_slice_route(monkeypatch):
    monkeypatch.delenv("LT_INFLUENCE_MODE", raising=False)
    monkeypatch.setenv("LT_WIDE2", "slices")
    atk, made = _chooser(monkeypatch, 64, 41)
    assert atk.baseline("delta", {}).kind == "for" and atk.baseline(None, {}).kind == "for" and made == ["for"]
    monkeypatch.setenv("LT_WIDE2", "handle")
    monkeypatch.setenv("LT_INFLUENCE_MODE", "sparse")
    atk, made = _chooser(monkeypatch, 64, 41)
    assert atk.baseline(None, {}).kind == "for" and made == ["for"]
    atk, made = _chooser(monkeypatch, 64, 41, env_mode="full")                    # the mode of the arguments
    assert atk.baseline(None, {}).kind == "for" and made == ["for"]

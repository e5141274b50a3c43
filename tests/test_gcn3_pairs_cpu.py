"""The pair list of the 3-layer model (lt_influence3_pairs) as far as it goes without a GPU: the ABI's host-side refusals and the
attacker's routing decision (``Attacker._pair_route``) on stub objects."""
import ctypes as C
import os
import types

import pytest

from linkteller_amd import engine


@pytest.fixture(scope="module")
def lt():
    from linkteller_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_gcn3_pairs_symbols_and_host_side_refusals(lt):
    h = lt.lib()
    for name in ("lt_influence3_pairs", "lt_influence3_pairs_workspace_bytes"):
        assert hasattr(h, name) and name in lt.SIGNATURES
    assert h.lt_abi_version() == 5
    ptr = (C.c_int64 * 2)(0, 1)
    assert h.lt_influence3_pairs(None, None, 1, ptr, None, 1, 1e-4, 2, None, None, 0, None) == -1
    assert b"baseline" in h.lt_last_error()
    assert h.lt_influence3_pairs_workspace_bytes(None, 10, 100) == 0


class _Three:
    """what ``baseline3()`` hands back for a stub attacker: an object with ``influence_pairs``"""

    def influence_pairs(self, *a, **k):
        raise AssertionError("the routing decision launches nothing")


def _stub(kind, cuda=True, env_mode=None, base2=None):
    """An Attacker whose model walk, features and baselines are stubs: ``_pair_route`` reads nothing else."""
    from linkteller_amd.attacker import Attacker
    atk = object.__new__(Attacker)
    atk.args = types.SimpleNamespace(influence=1e-4, influence_mode=env_mode)
    atk.features = types.SimpleNamespace(is_cuda=cuda)
    atk._walk = lambda: (kind, {})
    atk.three = _Three()
    atk.baseline3 = lambda sd=None: atk.three
    atk.baseline = lambda mode=None, sd=None: base2
    return atk


@pytest.mark.parametrize("mode", ["delta", "sparse", "full"])
def test_route_gcn3_takes_the_pair_list_in_every_mode(mode):
    atk = _stub("gcn3")
    assert atk._pair_route(mode) is atk.three
    assert _stub("gcn3", env_mode=mode)._pair_route() is not None      # the mode of the arguments, not of the call


def test_route_wide_gcn3_takes_the_pair_list_in_delta_alone(monkeypatch):
    monkeypatch.delenv("LT_INFLUENCE_MODE", raising=False)
    atk = _stub("gcn3w")
    assert atk._pair_route("delta") is atk.three
    assert atk._pair_route() is atk.three                              # (`delta` is the default mode)
    assert atk._pair_route("sparse") is None and atk._pair_route("full") is None
    assert _stub("gcn3w", env_mode="sparse")._pair_route() is None
    monkeypatch.setenv("LT_INFLUENCE_MODE", "sparse")
    assert atk._pair_route() is None


@pytest.mark.parametrize("mode", ["delta", "sparse", "full"])
def test_route_generic_stacks_and_cpu_features_keep_the_rectangle(mode):
    assert _stub("generic")._pair_route(mode) is None
    for kind in ("gcn2", "gcn3", "gcn3w", "generic"):
        assert _stub(kind, cuda=False)._pair_route(mode) is None
    # a 2-layer model: engine.Baseline has the list, whatever else baseline() builds (engine.WideBaseline) has not
    two = object.__new__(engine.Baseline)
    assert _stub("gcn2", base2=two)._pair_route(mode) is two
    assert _stub("gcn2", base2=object.__new__(engine.WideBaseline))._pair_route(mode) is None

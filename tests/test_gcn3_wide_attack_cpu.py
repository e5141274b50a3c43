"""The wide-class GCN3 attack without a GPU: lt_baseline3_create_wide is declared, bound and exported (the ABI version stays 5),
and Attacker._walk names the models the wide handle serves."""
import os
import re

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def lt():
    from linkteller_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_create_wide_declared_bound_and_exported(lt):
    src = open(os.path.join(REPO, "include", "linkteller_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(", code))
    h = lt.lib()
    name = "lt_baseline3_create_wide"
    assert name in declared and name in lt.SIGNATURES and hasattr(h, name)
    # same arguments, same handle type as the narrow entry point
    assert lt.SIGNATURES[name] == lt.SIGNATURES["lt_baseline3_create"]
    assert getattr(h, name).argtypes == lt.SIGNATURES[name][1]
    assert h.lt_abi_version() == lt.ABI_VERSION == 5
    assert "MODE RULE of a wide handle" in src


@pytest.mark.parametrize("shape,kind", [((30, 16, 8, 41), "gcn3w"), ((30, 16, 8, 8), "gcn3"), ((30, 16, 8, 9), "gcn3w"),
                                        ((30, 16, 8, 256), "gcn3w"), ((30, 300, 8, 41), "generic"),
                                        ((30, 16, 300, 41), "generic"), ((30, 16, 8, 257), "generic")])
def test_walk_names_the_wide_models(shape, kind):
    from linkteller_amd.attacker import Attacker
    from linkteller_amd.gcn import GCN3
    a = Attacker.__new__(Attacker)
    a.model = GCN3(*shape, 0.5)
    assert a._walk()[0] == kind
    assert a._walk()[0] == kind                          # (the cached walk)
    assert a._is_three_layer() == (kind == "gcn3")       # keeps its meaning: the narrow primitive

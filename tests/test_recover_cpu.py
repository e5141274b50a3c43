"""Edge recovery without a GPU: the host arithmetic of linkteller_amd/recover.py against hand-worked values of the reference's
post-processing script (attack_stats_all.py:44-116), the argument checks of lt_top_pairs_lower that happen before any device
call, and the command line's --recover / --density-belief."""
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


def test_density_ladder_hand_worked():
    from linkteller_amd import recover
    # 295 edges among 500 nodes: 295 / 124750 = 0.002365 -> x10 three times = 2.365 -> digit 2, rest 0.365 < 0.5 -> 2e-3
    lad = recover.density_ladder(295, 500)
    assert lad == [0.002 / 4, 0.002 / 2, 0.002, 0.002 * 2, 0.002 * 4]
    # 189 of the 25200 pairs of 225 nodes: 0.0075 -> 7.5 -> digit 7, rest 0.5 -> a half rounds UP -> 8e-3
    assert 189 / 25200 == 0.0075
    assert recover.density_ladder(189, 225)[2] == 0.008
    # 114 of the 120 pairs of 16 nodes: 0.95 -> 9.5 -> digit 9, rest 0.5 -> 10, exponent 1 -> 10 / 10 = 1.0
    assert 114 / 120 == 0.95
    lad = recover.density_ladder(114, 16)
    assert lad[2] == 1.0 and lad == [0.25, 0.5, 1.0, 2.0, 4.0]
    # a complete graph: the value is never scaled, digit 1, exponent 0
    assert recover.density_ladder(120, 16)[2] == 1.0
    # 0.0449.. -> 4.49 -> 4e-2 (no carry from the second digit)
    assert recover.density_ladder(56, 51)[2] == 0.04          # 56 / 1275 = 0.04392
    with pytest.raises(ValueError):
        recover.density_ladder(0, 500)
    with pytest.raises(ValueError):
        recover.density_ladder(3, 1)


def test_belief_counts_clip_and_ceil():
    from linkteller_amd import recover
    c = recover.belief_counts([0.5, 0.25, 0.26, 1e-9, 0.0, 1.0, 4.0, 0.01], 20)
    #            0.5 * 20 = 10 exactly -> 10 (ceil at an integer product adds nothing); 0.25 * 20 = 5; 0.26 * 20 = 5.2 -> 6
    assert c.dtype == np.int64 and c.tolist() == [10, 5, 6, 1, 1, 20, 20, 1]
    assert recover.belief_counts([0.01], 1770).tolist() == [18]          # 17.7 -> 18
    assert recover.belief_counts([0.002 * 4], 124750).tolist() == [998]
    with pytest.raises(ValueError):
        recover.belief_counts([0.1], 0)


def test_recovery_stats_hand_made():
    from linkteller_amd import recover
    ranked = [1, 0, 1, 1, 0, 0, 0, 1]
    s = recover.recovery_stats(ranked, 5, [1, 2, 4, 8])
    assert s["tp"].tolist() == [1, 1, 3, 4]
    assert np.array_equal(s["precision"], np.array([1.0, 0.5, 0.75, 0.5]))
    assert np.array_equal(s["recall"], np.array([0.2, 0.2, 0.6, 0.8]))
    assert np.allclose(s["f1"], [2 * 1.0 * 0.2 / 1.2, 2 * 0.5 * 0.2 / 0.7, 2 * 0.75 * 0.6 / 1.35, 2 * 0.5 * 0.8 / 1.3], rtol=1e-15)
    z = recover.recovery_stats([0, 0, 1], 2, [2, 3])            # tp = 0 at the first count: precision, recall and f1 are 0
    assert z["tp"].tolist() == [0, 1] and z["precision"][0] == 0 and z["recall"][0] == 0 and z["f1"][0] == 0
    assert z["f1"][1] == pytest.approx(2 * (1 / 3) * 0.5 / (1 / 3 + 0.5))
    with pytest.raises(ValueError):
        recover.recovery_stats([1, 0], 1, [3])
    with pytest.raises(ValueError):
        recover.recovery_stats([1, 0], 1, [0])


def test_recover_module_needs_no_gpu_import():
    import subprocess
    import sys
    from conftest import REPO
    code = "import sys; import linkteller_amd.recover; assert 'torch' not in sys.modules and 'linkteller_amd.engine' not in sys.modules"
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1000:]


def test_top_pairs_argument_errors(lt):
    h = lt.lib()
    q = h.lt_top_pairs_workspace_bytes
    assert q(500, 998) > 0 and q(2, 1) > 0 and q(2000, 1999000) >= q(500, 998)
    assert q(1, 1) == 0 and q(0, 1) == 0 and q(-3, 1) == 0
    assert q(500, 0) == 0 and q(500, -1) == 0 and q(500, 124751) == 0 and q(500, 124750) > 0
    # host memory stands in for the device pointers: every check below returns before anything is enqueued or dereferenced
    buf = np.zeros(1 << 16, dtype=np.int64)
    p = buf.ctypes.data
    need = q(8, 5)

    def call(scores=p, lds=8, n=8, m=5, idx=p, val=p, info=p, ws=p, ws_bytes=buf.nbytes):
        return h.lt_top_pairs_lower(scores, lds, n, m, idx, val, info, ws, ws_bytes, None)

    for kw in (dict(scores=None), dict(idx=None), dict(val=None), dict(info=None), dict(ws=None)):
        assert call(**kw) == -1 and b"NULL" in h.lt_last_error(), kw
    assert call(n=1, lds=1, m=1) == -1 and b"n >= 2" in h.lt_last_error()
    assert call(n=0, lds=1, m=1) == -1
    assert call(lds=7) == -1 and b"lds" in h.lt_last_error()
    assert call(m=0) == -1 and b"outside" in h.lt_last_error()
    assert call(m=29) == -1 and b"[1, 28]" in h.lt_last_error()
    assert call(m=-4) == -1
    assert call(ws_bytes=need - 1) == -1 and b"workspace" in h.lt_last_error()
    assert call(ws=p + 4) == -1 and b"aligned" in h.lt_last_error()
    assert call(ws_bytes=0) == -1


def test_cli_recover_flags():
    from linkteller_amd import main as lt_main
    a = lt_main.get_arguments([])
    assert a.recover is False and a.density_belief == 0.0
    a = lt_main.get_arguments("--attack --attack-mode efficient --sample-type unbalanced --recover --density-belief 0.01".split())
    assert a.recover is True and a.density_belief == 0.01
    lt_main.check_recover(a)                       # the served combination passes


@pytest.mark.parametrize("argv", [
    "--test --attack --recover --attack-mode naive --sample-type unbalanced",
    "--test --attack --recover --attack-mode baseline --sample-type unbalanced",
    "--test --attack --recover --attack-mode efficient --sample-type balanced-full",
    "--test --recover --attack-mode efficient --sample-type unbalanced",          # no --attack
])
def test_cli_recover_refused_before_a_worker_is_built(argv, monkeypatch):
    from linkteller_amd import main as lt_main, worker

    def boom(*a, **k):
        raise AssertionError("a Worker was built")
    monkeypatch.setattr(worker, "Worker", boom)
    monkeypatch.setattr(lt_main, "init_distributed", boom)
    with pytest.raises(NotImplementedError, match="--recover"):
        lt_main.main(argv.split())

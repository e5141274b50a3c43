"""Row bands of the baseline attacks' correlation square without a GPU: the three entry points (lt_corr_rows_workspace_bytes,
lt_corr_rows_prepare, lt_corr_rows) are declared, exported and bound; their argument checks happen before any device call; and the
command line's ``--baseline-scores stream`` is the device route that also admits --recover-chunk / --recover-nodes all."""
import argparse
import os
import re

import numpy as np
import pytest

NAMES = ("lt_corr_rows_workspace_bytes", "lt_corr_rows_prepare", "lt_corr_rows")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lt():
    from linkteller_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_symbols_declared_exported_and_bound(lt):
    with open(os.path.join(ROOT, "include", "linkteller_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define LT_ABI_VERSION 5\b", header)                 # additive: the version stays
    h = lt.lib()
    for name in NAMES:
        assert re.search(rf"^(size_t|int) {name}\(", header, flags=re.M), name
        assert name in lt.SIGNATURES, name
        assert getattr(h, name) is not None, name
    # the bound argument counts are the header's
    for name in NAMES:
        decl = re.search(rf"^(?:size_t|int) {name}\((.*?)\);", header, flags=re.M | re.S).group(1)
        assert len(lt.SIGNATURES[name][1]) == decl.count(",") + 1, name


def test_workspace_query(lt):
    q = lt.lib().lt_corr_rows_workspace_bytes
    assert q(0, 4, 1, 1) == 0 and q(4, 0, 1, 1) == 0 and q(4, 4, -1, 1) == 0 and q(4, 4, 1, -1) == 0 and q(-1, -1, -1, -1) == 0
    assert q(4385, 7, 0, 0) > 0                                             # empty list: still a valid (minimal) size
    for n, D, k in ((200, 7, 130), (200, 259, 130), (200, 3170, 130), (4385, 3170, 4385), (89250, 500, 89250)):
        sizes = [q(n, D, k, r) for r in sorted((0, 1, 63, 64, 65, 128, 129, 1024, k))]
        assert sizes[0] >= 8 * (D + k) and all(a <= b for a, b in zip(sizes, sizes[1:])), (n, D, k, sizes)
    # several K slices (130 rows, 17 staging steps): the band's partial tiles make the size follow max_rows ...
    assert q(200, 259, 130, 65) > q(200, 259, 130, 64) > q(200, 259, 130, 0)
    # ... one slice (thousands of tiles): nothing but the head, and nothing that grows with k^2
    assert q(89250, 500, 89250, 1024) == q(89250, 500, 89250, 0) < 8 * (500 + 1024 * 500 + 89250 + 8)


def test_argument_errors_come_before_any_device_call(lt):
    h = lt.lib()
    q = h.lt_corr_rows_workspace_bytes
    # host memory stands in for the device pointers: every check below returns before anything is enqueued or dereferenced
    buf = np.zeros(1 << 20, dtype=np.int64)
    p = buf.ctypes.data

    def prep(V=p, ldv=259, n=200, D=259, nodes=p, k=130, info=p, ws=p, ws_bytes=buf.nbytes):
        return h.lt_corr_rows_prepare(V, ldv, n, D, nodes, k, info, ws, ws_bytes, None)

    def rows(V=p, ldv=259, n=200, D=259, nodes=p, k=130, row_begin=0, n_rows=64, n_cols=130, out=p, ldo=130, ws=p,
             ws_bytes=buf.nbytes):
        return h.lt_corr_rows(V, ldv, n, D, nodes, k, row_begin, n_rows, n_cols, out, ldo, ws, ws_bytes, None)

    for kw in (dict(V=None), dict(nodes=None), dict(info=None), dict(ws=None)):
        assert prep(**kw) == -1 and b"NULL" in h.lt_last_error(), kw
    for kw in (dict(V=None), dict(nodes=None), dict(out=None), dict(ws=None)):
        assert rows(**kw) == -1 and b"NULL" in h.lt_last_error(), kw
    for call in (prep, rows):
        assert call(n=0) == -1 and call(n=-3) == -1 and call(D=0) == -1 and call(D=-1, ldv=-1) == -1 and call(k=-1) == -1
        assert call(ldv=258) == -1 and b"ldv" in h.lt_last_error()
        assert call(ws=p + 4) == -1 and b"aligned" in h.lt_last_error()
        assert call(ws_bytes=0) == -1 and b"workspace" in h.lt_last_error()
    head = q(200, 259, 130, 0)
    assert prep(ws_bytes=head - 1) == -1 and b"workspace" in h.lt_last_error()
    assert rows(ldo=129) == -1 and b"ldo" in h.lt_last_error()
    assert rows(n_cols=64, ldo=63) == -1 and b"ldo" in h.lt_last_error()
    assert rows(row_begin=-1) == -1 and rows(n_rows=-1) == -1
    assert rows(row_begin=67, n_rows=64) == -1 and b"rows" in h.lt_last_error()          # 67 + 64 > 130
    assert rows(row_begin=131, n_rows=0) == -1
    assert rows(row_begin=2 ** 31 - 1, n_rows=2 ** 31 - 1, k=2 ** 31 - 1) == -1           # the sum does not wrap
    assert rows(n_cols=-1) == -1 and b"n_cols" in h.lt_last_error()
    assert rows(n_cols=131, ldo=131) == -1 and b"n_cols" in h.lt_last_error()
    # a band longer than the max_rows the workspace was sized for, and a short workspace
    assert q(200, 259, 130, 64) < q(200, 259, 130, 65)
    assert rows(n_rows=65, ws_bytes=q(200, 259, 130, 64)) == -1 and b"max_rows" in h.lt_last_error()
    assert rows(n_rows=64, ws_bytes=q(200, 259, 130, 64) - 1) == -1 and b"workspace" in h.lt_last_error()
    # empty bands: successful no-ops, nothing is enqueued
    assert rows(n_rows=0) == 0 and rows(n_cols=0, ldo=0) == 0 and rows(row_begin=130, n_rows=0) == 0
    assert rows(k=0, n_rows=0, n_cols=0) == 0 and prep(k=0) == 0


# ---- the command line -----------------------------------------------------------------------------------------------------------
def _args(s):
    from linkteller_amd import main as lt_main
    return lt_main.get_arguments(s.split())


def test_cli_stream_choice_parses_and_is_admitted():
    from linkteller_amd import main as lt_main
    assert _args("--baseline-scores stream").baseline_scores == "stream"
    for am in ("baseline", "baseline-feat"):
        for st in ("unbalanced", "unbalanced-lo", "unbalanced-hi"):
            for extra in ("", " --recover-chunk 64", " --recover-nodes all", " --recover-nodes all --recover-chunk 64"):
                a = _args(f"--test --attack --attack-mode {am} --sample-type {st} --baseline-scores stream --recover" + extra)
                lt_main.check_baseline_scores(a)
                lt_main.check_recover(a)
                lt_main.check_recover_stream(a)
            a = _args(f"--test --attack --attack-mode {am} --sample-type {st} --baseline-scores stream --metrics-only")
            lt_main.check_baseline_scores(a)
            lt_main.check_metrics_only(a)
        # everything 'device' serves: the pair lists of balanced-full under --metrics-only
        b = _args(f"--test --attack --attack-mode {am} --sample-type balanced-full --baseline-scores stream --metrics-only")
        lt_main.check_baseline_scores(b)
        lt_main.check_metrics_only(b)
        # 'device' and 'host' keep refusing the chunked route
        for route in ("device", "host"):
            with pytest.raises(NotImplementedError, match="--recover"):
                lt_main.check_recover_stream(_args(f"--attack --attack-mode {am} --sample-type unbalanced --baseline-scores {route} "
                                                   "--recover --recover-chunk 8"))
    # the chunk's own checks still hold under 'stream'
    with pytest.raises(ValueError, match="--recover-chunk"):
        lt_main.check_recover_stream(_args("--attack --attack-mode baseline --baseline-scores stream --recover --recover-chunk -3"))
    with pytest.raises(NotImplementedError, match="--recover"):
        lt_main.check_recover_stream(_args("--attack --attack-mode baseline --baseline-scores stream --recover-chunk 8"))


@pytest.mark.parametrize("argv,match", [
    ("--test --attack --attack-mode efficient --sample-type unbalanced --baseline-scores stream", "--baseline-scores"),
    ("--test --attack --attack-mode naive --sample-type unbalanced --baseline-scores stream", "--baseline-scores"),
    ("--test --attack-mode baseline --sample-type unbalanced --baseline-scores stream", "--baseline-scores"),
    ("--test --attack --recover --attack-mode baseline --sample-type balanced-full --baseline-scores stream", "--recover"),
    ("--test --attack --recover --recover-chunk 64 --attack-mode baseline-feat --sample-type balanced-full --baseline-scores stream",
     "--recover"),
])
def test_cli_stream_refusals_come_before_a_worker_is_built(argv, match, monkeypatch):
    from linkteller_amd import main as lt_main, worker

    def boom(*a, **k):
        raise AssertionError("a Worker was built")
    monkeypatch.setattr(worker, "Worker", boom)
    monkeypatch.setattr(lt_main, "init_distributed", boom)
    with pytest.raises(NotImplementedError, match=match):
        lt_main.main(argv.split())


def test_trainer_whole_graph_line_follows_the_flag(monkeypatch):
    """GCNTrainer._recover_whole_graph reaches the Attacker for a baseline attack with baseline_scores = stream and refuses
    host (and device, whose square is formed in one piece); eval_output's sampled line treats stream as a device route."""
    from linkteller_amd import trainer as lt_trainer

    class Reached(Exception):
        pass

    def attacker(**kw):
        raise Reached()
    monkeypatch.setattr(lt_trainer, "Attacker", attacker)
    t = lt_trainer.GCNTrainer.__new__(lt_trainer.GCNTrainer)
    t.model = t.worker = None
    for am in ("baseline", "baseline-feat"):
        for st in ("unbalanced", "unbalanced-lo", "unbalanced-hi"):
            t.args = argparse.Namespace(attack=True, recover=True, recover_nodes="all", recover_chunk=64, attack_mode=am,
                                        sample_type=st, baseline_scores="stream")
            with pytest.raises(Reached):
                t._recover_whole_graph()
            with pytest.raises(Reached):
                t.eval_output(None)
            t.args.recover_nodes = "sample"
            with pytest.raises(Reached):
                t.eval_output(None)
            for route in ("host", "device"):
                t.args.baseline_scores, t.args.recover_nodes = route, "all"
                with pytest.raises(NotImplementedError, match="recover"):
                    t._recover_whole_graph()
        t.args = argparse.Namespace(attack=True, recover=True, recover_nodes="all", attack_mode=am, sample_type="balanced-full",
                                    baseline_scores="stream")
        with pytest.raises(NotImplementedError, match="recover"):
            t._recover_whole_graph()


def test_attacker_route_names():
    """``_baseline_route``: 'stream' is the device route; anything unknown is still a ValueError; the chunked call refuses the host
    route before it touches the GPU."""
    import types
    import scipy.sparse as sp
    import torch
    from linkteller_amd.attacker import Attacker
    w = types.SimpleNamespace(features_2=torch.zeros(4, 3), adj_2=None, adj_ori=sp.identity(4, format="csr"), n_nodes=4)
    args = argparse.Namespace(dataset="twitch/x", sample_type="unbalanced", n_test=4, attack_mode="baseline-feat",
                              baseline_scores="stream")
    atk = Attacker(args, None, w)
    assert atk._baseline_route() == "device"
    args.baseline_scores = "device"
    assert atk._baseline_route() == "device"
    args.baseline_scores = "host"
    assert atk._baseline_route() == "host"
    with pytest.raises(NotImplementedError, match="baseline_scores"):
        atk._stream_scores(None, torch.zeros(4, dtype=torch.int32), 3, 2)
    args.baseline_scores = "gpu"
    with pytest.raises(ValueError, match="baseline_scores"):
        atk._baseline_route()

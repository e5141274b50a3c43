"""The bits of the three probe handles (lt_baseline_* / lt_baseline3_* / lt_baseline2w_*; engine.Baseline, Baseline3, Baseline2W),
pinned: per case the SHA-256 of the raw bytes of every result -- logits(), a rectangle of influence_rows, a list of influence_pairs --
against tests/golden/probe_bits.json.  The pair lists' scores are kept word for word as well, so a failure says where.  The other
tests of these handles compare with the fp64 oracle under gates or the library with itself; this file is what notices a changed bit.

The digests belong to the pinned toolchain.  The committed file was written once, on the MI355X, from the library built at the PARENT
COMMIT of the change that folded the three handles onto one engine base and one exact chain (the hash is in the file, key
"parent_commit"), and is never rewritten from the code under test: a digest that differs after a change that claims to keep the bits
is a bug in that change.  A toolchain change regenerates the file from the then-current main branch:

    python tests/test_probe_bits_gpu.py --write --parent COMMIT [--lib path/to/liblinkteller_hip.so] [--out path/to/probe_bits.json]

(``--parent`` is the hash of the commit the library was built from, recorded in the file; ``--lib`` binds the package to another
build of the library, ``--out`` writes elsewhere than tests/golden/).

Cases, on the small graphs `er` and `loops` of the case modules (wide2_shape_cases for two layers, gcn3_shape_cases for three):
    Baseline        (H, C) = (13, 3): pad columns, the fused class epilogue          full, sparse, delta
    Baseline3       (30, 19, 7) narrow                                                sparse, delta
    Baseline3       (30, 19, 11) and (21, 14, 65) wide                                delta
    Baseline2W      (7, 33) and (13, 129)                                             delta
Lists: twelve probes (the all-zero feature row, a repeated probe; on `loops` the isolated node and two self loops), the graph's
observed list (repeated ids, u == v), and a grouped pair list in which probe 2 owns no pair and probes 5 .. 9 -- a whole chunk of the
forced chunking below -- own none.

Settings, every combination, reset in a ``finally``:
    chunk_budget_bytes   default (one chunk), and five probes' worth: chunks of 5, 5 and 2 probes.  Every carve (carve_infl, carve3,
                         carve2w) takes chunk = budget / per_probe clamped to [1, min(65534, n_probe)], per_probe a function of the
                         handle and the mode alone; the test finds per_probe from the library's own workspace query -- the smallest
                         budget at which twelve probes' workspace grows past the one-probe-per-chunk size is 2 * per_probe -- and
                         then asserts the steps of that query at 5 and 6 probes' worth, so the chunk IS five.
    gcn3_product_gather  0 and 1, on the handles that read it (Baseline3 `delta`, Baseline2W)
and, per handle and mode once, after W1 was scaled in place on its even columns and refresh() called."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import boundary_cases as B      # noqa: F401  (the case modules below build on it)
import gcn3_shape_cases as S3
import wide2_shape_cases as S2

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_bits.json")
DELTA = 1e-4
N_PROBE, CHUNK = 12, 5
# name -> (class, shape, modes)
HANDLES = {
    "b2": ("Baseline", (13, 3), ("full", "sparse", "delta")),
    "b3": ("Baseline3", (30, 19, 7), ("sparse", "delta")),
    "b3w11": ("Baseline3", (30, 19, 11), ("delta",)),
    "b3w65": ("Baseline3", (21, 14, 65), ("delta",)),
    "b2w33": ("Baseline2W", (7, 33), ("delta",)),
    "b2w129": ("Baseline2W", (13, 129), ("delta",)),
}
GRAPHS = ("er", "loops")
CASES = [f"{h}.{g}" for h in HANDLES for g in GRAPHS]


def _inputs(handle, graph):
    """(a_hat, x, params in call order, probes [12], observed, (pair_ptr, pair_obs))"""
    _, shape, _ = HANDLES[handle]
    if len(shape) == 3:
        a_hat, x, probes, obs, zrow = S3.small_graph(graph)
        p = S3.small_params(graph, shape)
        params = [p[k] for k in S3.KEYS]
    else:
        a_hat, x, probes, obs, zrow = S2.small_graph(graph)
        p = S2.small_params(shape)
        params = [p[k] for k in S2.KEYS]
    pl = np.concatenate([probes[:8], probes[3:4], probes[-3:]]).astype(np.int32)
    assert zrow < 8 and len(pl) == N_PROBE and len(set(pl)) < len(pl) and len(set(obs)) < len(obs)
    rng = np.random.RandomState(91)
    counts = rng.randint(3, 8, N_PROBE)
    counts[2] = 0
    counts[CHUNK:2 * CHUNK] = 0
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pobs = obs[rng.randint(0, len(obs), int(ptr[-1]))].astype(np.int32)
    return a_hat, x, params, pl, obs, (ptr, pobs)


def _ws_bytes(base, mode):
    """the rectangle's workspace for twelve probes and one observed node under the current knobs (host arithmetic)"""
    from linkteller_amd import _lib
    name = type(base).__name__
    if name == "Baseline":
        return _lib.lib().lt_influence_workspace_bytes(base._h, N_PROBE, 1, _lib.MODES[mode])
    query = _lib.lib().lt_influence3_workspace_bytes if name == "Baseline3" else _lib.lib().lt_influence2w_workspace_bytes
    return query(base._h, N_PROBE, 1)


def chunk_budget(base, mode):
    """The chunk_budget_bytes that makes chunks of CHUNK probes on this handle in this mode (see the module docstring)."""
    from linkteller_amd import _lib

    def at(budget):
        _lib.set_tuning("chunk_budget_bytes", budget)
        return _ws_bytes(base, mode)
    one = at(1)
    lo, hi = 1, 1 << 30                 # at(lo) == one < at(hi)
    assert at(hi) > one
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if at(mid) == one else (lo, mid)
    assert hi % 2 == 0
    per = hi // 2
    assert at(CHUNK * per - 1) < at(CHUNK * per) == at((CHUNK + 1) * per - 1) < at((CHUNK + 1) * per), (type(base).__name__, mode, per)
    return CHUNK * per


def arrays_of(case):
    """{key: array} of one case: every setting's rectangle and pair scores, the logits, and the same after an edit of W1."""
    import torch
    from linkteller_amd import _lib, engine, graph
    handle, gname = case.split(".")
    cls, shape, modes = HANDLES[handle]
    a_hat, x, params, probes, obs, (ptr, pobs) = _inputs(handle, gname)
    dev = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in params]
    base = getattr(engine, cls)(graph.HipGraph(a_hat), torch.from_numpy(x).cuda(), *dev)
    assert getattr(base, "wide", False) == (handle.startswith("b3w"))
    out = {"logits": base.logits().cpu().numpy()}

    def both(tag, mode):
        out[f"{tag}.rows"] = base.influence_rows(probes, obs, DELTA, mode).cpu().numpy()
        out[f"{tag}.pairs"] = base.influence_pairs(probes, ptr, pobs, DELTA, mode).cpu().numpy()
    try:
        for mode in modes:
            gathers = (1, 0) if mode == "delta" and cls != "Baseline" else (None,)
            small = chunk_budget(base, mode)
            for budget, btag in ((None, "one"), (small, "split")):
                for gather in gathers:
                    _lib.set_tuning("chunk_budget_bytes", budget)
                    _lib.set_tuning("gcn3_product_gather", gather)
                    both(f"{mode}.{btag}" + ("" if gather is None else f".g{gather}"), mode)
        _lib.set_tuning("chunk_budget_bytes", None)
        _lib.set_tuning("gcn3_product_gather", None)
        dev[0][:, ::2] *= 1.25          # in place: torch's version counter of W1 moves, the features' does not
        base.refresh()
        out["w1.logits"] = base.logits().cpu().numpy()
        for mode in modes:
            both(f"w1.{mode}", mode)
    finally:
        _lib.set_tuning("chunk_budget_bytes", None)
        _lib.set_tuning("gcn3_product_gather", None)
    return out


def table_of(case):
    """{"sha256": {key: digest}, "words": {key: [uint32]}} of one case: the digest of every array, the words of the pair scores."""
    arrays = {k: np.ascontiguousarray(a) for k, a in sorted(arrays_of(case).items())}
    assert all(a.dtype == np.float32 for a in arrays.values())
    return {"sha256": {k: hashlib.sha256(a.tobytes()).hexdigest() for k, a in arrays.items()},
            "words": {k: [int(w) for w in a.reshape(-1).view(np.uint32)] for k, a in arrays.items() if k.endswith(".pairs")}}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case", CASES)
def test_bits_are_the_pinned_ones(golden, case):
    got, want = table_of(case), golden[case]
    assert sorted(got["sha256"]) == sorted(want["sha256"]) and sorted(got["words"]) == sorted(want["words"])
    bad = []
    for k, digest in got["sha256"].items():
        if digest == want["sha256"][k]:
            continue
        g, w = got["words"].get(k), want["words"].get(k)
        if g is None or len(g) != len(w):
            bad.append(k)
            continue
        diff = [i for i in range(len(g)) if g[i] != w[i]]
        bad.append(f"{k}: {len(diff)} of {len(g)} words differ, first " + ", ".join(f"[{i}] {g[i]:#010x} != {w[i]:#010x}" for i in diff[:4]))
    assert not bad, f"case {case}: " + "; ".join(bad)


def write(out_file, parent):
    with open(out_file, "w") as fh:
        fh.write("{\n" + json.dumps("parent_commit") + ":" + json.dumps(parent) + ",\n")
        for i, case in enumerate(CASES):      # one case per line
            fh.write(json.dumps(case) + ":" + json.dumps(table_of(case), separators=(",", ":")) + (",\n" if i + 1 < len(CASES) else "\n"))
            print(case, "done", flush=True)
        fh.write("}\n")
    print("wrote", out_file, os.path.getsize(out_file), "bytes")


if __name__ == "__main__":
    if "--write" not in sys.argv or "--parent" not in sys.argv:
        sys.exit("usage: python tests/test_probe_bits_gpu.py --write --parent COMMIT [--lib LIBRARY] [--out FILE]")
    if "--lib" in sys.argv:
        from linkteller_amd import _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
        print("library:", _lib.LIB_PATH)
    write(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN_FILE, sys.argv[sys.argv.index("--parent") + 1])

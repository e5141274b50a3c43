"""The bits of the 2-layer trainer with the wide head (lt_gcn2_trainer_create_wide; engine.GCN2Trainer(head="wide")), pinned in
the manner of test_train_bits_gpu.py, which was written before the wide head existed: per case the SHA-256 of the raw bytes of
every array a training leaves behind, against tests/golden/train_wide_bits.json.  Small arrays are kept word for word as well,
so a failure says where.

The committed file was written once, from the library built from the commit BEFORE the wide route's launchers took their layer
indices from the trainer's depth (the change that lets GCN3 train with the wide head), and is never rewritten from the code
under test: a digest that differs after a change that claims to keep the bits is a bug in that change.  A toolchain change
regenerates the file from the then-current main branch:

    python tests/test_train_wide_bits_gpu.py --write [--lib path/to/liblinkteller_hip.so] [--out path/to/train_wide_bits.json]

Cases: W9, W41, W65, W121 and W256ce of train_wide_cases.py at p as given (both losses, every lane-group width of the head, a
directed and a power-law graph with hub rows, C > H).
    run A  run(4): the loss / tp record, grads(), logits(), hidden(), counts(), the four parameters afterwards
    run B  a fresh trainer, validation attached on the training graph with keep_best and patience 2, run_validated(6): loss,
           val_loss, val_counts, best_epoch, stop_epoch, the 8 state words, val_logits(), the parameters after restore_best()
    run C  run B with the head over every third node id in descending order and the first id once more"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import train_wide_cases as KW

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_wide_bits.json")
CASES = ["W9", "W41", "W65", "W121", "W256ce"]
WORD_KEYS = ("record", "counts", "loss", "val_loss", "val_counts", "best_epoch", "stop_epoch", "val_state")   # kept word for word
PLAIN_EPOCHS, VAL_EPOCHS, PATIENCE = 4, 6, 2


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _trainer(case):
    from linkteller_amd import engine
    params = [_dev(p.copy()) for p in case["params"]]
    return engine.GCN2Trainer(case["adj"], _dev(case["x"]), _dev(case["y"]), *params, lr=KW.LR, weight_decay=KW.DECAY,
                              dropout=case["p"], seed=KW.SEED, head="wide", loss=case["loss"])


def _validated(case, out, tag, rows):
    from linkteller_amd import engine
    tr = _trainer(case)
    tr.attach_validation(case["adj"], _dev(case["x"]), _dev(case["y"]), keep_best=True, patience=PATIENCE, rows=rows)
    res = tr.run_validated(VAL_EPOCHS)
    out[f"{tag}.loss"] = res["loss"]
    out[f"{tag}.val_loss"] = res["val_loss"]
    out[f"{tag}.val_counts"] = res["val_counts"]
    out[f"{tag}.best_epoch"] = np.array([res["best_epoch"]], dtype=np.int32)
    out[f"{tag}.stop_epoch"] = np.array([res["stop_epoch"]], dtype=np.int32)
    words = (C.c_int32 * 8)()
    tr._call("val_state", words, engine._stream())
    out[f"{tag}.val_state"] = np.array(list(words), dtype=np.int32)
    out[f"{tag}.val_logits"] = tr.val_logits().cpu().numpy()
    tr.restore_best()
    for k, p in enumerate(tr.params):
        out[f"{tag}.param{k}"] = p.cpu().numpy()


def arrays_of(name):
    """{key: array} of one case's runs A, B and C."""
    case = KW.make(name)
    out = {}
    tr = _trainer(case)
    out["a.record"] = tr.run_async(PLAIN_EPOCHS).cpu().numpy()
    for k, g in enumerate(tr.grads()):
        out[f"a.grad{k}"] = g.cpu().numpy()
    out["a.logits"] = tr.logits().cpu().numpy()
    out["a.hidden"] = tr.hidden().cpu().numpy()
    out["a.counts"] = tr.counts().cpu().numpy()
    for k, p in enumerate(tr.params):
        out[f"a.param{k}"] = p.cpu().numpy()
    del tr
    _validated(case, out, "b", None)
    ids = np.arange(case["n"] - 1, -1, -3)
    _validated(case, out, "c", np.concatenate([ids, ids[:1]]).astype(np.int64))
    return out


def table_of(name):
    """{"sha256": {key: digest}, "words": {key: [uint32]}} of one case: the digest of every array, the words of the small ones."""
    arrays = {k: np.ascontiguousarray(a) for k, a in sorted(arrays_of(name).items())}
    assert all(a.dtype.itemsize == 4 for a in arrays.values())
    return {"sha256": {k: hashlib.sha256(a.tobytes()).hexdigest() for k, a in arrays.items()},
            "words": {k: [int(w) for w in a.reshape(-1).view(np.uint32)] for k, a in arrays.items() if k.split(".")[1] in WORD_KEYS}}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", CASES)
def test_wide_bits_are_the_pinned_ones(golden, name):
    got, want = table_of(name), golden[name]
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
    assert not bad, f"case {name}: " + "; ".join(bad)


def write(out_file):
    with open(out_file, "w") as fh:
        fh.write("{\n")
        for i, name in enumerate(CASES):      # one case per line
            fh.write(json.dumps(name) + ":" + json.dumps(table_of(name), separators=(",", ":")) + (",\n" if i + 1 < len(CASES) else "\n"))
            print(name, "done")
        fh.write("}\n")
    print("wrote", out_file, os.path.getsize(out_file), "bytes")


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit("usage: python tests/test_train_wide_bits_gpu.py --write [--lib LIBRARY] [--out FILE]")
    if "--lib" in sys.argv:
        from linkteller_amd import _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
        print("library:", _lib.LIB_PATH)
    write(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN_FILE)

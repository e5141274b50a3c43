"""The GraphSAINT dataset family (flickr / reddit / ppi / ppi-large: one graph with a train / validation / test split of its
nodes) on the host: the loader and ``Worker`` against the reference's outputs, ``engine.f1_from_confusion`` against sklearn,
the refusals that precede any GPU work, and the new exports.  CPU only."""
import argparse
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import REPO, load_golden
from linkteller_amd import _lib, engine, main as lt_main, synth

NEW_SYMBOLS = ("lt_eval_head_rows_workspace_bytes", "lt_eval_head_rows", "lt_gcn2_trainer_attach_validation_rows",
               "lt_gcn3_trainer_attach_validation_rows")


@pytest.fixture(scope="module")
def gold():
    return load_golden("graphsaint_loader.npz")


def _csr(g, prefix):
    return sp.csr_matrix((g[prefix + ".data"], g[prefix + ".indices"], g[prefix + ".indptr"]), shape=tuple(g[prefix + ".shape"]))


def _write(g, root, name, as_name=None):
    roles = {k: g[f"in.role.{k}"].tolist() for k in ("tr", "va", "te")}
    synth.write_graphsaint_dataset(str(root), as_name or name, _csr(g, "in.adj"), g["in.feats"], g[f"in.labels.{name}"], roles)


def _args(**kw):
    base = dict(mode="vanilla-clean", norm="FirstOrderGCN", perturb_type="continuous", epsilon=5.0, noise_seed=42,
                noise_type="laplace", delta=1e-5)
    base.update(kw)
    return argparse.Namespace(**base)


def _same_csr(a, g, prefix):
    a = sp.csr_matrix(a)
    a.sort_indices()
    assert str(a.dtype) == str(g[prefix + ".dtype"]), prefix
    assert list(a.shape) == g[prefix + ".shape"].tolist(), prefix
    assert np.array_equal(a.indptr, g[prefix + ".indptr"]) and np.array_equal(a.indices, g[prefix + ".indices"]), prefix
    assert np.array_equal(a.data, g[prefix + ".data"]), prefix


def test_fixture_is_the_case_it_claims(gold):
    assert gold["flickr.sizes"].tolist() == [60, 12, 7, 1] and gold["ppi.sizes"].tolist() == [60, 12, 5, 5]
    y, tr = gold["flickr.labels"], gold["flickr.idx_train"]
    assert y.shape == (60, 1) and y.dtype == np.int64 and 6 not in set(y[tr, 0]) and y.max() == 6      # one class never trained on
    assert gold["ppi.labels"].shape == (60, 5)
    assert int((np.diff(gold["flickr.adj_train_raw.indptr"]) == 0).sum()) >= 2                           # isolated in the subgraph
    for k in ("idx_train", "idx_val", "idx_test"):
        assert np.all(np.diff(gold[f"flickr.{k}"]) > 0)
    assert not np.all(np.diff(gold["in.role.tr"]) > 0)                                                   # stored unsorted


@pytest.mark.parametrize("name", ["flickr", "ppi"])
def test_worker_matches_reference_loader(gold, name, tmp_path, monkeypatch):
    """``tests/golden/graphsaint_loader.npz`` holds what the REFERENCE's ``feature_reader`` / ``graph_reader`` / ``Worker``
    (utils/load.py:115-148, 209-216, 485-488; worker.py:425-441, 532-541, 615-629) produced from files rebuilt here from the
    stored inputs: every attribute must be equal bit for bit."""
    from linkteller_amd import worker as W
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _write(gold, tmp_path, name)
    monkeypatch.setattr(W.Worker, "_prepare_graphsaint", lambda self: None)      # the state load_data hands to prepare_data
    raw = W.Worker(_args(), dataset=name, mode="vanilla-clean", data_root=str(tmp_path))
    _same_csr(raw.adj_train, gold, f"{name}.adj_train_raw")
    _same_csr(raw.adj_full, gold, f"{name}.adj_full_raw")
    monkeypatch.undo()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    w = W.Worker(_args(), dataset=name, mode="vanilla-clean", data_root=str(tmp_path))
    assert w.transfer is False
    assert w.features.dtype == torch.float32 and w.features_train.dtype == torch.float32 and w.labels.dtype == torch.int64
    assert np.array_equal(w.features.numpy(), gold[f"{name}.features"])
    assert np.array_equal(w.features_train.numpy(), gold[f"{name}.features_train"])
    assert np.array_equal(w.labels.numpy(), gold[f"{name}.labels"])
    for k in ("idx_train", "idx_val", "idx_test"):
        got = getattr(w, k)
        assert isinstance(got, np.ndarray) and got.dtype == gold[f"{name}.{k}"].dtype and np.array_equal(got, gold[f"{name}.{k}"])
    assert [w.n_nodes, w.n_features, w.n_classes, w.multi_label] == gold[f"{name}.sizes"].tolist()
    assert isinstance(w.n_classes, int)
    _same_csr(w.adj_ori, gold, f"{name}.adj_ori")
    for which in ("adj_train", "adj_full"):
        t = getattr(w, which).coalesce()
        assert t.dtype == torch.float32 and list(t.shape) == gold[f"{name}.clean.{which}.shape"].tolist()
        assert np.array_equal(t.indices().numpy(), gold[f"{name}.clean.{which}.indices"]), which
        assert np.array_equal(t.values().numpy(), gold[f"{name}.clean.{which}.values"]), which


def test_worker_dp_perturbs_both_graphs_and_keeps_the_clean_one(gold, tmp_path, monkeypatch):
    from linkteller_amd import dp
    from linkteller_amd.worker import Worker
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _write(gold, tmp_path, "flickr")
    calls = []
    real = dp.perturb_adj
    monkeypatch.setattr(dp, "perturb_adj", lambda adj, *a, **k: (calls.append(adj.shape), real(adj, *a, **k))[1])
    w = Worker(_args(mode="vanilla"), dataset="flickr", mode="vanilla", data_root=str(tmp_path))
    assert calls == [(60, 60), (30, 30)]                       # the full graph first, then the training subgraph (worker.py:618-619)
    _same_csr(w.adj_ori, gold, "flickr.adj_ori")               # the pairs still come from the clean graph
    assert not np.array_equal(w.adj_full.coalesce().values().numpy(), gold["flickr.clean.adj_full.values"])
    for name in ("cora", "citeseer", "pubmed", "twitch-train/ES"):
        with pytest.raises(NotImplementedError):
            Worker(_args(), dataset=name, mode="vanilla-clean", data_root=str(tmp_path))


def test_f1_from_confusion_against_sklearn():
    from sklearn.metrics import f1_score
    rng = np.random.RandomState(11)
    n, c = 400, 7
    y = rng.choice([0, 1, 2, 4, 6], n)                # classes 3 and 5 are never true
    p = rng.choice([0, 1, 2, 4, 5, 6], n)             # 3 is never predicted either; 5 is predicted but never true
    conf = np.zeros((c, c), dtype=np.int32)
    np.add.at(conf, (y, p), 1)
    got = engine.f1_from_confusion(conf)
    want = tuple(f1_score(y, p, average=k) for k in ("micro", "macro", "weighted"))
    assert all(isinstance(v, float) for v in got)
    for g, w_ in zip(got, want):
        assert abs(g - w_) <= 1e-12, (got, want)
    assert engine.f1_from_confusion(torch.from_numpy(conf)) == got
    # zero division gives 0: nothing right at all, and an empty table
    assert engine.f1_from_confusion(np.array([[0, 3], [2, 0]])) == (0.0, 0.0, 0.0)
    assert engine.f1_from_confusion(np.zeros((3, 3), dtype=np.int64)) == (0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        engine.f1_from_confusion(np.zeros((2, 3)))


def _no_gpu(monkeypatch):
    """Any use of the library or of a CUDA tensor fails the test: the refusals come first."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was loaded before the refusal"))


_TRAIN = ["--train", "--hidden", "8", "--norm", "FirstOrderGCN", "--num-epochs", "2"]


def test_train_refusals_by_flags(tmp_path, monkeypatch):
    from linkteller_amd import worker as W
    _no_gpu(monkeypatch)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(W, "Worker", lambda *a, **k: pytest.fail("a Worker was built before the refusal"))
    for name in ("ppi", "ppi-large", "reddit"):
        with pytest.raises(NotImplementedError, match="single label and at most 8"):
            lt_main.main(_TRAIN + ["--dataset", name, "--data-root", str(tmp_path)])
    with pytest.raises(NotImplementedError, match="--fastmode"):
        lt_main.main(_TRAIN + ["--dataset", "flickr", "--fastmode", "--data-root", str(tmp_path)])
    with pytest.raises(ValueError, match="--patience"):
        lt_main.main(_TRAIN + ["--dataset", "flickr", "--early", "--patience", "0", "--data-root", str(tmp_path)])
    assert not os.listdir(tmp_path)                                      # neither log nor model directory
    lt_main.check_split_dataset(lt_main.get_arguments(["--dataset", "ppi", "--test"]))           # testing a saved model is served
    lt_main.check_split_dataset(lt_main.get_arguments(["--dataset", "twitch/ES/RU", "--train", "--fastmode"]))   # not this family


def test_train_refusals_by_data(gold, tmp_path, monkeypatch):
    """What only the files decide is refused in ``init_model``, before a GPU trainer exists: multi-label data and a ninth class
    under the name ``flickr``; ``--fastmode`` for a caller that builds ``GCNTrainer`` itself."""
    from linkteller_amd.trainer import GCNTrainer
    from linkteller_amd.worker import Worker
    _no_gpu(monkeypatch)
    monkeypatch.chdir(tmp_path)
    _write(gold, tmp_path / "multi", "ppi", as_name="flickr")
    with pytest.raises(NotImplementedError, match="multi_label = 5"):
        lt_main.main(_TRAIN + ["--dataset", "flickr", "--data-root", str(tmp_path / "multi")])
    nine = gold["in.labels.flickr"].copy()
    nine[0] = 8
    roles = {k: gold[f"in.role.{k}"].tolist() for k in ("tr", "va", "te")}
    synth.write_graphsaint_dataset(str(tmp_path / "nine"), "flickr", _csr(gold, "in.adj"), gold["in.feats"], nine, roles)
    with pytest.raises(NotImplementedError, match="n_classes = 9"):
        lt_main.main(_TRAIN + ["--dataset", "flickr", "--data-root", str(tmp_path / "nine")])
    _write(gold, tmp_path / "ok", "flickr")
    args = lt_main.get_arguments(_TRAIN + ["--dataset", "flickr", "--fastmode"])
    w = Worker(args, dataset="flickr", mode="vanilla-clean", data_root=str(tmp_path / "ok"))
    with pytest.raises(NotImplementedError, match="--fastmode"):
        GCNTrainer(args, worker=w).init_model()


def test_early_help_names_the_family():
    text = " ".join(lt_main.build_parser().format_help().split())
    assert "flickr" in text and "saves the last model" in text


def test_new_symbols_are_declared_and_exported():
    with open(os.path.join(REPO, "include", "linkteller_hip.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^(int|size_t) " + name + r"\(", header, flags=re.M), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"^#define LT_ABI_VERSION 5\b", header, flags=re.M) and "lt_eval_head_rows" in header.split("typedef enum lt_status")[0]
    import ctypes
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name

"""``Worker`` for the datasets the hot path is evaluated on: the twitch transfer
setting ``twitch/<TRAIN>/<TEST>`` of reference worker.py:470-496, 549-552, 589-678, and the GraphSAINT family
(``flickr``, ``reddit``, ``ppi``, ``ppi-large``: one graph with a train / validation / test split of its nodes,
worker.py:425-441, 532-541, 615-629).

Reads the MUSAE files the reference reads (``./data/twitch/<CC>/musae_<CC>_{features.json,
target.csv,edges.csv}``, utils/load.py:42-93, 452-460), standardises the one-hot features with
statistics of graph 1, optionally perturbs both graphs (edge DP), normalises, and exposes the
attributes ``Attacker`` / ``GCNTrainer`` use: ``features_1/2``, ``adj_1/2`` (normalised, torch sparse
COO like the reference), ``adj_ori`` (clean scipy CSR of graph 2), ``labels_1/2``, sizes.  The GraphSAINT family reads ``role.json``,
``feats.npy``, ``class_map.json`` and ``adj_full.npz`` and exposes ``features`` / ``features_train``, ``labels``,
``idx_train/val/test``, ``adj_full`` / ``adj_train`` (normalised sparse tensors) and the clean ``adj_ori``.
The other dataset families of the reference (the pickled planetoid graphs, ``twitch-train``) are refused.
"""
from __future__ import annotations

import json
import os

import numpy as np
import scipy.sparse as sp
import torch

from . import dp
from .graph import fetch_normalization, sparse_mx_to_torch_sparse_tensor

TWITCH_N_FEATURES = 3170   # reference utils/load.py:56


def read_musae_features(folder: str, code: str, n_features: int = TWITCH_N_FEATURES):
    """musae_<code>_features.json -> dense 0/1 [n, n_features]; musae_<code>_target.csv -> labels
    ('mature' looked up by 'new_id'), reference utils/load.py:47-69."""
    import pandas as pd
    with open(os.path.join(folder, f"musae_{code}_features.json")) as fh:
        data = json.load(fh)
    n = len(data)
    feats = np.zeros((n, n_features))
    for node, items in data.items():
        feats[int(node), items] = 1
    tgt = pd.read_csv(os.path.join(folder, f"musae_{code}_target.csv"))
    by_id = dict(zip(map(int, tgt["new_id"].values), map(int, tgt["mature"].values)))
    labels = torch.LongTensor([by_id[i] for i in range(n)])
    return feats, labels


def read_musae_edges(folder: str, code: str, n_nodes: int):
    """musae_<code>_edges.csv -> A + A^T as float32 CSR (reference utils/load.py:452-460)."""
    import pandas as pd
    edges = pd.read_csv(os.path.join(folder, f"musae_{code}_edges.csv")).values
    a = sp.csr_matrix((np.ones(edges.shape[0]), (edges[:, 0], edges[:, 1])), shape=(n_nodes, n_nodes),
                      dtype=np.float32)
    return a + a.T


GRAPHSAINT = ("reddit", "flickr", "ppi", "ppi-large")      # reference utils/load.py:115


def is_transfer(dataset: str) -> bool:
    """The reference's transfer rule (gcn_trainer.py:54-56, mlp_trainer.py:39-41): two graphs, train on one, test on the other."""
    return (dataset.startswith("twitch") and not dataset.startswith("twitch-train")) \
        or dataset.startswith("wikipedia") or dataset.startswith("deezer")


def is_served(dataset: str) -> bool:
    """The datasets this package reads: ``twitch/<A>/<B>`` and the GraphSAINT family."""
    return dataset in GRAPHSAINT or (dataset.startswith("twitch") and not dataset.startswith("twitch-train")
                                     and len(dataset.split("/")) == 3)


def read_graphsaint(folder: str, with_adj: bool = True):
    """``role.json`` / ``feats.npy`` / ``class_map.json`` / ``adj_full.npz`` of a GraphSAINT dataset -> (features, features_train,
    labels, idx_train, idx_val, idx_test, adj_full) as reference utils/load.py:115-148, 209-216, 485-488 forms them: sorted
    index arrays, features standardised in float64 with the training rows' statistics and then narrowed to float32, labels a
    LongTensor [n, multi_label] (``multi_label`` = the length of the first value of the class map, 1 for a plain int).
    ``with_adj=False`` leaves ``adj_full.npz`` unread and returns None in its place (the feature-only baselines)."""
    from sklearn.preprocessing import StandardScaler
    with open(os.path.join(folder, "role.json")) as fh:
        role = json.load(fh)
    idx_train, idx_val, idx_test = (np.asarray(sorted(role[k])) for k in ("tr", "va", "te"))
    features = np.load(os.path.join(folder, "feats.npy"))
    scaler = StandardScaler().fit(features[idx_train])
    features = torch.FloatTensor(scaler.transform(features))
    features_train = features[idx_train]
    n_nodes = len(features)
    with open(os.path.join(folder, "class_map.json")) as fh:
        class_map = json.load(fh)
    multi_label = 1
    for value in class_map.values():
        if type(value) == list:
            multi_label = len(value)
        break
    labels = np.zeros((n_nodes, multi_label))
    for key, value in class_map.items():
        labels[int(key)] = value
    labels = torch.LongTensor(labels)
    if not with_adj:
        return features, features_train, labels, idx_train, idx_val, idx_test, None
    adj = np.load(os.path.join(folder, "adj_full.npz"))
    n, m = adj["shape"]
    adj_full = sp.csr_matrix((adj["data"], adj["indices"], adj["indptr"]), (n, m))
    return features, features_train, labels, idx_train, idx_val, idx_test, adj_full


class Worker:
    def __init__(self, args, dataset="", mode="", data_root="./data"):
        self.args = args
        self.dataset = dataset
        self.mode = mode
        self.data_root = data_root
        self.transfer = is_transfer(dataset)
        self.load_data()

    def load_data(self):
        if self.dataset in GRAPHSAINT:
            self._load_graphsaint()
            return
        if not (self.dataset.startswith("twitch") and not self.dataset.startswith("twitch-train")):
            raise NotImplementedError(f"dataset = {self.dataset} not implemented! (served: twitch/<A>/<B>, "
                                      f"{' / '.join(GRAPHSAINT)})")
        family, code_1, code_2 = self.dataset.split("/")        # twitch/ES/RU
        self.dataset1, self.dataset2 = f"{family}/{code_1}", f"{family}/{code_2}"
        f1, self.labels_1 = read_musae_features(os.path.join(self.data_root, family, code_1), code_1)
        f2, self.labels_2 = read_musae_features(os.path.join(self.data_root, family, code_2), code_2)
        from sklearn.preprocessing import StandardScaler
        scaler = StandardScaler().fit(f1)                         # worker.py:486-490
        self.features_1 = torch.FloatTensor(scaler.transform(f1))
        self.features_2 = torch.FloatTensor(scaler.transform(f2))
        self.n_nodes_1, self.n_nodes_2 = len(self.labels_1), len(self.labels_2)
        self.n_nodes = self.n_nodes_2
        self.n_features, self.multi_label, self.n_classes = TWITCH_N_FEATURES, 1, 2
        self.adj_1 = read_musae_edges(os.path.join(self.data_root, family, code_1), code_1, self.n_nodes_1)
        self.adj_2 = read_musae_edges(os.path.join(self.data_root, family, code_2), code_2, self.n_nodes_2)
        self.adj_ori = sp.csr_matrix.copy(self.adj_2)             # clean ground truth, worker.py:552
        self.prepare_data()

    def _load_graphsaint(self):
        """worker.py:425-441, 532-541: one graph, the model trains on the subgraph induced by ``idx_train``."""
        (self.features, self.features_train, self.labels, self.idx_train, self.idx_val, self.idx_test,
         self.adj_full) = read_graphsaint(os.path.join(self.data_root, self.dataset))
        print(f"loading {self.dataset} graph done!")
        self.n_nodes = len(self.labels)
        self.n_features = self.features.shape[1]
        self.multi_label = self.labels.shape[1]
        self.n_classes = self.labels.max().item() + 1 if self.multi_label == 1 else self.multi_label
        self.adj_train = self.adj_full[self.idx_train, :][:, self.idx_train]
        self.adj_ori = sp.csr_matrix.copy(self.adj_full)          # clean ground truth, worker.py:541
        self._prepare_graphsaint()

    def _prepare_graphsaint(self):
        """worker.py:615-629, 665-670: under edge DP both graphs are perturbed, each by its own draw (the full graph first)."""
        a = self.args
        if self.mode not in ("vanilla", "vanilla-clean"):
            raise NotImplementedError("mode = {} not implemented!".format(self.mode))
        if self.mode == "vanilla" and getattr(a, "dp_build", "host") == "device":
            from .graph import normalize_device, torch_sparse_from_device_csr
            if getattr(a, "noise_rng", "numpy") != "philox":
                raise NotImplementedError("dp_build = device needs noise_rng = philox (the numpy stream is drawn on the host)")
            pattern_full = dp.perturb_adj_device(self.adj_full, a.perturb_type, a.epsilon, a.noise_seed, a.noise_type, a.delta)
            pattern_train = dp.perturb_adj_device(self.adj_train, a.perturb_type, a.epsilon, a.noise_seed, a.noise_type, a.delta)
            print("perturbing done!")
            self.adj_train = torch_sparse_from_device_csr(*normalize_device(a.norm, *pattern_train))
            self.adj_full = torch_sparse_from_device_csr(*normalize_device(a.norm, *pattern_full))
            print("Normalizing Adj done!")
            self.features, self.features_train = self.features.cuda(), self.features_train.cuda()
            self.labels = self.labels.cuda()
            return
        if self.mode == "vanilla":
            noise_rng = getattr(a, "noise_rng", "numpy")
            self.adj_full = dp.perturb_adj(self.adj_full, a.perturb_type, a.epsilon, a.noise_seed, a.noise_type, a.delta, rng=noise_rng)
            self.adj_train = dp.perturb_adj(self.adj_train, a.perturb_type, a.epsilon, a.noise_seed, a.noise_type, a.delta, rng=noise_rng)
            print("perturbing done!")
        normalizer = fetch_normalization(a.norm)
        self.adj_train = sparse_mx_to_torch_sparse_tensor(normalizer(self.adj_train))
        self.adj_full = sparse_mx_to_torch_sparse_tensor(normalizer(self.adj_full))
        print("Normalizing Adj done!")
        if torch.cuda.is_available():
            self.features, self.features_train = self.features.cuda(), self.features_train.cuda()
            self.labels = self.labels.cuda()
            self.adj_train, self.adj_full = self.adj_train.cuda(), self.adj_full.cuda()

    def prepare_data(self):
        a = self.args
        if self.mode == "vanilla" and getattr(a, "dp_build", "host") == "device":   # --dp-build, an addition: the DP graphs never
            self._prepare_dp_on_device()                                            # leave the device
            return
        if self.mode == "vanilla":                                # serve the model on DP graphs, worker.py:632-635
            noise_rng = getattr(a, "noise_rng", "numpy")          # --noise-rng, an addition: callers' Namespaces may lack it
            self.adj_1 = dp.perturb_adj(self.adj_1, a.perturb_type, a.epsilon, a.noise_seed, a.noise_type, a.delta, rng=noise_rng)
            self.adj_2 = dp.perturb_adj(self.adj_2, a.perturb_type, a.epsilon, a.noise_seed, a.noise_type, a.delta, rng=noise_rng)
            print("perturbing done!")
        elif self.mode != "vanilla-clean":
            raise NotImplementedError("mode = {} not implemented!".format(self.mode))
        normalizer = fetch_normalization(a.norm)
        self.adj_1 = sparse_mx_to_torch_sparse_tensor(normalizer(self.adj_1))
        self.adj_2 = sparse_mx_to_torch_sparse_tensor(normalizer(self.adj_2))
        print("Normalizing Adj done!")
        if torch.cuda.is_available():                             # worker.py:665-678
            self.features_1, self.features_2 = self.features_1.cuda(), self.features_2.cuda()
            self.labels_1, self.labels_2 = self.labels_1.cuda(), self.labels_2.cuda()
            self.adj_1, self.adj_2 = self.adj_1.cuda(), self.adj_2.cuda()

    def _prepare_dp_on_device(self):
        """``--dp-build device`` (with ``--noise-rng philox``): scipy -> perturbed CSR -> normalised CSR -> sparse tensor, all on the
        GPU; ``adj_1`` / ``adj_2`` hold what the host route's ``.cuda()`` tensors hold, without its explicit zeros."""
        from .graph import normalize_device, torch_sparse_from_device_csr
        a = self.args
        if getattr(a, "noise_rng", "numpy") != "philox":
            raise NotImplementedError("dp_build = device needs noise_rng = philox (the numpy stream is drawn on the host)")
        pattern_1 = dp.perturb_adj_device(self.adj_1, a.perturb_type, a.epsilon, a.noise_seed, a.noise_type, a.delta)
        pattern_2 = dp.perturb_adj_device(self.adj_2, a.perturb_type, a.epsilon, a.noise_seed, a.noise_type, a.delta)
        print("perturbing done!")
        self.adj_1 = torch_sparse_from_device_csr(*normalize_device(a.norm, *pattern_1))
        self.adj_2 = torch_sparse_from_device_csr(*normalize_device(a.norm, *pattern_2))
        print("Normalizing Adj done!")
        self.features_1, self.features_2 = self.features_1.cuda(), self.features_2.cuda()
        self.labels_1, self.labels_2 = self.labels_1.cuda(), self.labels_2.cuda()


class FeatureData:
    """The graph-free view of a dataset for the feature-only baselines (``main_simple``): what ``Worker`` exposes of it,
    without reading, perturbing or normalising an adjacency (no edge file is opened for either dataset family).  Transfer datasets (``twitch/<A>/<B>``):
    ``features_1 / labels_1`` (training graph's nodes), ``features_2 / labels_2``.  The GraphSAINT family: ``features``,
    ``labels`` [n, multi_label], ``idx_train / idx_val / idx_test``."""

    def __init__(self, dataset, mode="mlp", data_root="./data"):
        self.dataset, self.mode, self.data_root = dataset, mode, data_root
        self.transfer = is_transfer(dataset)
        dev = "cuda" if torch.cuda.is_available() else "cpu"
        if dataset in GRAPHSAINT:
            (features, _, labels, self.idx_train, self.idx_val, self.idx_test, _) = \
                read_graphsaint(os.path.join(data_root, dataset), with_adj=False)
            self.features, self.labels = features.to(dev), labels.to(dev)
            self.n_nodes, self.n_features = len(labels), features.shape[1]
            self.multi_label = labels.shape[1]
            self.n_classes = labels.max().item() + 1 if self.multi_label == 1 else self.multi_label
            return
        if not (dataset.startswith("twitch") and not dataset.startswith("twitch-train")):
            raise NotImplementedError(f"dataset = {dataset} not implemented! (served: twitch/<A>/<B>, {' / '.join(GRAPHSAINT)})")
        family, code_1, code_2 = dataset.split("/")
        f1, labels_1 = read_musae_features(os.path.join(data_root, family, code_1), code_1)
        f2, labels_2 = read_musae_features(os.path.join(data_root, family, code_2), code_2)
        from sklearn.preprocessing import StandardScaler
        scaler = StandardScaler().fit(f1)                         # worker.py:486-490
        self.features_1 = torch.FloatTensor(scaler.transform(f1)).to(dev)
        self.features_2 = torch.FloatTensor(scaler.transform(f2)).to(dev)
        self.labels_1, self.labels_2 = labels_1.to(dev), labels_2.to(dev)
        self.n_nodes_1, self.n_nodes_2 = len(labels_1), len(labels_2)
        self.n_nodes = self.n_nodes_2
        self.n_features, self.multi_label, self.n_classes = TWITCH_N_FEATURES, 1, 2

"""``MLPTrainer`` (reference mlp_trainer.py): the feature-only baselines -- ``OneLayerMLP`` (``--depth 1``) and
``SingleHiddenLayerMLP`` (``--depth 2``) -- trained on the GPU by ``engine.MLPTrainer`` (Adam on shuffled minibatches of
``--batch-size`` rows; forward, loss, backward and Adam as HIP kernels, a whole run enqueued by one library call) and tested
through ``engine.mlp_forward``.

It offers the reference's ``init_model`` / ``train`` / ``test`` / ``eval_output``.  Transfer datasets train on
``features_1 / labels_1`` and test on ``features_2`` with ``rare_class_f1``; datasets with a split train on
``features[idx_train]`` and print validation and test lines over ``idx_val`` / ``idx_test`` with micro / macro / weighted F1
from the device heads (``engine.eval_head_wide``, ``engine.f1_from_counts``).  As the reference, a run logs ``[epoch k]`` per
epoch and prints the total time.

Differences from the reference, all documented: each epoch's permutation is drawn as ``DataLoader(shuffle=True)`` draws it
under ``--seed`` (``order="torch"``), so a seed gives the reference's batch composition, while dropout draws a Philox4x32-10
mask keyed by ``--seed`` and the step (include/linkteller_hip.h), not torch's generator; no TensorBoard logs are written and no
per-epoch validation pass runs (the reference only feeds it to TensorBoard).  ``--early`` is accepted and, as in the reference
-- whose ``MLPTrainer`` builds an ``EarlyStopping`` and never calls it -- stops nothing."""
from __future__ import annotations

import logging
import os
import time

import torch
import torch.nn.functional as F

from .gcn import OneLayerMLP, SingleHiddenLayerMLP


class MLPTrainer:
    def __init__(self, args, subdir="", worker=None, train=True):
        self.args = args
        self.worker = worker
        self.mode = worker.mode
        self.dataset = worker.dataset
        self.subdir = subdir
        self.is_train = train
        self.transfer = worker.transfer
        self.loss_kind = "ce" if worker.multi_label == 1 else "bce"
        self.gpu_trainer = None
        if subdir:                                             # mlp_trainer.py:68-72 (without the SummaryWriter)
            self.model_path = os.path.join("model_{}".format(self.dataset), subdir)
            os.makedirs(self.model_path, exist_ok=True)

    def _train_rows(self):
        """(features, labels) the model trains on: mlp_trainer.py:53-65."""
        w = self.worker
        if self.transfer:
            return w.features_1, w.labels_1
        idx = torch.as_tensor(w.idx_train, device=w.labels.device)
        labels = w.labels[idx]
        return w.features[idx].contiguous(), labels.squeeze(1) if w.multi_label == 1 else labels

    def init_model(self, model_path=""):
        a, w = self.args, self.worker
        if self.mode != "mlp":
            raise NotImplementedError("mode = {} no corrsponding model!".format(self.mode))
        if a.depth == 1:                                       # mlp_trainer.py:77-85
            self.model = OneLayerMLP(nfeat=w.n_features, nclass=w.n_classes)
        elif a.depth == 2:
            self.model = SingleHiddenLayerMLP(nfeat=w.n_features, nhid=a.hidden, nclass=w.n_classes, dropout=a.dropout)
        else:
            raise NotImplementedError(f"depth = {a.depth} not implemented!")
        if model_path:
            self.model.load_state_dict(torch.load(model_path, map_location="cpu"))
            print("load model from {} done!".format(model_path))
        if torch.cuda.is_available():
            self.model.cuda()
        if not model_path:
            # the optimizer of mlp_trainer.py:91-92: Adam's moments live in the GPU trainer; it updates these [in, out] copies
            # in place and train() writes them back into the nn.Linear layers
            from .engine import MLPTrainer as GpuMLPTrainer
            x, labels = self._train_rows()
            n = x.shape[0]
            if not a.batch and not self.transfer:
                raise NotImplementedError("the full-batch branch (no --batch) runs on transfer datasets only, as in the reference")
            self._params = self.model.project_params()
            self.gpu_trainer = GpuMLPTrainer(x, labels, *self._params, depth=a.depth, batch_size=a.batch_size if a.batch else n,
                                             lr=a.lr, weight_decay=a.weight_decay, dropout=a.dropout, seed=a.seed,
                                             loss=self.loss_kind)

    ORDER_ENTRIES = 1 << 22      # row ids of the epoch orders held at once (host int64 + device int32: 48 MB)

    def train(self):
        """mlp_trainer.py:144-159: ``num_epochs`` epochs, ``[epoch k]`` per epoch in the log, ``model.pt`` under
        ``model_<dataset>/<subdir>``, the total time.  The epochs run in chunks of as many epochs as ``ORDER_ENTRIES`` row ids
        of their orders allow (at least one): a chunk's orders are drawn, uploaded and enqueued by one library call, its
        record is read back, and its epochs' log lines are written then.  ``run(a); run(b)`` is ``run(a + b)`` bit for bit and
        the orders are drawn in epoch order, so the chunking changes nothing but the memory held.  ``self.record`` keeps
        (loss, count) per optimiser step."""
        if self.gpu_trainer is None:
            raise RuntimeError("init_model() without a model path first")
        a = self.args
        t_total = time.time()
        n_epochs = int(a.num_epochs)
        n = self.gpu_trainer.n
        per_chunk = max(1, self.ORDER_ENTRIES // n)
        losses, counts = [], []
        for first in range(0, n_epochs, per_chunk):
            k = min(per_chunk, n_epochs - first)
            order = "torch" if a.batch else torch.arange(n, dtype=torch.int32).repeat(k, 1)
            loss, count = self.gpu_trainer.run(k, order=order)
            losses.append(loss)
            counts.append(count)
            for epoch in range(first, first + k):
                logging.info("[epoch {}]".format(epoch))
        import numpy as np
        self.record = (np.concatenate(losses) if losses else np.zeros(0, dtype=np.float32),
                       np.concatenate(counts) if counts else np.zeros(0, dtype=np.int64))
        self.model.load_project_params(self._params)
        self.model.eval()
        torch.save(self.model.state_dict(), os.path.join(self.model_path, "model.pt"))
        print("Total time elapsed: {:.4f}s".format(time.time() - t_total))

    def rare_class_f1(self, output, labels):
        """mlp_trainer.py:181-202: F1 / precision / recall / AP of the minority class (``metrics.rare_class_f1``).  Where no row
        is predicted as the rare class the reference returns a bare 0 and then fails to index it; here the line prints zeros
        and the AP."""
        from .metrics import rare_class_f1
        return rare_class_f1(output, labels, bare_zero=False)

    def _score_rows(self, rows):
        """(loss, (micro, macro, weighted) F1, logits) over the listed rows of a split dataset, on the device."""
        from .engine import eval_head_wide, f1_from_counts
        w = self.worker
        out = self.model(w.features, rows=torch.as_tensor(rows, dtype=torch.int32, device=w.features.device))
        idx = torch.as_tensor(rows, device=w.labels.device)
        labels = w.labels[idx]
        loss, counts = eval_head_wide(out, labels.squeeze(1) if w.multi_label == 1 else labels, loss=self.loss_kind)
        return float(loss), f1_from_counts(counts, present_only=self.loss_kind == "ce"), out

    def eval_output(self):
        """mlp_trainer.py:205-230: the validation line (split datasets) and the test line."""
        w = self.worker
        if not self.transfer:
            loss_val, acc_val, _ = self._score_rows(w.idx_val)
            output_info = f"Valid set results: loss = {loss_val:.4f} f1_score = {acc_val[0]:.4f} "
            print(output_info)
            logging.info(output_info)
            loss_test, acc_test, self.test_output = self._score_rows(w.idx_test)
            output_info = f"Test set results: loss = {loss_test:.4f} " \
                          f"f1_score [micro, macro, weighted] = {acc_test[0]:.4f} {acc_test[1]:.4f} {acc_test[2]:.4f}"
        else:
            self.test_output = output = self.model(w.features_2)
            loss_test = F.cross_entropy(output, w.labels_2.squeeze()).item()
            acc_test = self.rare_class_f1(output, w.labels_2)
            output_info = f"Test set results: loss = {loss_test:.4f} " \
                          f"rare_class_f1 = {acc_test[0]:.4f} prec = {acc_test[1]:.4f} reca = {acc_test[2]:.4f} " \
                          f"ap_score = {acc_test[3]:.4f}"
        print(output_info)
        logging.info(output_info)
        self.test_results = {"loss_test": loss_test, "f1_test": acc_test}

    def test(self, eval_degree=False):
        self.model.eval()
        self.eval_output()

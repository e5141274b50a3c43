"""``GCNTrainer`` (reference gcn_trainer.py:23-110, 113-243, 262-284, 320-406): build the model, either load a
``state_dict`` or train the model on the GPU (``engine.GCN2Trainer`` / ``engine.GCN3Trainer``: forward, cross-entropy,
backward and Adam as HIP kernels), one clean forward for the utility metrics, dispatch to ``Attacker``.

Training differs from the reference in two documented ways: dropout draws a Philox4x32-10 mask keyed by ``--seed`` and the
epoch (include/linkteller_hip.h), not torch's generator; and no TensorBoard logs are written (``tensorboard`` is not a
dependency of this package) -- the per-epoch lines go to the log file as the reference writes them."""
from __future__ import annotations

import logging
import os
import time

import torch
import torch.nn.functional as F

from .attacker import Attacker, DEVICE_BASELINE_SCORES, STREAM_BASELINE_SCORES
from .gcn import GCN, GCN3


class GCNTrainer:
    def __init__(self, args, subdir="", worker=None):
        self.args = args
        self.worker = worker
        self.mode = worker.mode
        self.dataset = worker.dataset
        self.subdir = subdir
        self.gpu_trainer = None
        if subdir:                                             # gcn_trainer.py:37-52 (without the SummaryWriter)
            self.model_path = os.path.join("model_{}".format(self.dataset), subdir)
            os.makedirs(self.model_path, exist_ok=True)

    def init_model(self, model_path=""):
        a, w = self.args, self.worker
        if self.mode not in ("vanilla-clean", "vanilla"):
            raise NotImplementedError("mode = {} no corrsponding model!".format(self.mode))
        if a.n_layer == 2:
            self.model = GCN(nfeat=w.n_features, nhid=a.hidden, nclass=w.n_classes, dropout=a.dropout)
        elif a.n_layer == 3:
            self.model = GCN3(nfeat=w.n_features, nhid1=a.hidden1, nhid2=a.hidden2, nclass=w.n_classes,
                              dropout=a.dropout)
        else:
            raise NotImplementedError(f"n_layer = {a.n_layer} not implemented!")
        if model_path:
            self.model.load_state_dict(torch.load(model_path, map_location="cpu"))
            print("load model from {} done!".format(model_path))
            self.model_path = model_path
        if torch.cuda.is_available():
            self.model.cuda()
        if not model_path:
            # the optimizer state of gcn_trainer.py:106-108: Adam's moments live in the GPU trainer, which updates the
            # model's parameters in place
            from .engine import GCN2Trainer, GCN3Trainer
            wide = getattr(a, "train_head", "narrow") == "wide"      # either model: GCN3Trainer takes the wide head too
            if w.transfer:
                train_on = (w.adj_1, w.features_1, w.labels_1)
            else:                                              # gcn_trainer.py:131, 154: the induced training subgraph
                if getattr(a, "fastmode", False):
                    raise NotImplementedError(f"dataset = {self.dataset}: --fastmode is refused (the reference then indexes the "
                                              "training subgraph's logits with ids of the full graph)")
                if wide and w.n_classes > 256:
                    raise NotImplementedError(f"dataset = {self.dataset}: the wide head trains at most 256 classes (got "
                                              f"n_classes = {w.n_classes})")
                if not wide and (w.multi_label > 1 or w.n_classes > 8):
                    raise NotImplementedError(
                        f"dataset = {self.dataset}: training is implemented for a single label and at most 8 classes (got "
                        f"multi_label = {w.multi_label}, n_classes = {w.n_classes}); load a trained model with --test --model-path")
                train_on = (w.adj_train, w.features_train, w.labels[torch.as_tensor(w.idx_train, device=w.labels.device)])
            rows = {}
            if getattr(a, "train_setting", "inductive") == "transductive":      # addition: --train-setting
                if w.transfer:
                    raise NotImplementedError(f"dataset = {self.dataset}: train_setting = transductive needs one graph with a "
                                              "split of its nodes (a transfer dataset has nothing to list)")
                # gcn_trainer.py:150-156 where adj_train is the full graph: forward everything, the loss over idx_train
                train_on, rows = (w.adj_full, w.features, w.labels), dict(train_rows=w.idx_train)
            layers = [self.model.gc1, self.model.gc2] + ([self.model.gc3] if a.n_layer == 3 else [])
            params = [t.detach() for g in layers for t in (g.weight, g.bias)]
            head = dict(head="wide", loss="bce" if getattr(w, "multi_label", 1) > 1 else "ce") if wide else {}
            self.gpu_trainer = (GCN3Trainer if a.n_layer == 3 else GCN2Trainer)(
                *train_on, *params, lr=a.lr, weight_decay=a.weight_decay, dropout=a.dropout, seed=a.seed, **head, **rows)

    def train(self):
        """gcn_trainer.py:200-243 on a transfer dataset: ``num_epochs`` epochs on (features_1, adj_1, labels_1), the
        per-epoch log line of train_one_epoch, ``model.pt`` under ``model_<dataset>/<subdir>``.  The epochs run back to back
        on the device and the per-epoch record is read once at the end, so the ``time`` of an epoch's line is the run's wall
        time divided by the number of epochs.  A dataset with one graph and a split of its nodes: ``_train_split``."""
        if self.gpu_trainer is None:
            raise RuntimeError("init_model() without a model path first")
        a = self.args
        t_total = time.time()
        self.model.train()
        n_epochs = int(a.num_epochs)
        validate = getattr(a, "validate", "off")
        if not self.worker.transfer:
            self._train_split(n_epochs, validate, t_total)
        elif validate != "off":
            self._train_validated(n_epochs, validate, t_total)
        else:
            loss, correct = self.gpu_trainer.run(n_epochs)
            per_epoch = (time.time() - t_total) / max(n_epochs, 1)
            n = self.gpu_trainer.n
            for epoch in range(n_epochs):
                logging.info("[epoch {}]".format(epoch))
                output_info = "Epoch: {:04d}".format(epoch + 1), \
                    "loss_train: {:.4f}".format(float(loss[epoch])), \
                    "acc_train: {:.4f}".format(int(correct[epoch]) / n), \
                    "time: {:.4f}s".format(per_epoch)
                logging.info(output_info)
        self.model.eval()
        torch.save(self.model.state_dict(), os.path.join(self.model_path, "model.pt"))
        print("Optimization Finished!")
        print("Total time elapsed: {:.4f}s".format(time.time() - t_total))

    def _train_validated(self, n_epochs, validate, t_total):
        """``--validate log / best / early`` (an addition; the reference validates a transfer dataset every epoch,
        gcn_trainer.py:167-174, and selects a model only on the other datasets, :195-196, :235-238): every epoch is followed
        on the device by the forward of (features_2, adj_2), the evaluation head and the early-stopping state.  The log
        tuple gains ``loss_val`` / ``acc_val`` as the reference's non-transfer line has them (gcn_trainer.py:198-203);
        ``best`` and ``early`` restore the parameters of the best validation loss before ``model.pt`` is written."""
        w, tr = self.worker, self.gpu_trainer
        keep = validate in ("best", "early")
        tr.attach_validation(w.adj_2, w.features_2, w.labels_2, keep_best=keep,
                             patience=int(self.args.patience) if validate == "early" else 0)
        self._log_validated(tr.run_validated(n_epochs), t_total, tr.n2, restore=keep)

    def _log_validated(self, r, t_total, n_val, restore):
        """The log lines of a validated run ``r`` (``run_validated``'s dict) whose head scored ``n_val`` rows; with ``restore``
        the parameters of the best validation loss are put back."""
        tr = self.gpu_trainer
        done = len(r["loss"])
        per_epoch = (time.time() - t_total) / max(done, 1)
        # the record's second word is the sum of tp over the classes: the correct rows of a single-label trainer; of a multi-label
        # one the (node, label) pairs that are true positives, printed as their share of all n C pairs (never above 1; the
        # training rows' (fp, fn) are kept for the last epoch only, so a per-epoch F1 as acc_val's cannot be formed)
        # (--train-setting transductive: over the listed training rows, n_train of the n forwarded)
        train_terms = getattr(tr, "n_train", tr.n) * (tr.c if getattr(tr, "loss", "ce") == "bce" else 1)
        for epoch in range(done):
            logging.info("[epoch {}]".format(epoch))
            output_info = "Epoch: {:04d}".format(epoch + 1), \
                "loss_train: {:.4f}".format(float(r["loss"][epoch])), \
                "acc_train: {:.4f}".format(int(r["correct"][epoch]) / train_terms), \
                "loss_val: {:.4f}".format(float(r["val_loss"][epoch])), \
                "acc_val: {:.4f}".format(self._acc_val(r["val_counts"][epoch], n_val)), \
                "time: {:.4f}s".format(per_epoch)
            logging.info(output_info)
        if r["stop_epoch"] >= 0:      # (only a run with a patience stops)
            logging.info(f"early stop at epoch {r['stop_epoch']}")
        if done and restore:
            tr.restore_best()
            info = f"best validation loss {float(r['val_loss'][r['best_epoch']]):.4f} at epoch {r['best_epoch']}: that model is saved"
            print(info)
            logging.info(info)

    def _acc_val(self, counts, n_val):
        """An epoch's ``acc_val``: the confusion's trace over the rows scored; with the wide head the micro F1 of its (tp, fp, fn)
        counts -- for a single label the accuracy, as the reference's ``f1_score(...)[0]`` (gcn_trainer.py:246-252)."""
        if getattr(self.gpu_trainer, "head", "narrow") == "wide":
            from .engine import f1_from_counts
            return f1_from_counts(counts)[0]
        return int(counts.trace()) / n_val

    def _train_split(self, n_epochs, validate, t_total):
        """gcn_trainer.py:183-206, 229-238 on a dataset with one graph and a split of its nodes: always validated -- every epoch
        is followed on the device by the forward of (features, adj_full) and the evaluation head over ``idx_val``
        (``attach_validation(..., rows=idx_val)``).  ``--early`` has the reference's meaning here: the run stops after
        ``--patience`` epochs without improvement and saves the best model, a run that never stops saves the last one.
        ``--validate best`` / ``early`` keep the project's meaning (the best model is always restored); ``off`` is ``log``."""
        a, w, tr = self.args, self.worker, self.gpu_trainer
        early = bool(getattr(a, "early", False))
        keep = early or validate in ("best", "early")
        tr.attach_validation(w.adj_full, w.features, w.labels, rows=w.idx_val, keep_best=keep,
                             patience=int(a.patience) if (early or validate == "early") else 0)
        r = tr.run_validated(n_epochs)
        self._log_validated(r, t_total, len(w.idx_val), restore=validate in ("best", "early") or (early and r["stop_epoch"] >= 0))

    def forward(self, mode="train"):
        w = self.worker
        if not w.transfer:                                     # gcn_trainer.py:129-132
            return self.model(w.features_train, w.adj_train) if mode == "train" else self.model(w.features, w.adj_full)
        return self.model(w.features_1, w.adj_1) if mode == "train" else self.model(w.features_2, w.adj_2)

    def _eval_split(self, output, mode):
        """gcn_trainer.py:341-384 for a dataset with a split: validation loss / F1 over ``idx_val``, test loss and micro / macro /
        weighted F1 over ``idx_test``.  Single label with at most 8 classes: the evaluation head over the row list on the
        device and ``f1_from_confusion``; multi-label or wider: host torch / sklearn, as the reference does -- or, in a run with
        ``--train-head wide``, ``eval_head_wide`` and ``f1_from_counts`` on the device."""
        w = self.worker
        if getattr(self.args, "train_head", "narrow") == "wide":      # any width up to 256, either label kind, on the device
            from .engine import eval_head_wide, f1_from_counts
            kind = "bce" if w.multi_label > 1 else "ce"

            def score(rows):
                loss, counts = eval_head_wide(output, w.labels, rows=rows, loss=kind)
                return float(loss), f1_from_counts(counts, present_only=kind == "ce")
        elif w.multi_label == 1 and w.n_classes <= 8:
            from .engine import eval_head, f1_from_confusion

            def score(rows):
                loss, conf = eval_head(output, w.labels, rows=rows)
                return float(loss), f1_from_confusion(conf)
        else:
            from sklearn.metrics import f1_score

            def score(rows):
                rows = torch.as_tensor(rows, device=output.device)
                out, target = output[rows], w.labels[rows]
                if w.multi_label == 1:                        # gcn_trainer.py:60-64, 246-252
                    loss = F.cross_entropy(out, target.squeeze())
                    preds = F.softmax(out, dim=1).max(1)[1].type_as(target)
                else:
                    loss = F.binary_cross_entropy_with_logits(out, target.float())
                    preds = torch.sigmoid(out) > 0.5
                t, p = target.cpu(), preds.detach().cpu()
                return loss.item(), tuple(f1_score(t, p, average=k) for k in ("micro", "macro", "weighted"))
        loss_valid, acc_valid = score(w.idx_val)
        info = f"[{mode}] Validation set results: loss = {loss_valid:.4f} f1_score = {acc_valid[0]:.4f}"
        print(info)
        logging.info(info)
        loss_test, acc_test = score(w.idx_test)
        info = f"[{mode}] Test set results: loss = {loss_test:.4f} " \
               f"f1_score [micro, macro, weighted] = {acc_test[0]:.4f} {acc_test[1]:.4f} {acc_test[2]:.4f}"
        print(info)
        logging.info(info)
        self.split_results = {"loss_valid": loss_valid, "f1_valid": acc_valid, "loss_test": loss_test, "f1_test": acc_test}

    def rare_class_f1(self, output, labels):
        """gcn_trainer.py:262-284: F1 / precision / recall / AP of the minority class (``metrics.rare_class_f1``)."""
        from .metrics import rare_class_f1
        return rare_class_f1(output, labels)

    def _recover_whole_graph(self):
        """addition: ``--recover --recover-nodes all`` -- the attacked graph itself instead of a sample (``Attacker.recover_graph``)."""
        a = self.args
        # (baseline_scores = stream: the baseline attacks' correlation square arrives in bands of rows and is ranked the same way)
        served = ("efficient", "baseline", "baseline-feat") if getattr(a, "baseline_scores", "host") in STREAM_BASELINE_SCORES else ("efficient",)
        if not (a.attack_mode in served and str(a.sample_type).startswith("unbalanced")):
            raise NotImplementedError("recover: served after the efficient attack on an unbalanced* sample only")
        self.attacker = Attacker(args=a, model=self.model, worker=self.worker)
        print("recover-nodes = all: the sampled AUC attack is skipped, every node is perturbed and every pair ranked")
        belief = float(getattr(a, "density_belief", 0.0) or 0.0)
        t = time.time()
        self.attacker.recover_graph(beliefs=[belief] if belief > 0 else None, chunk=int(getattr(a, "recover_chunk", 0) or 0) or 1024)
        print(f"whole-graph recovery done using {time.time() - t} seconds!")
        self.attacker.save_recovered(self.attacker.recovered_all_filename())

    def eval_output(self, output, mode="clean", eval_degree=False):
        a = self.args
        if a.attack and getattr(a, "recover", False) and getattr(a, "recover_nodes", "sample") == "all":
            self._recover_whole_graph()
        elif a.attack:
            # (addition: with baseline_scores = device the baseline attacks' square lives on the device and is ranked there too)
            served = (("efficient", "baseline", "baseline-feat") if getattr(a, "baseline_scores", "host") in DEVICE_BASELINE_SCORES
                      else ("efficient",))
            if getattr(a, "recover", False) and not (a.attack_mode in served and str(a.sample_type).startswith("unbalanced")):
                raise NotImplementedError("recover: served after the efficient attack on an unbalanced* sample only")
            self.attacker = Attacker(args=a, model=self.model, worker=self.worker)
            build, rng = getattr(a, "sample_build", "host"), getattr(a, "sample_rng", "numpy")
            if build == "host" and rng == "numpy":
                self.attacker.prepare_test_data()
            else:                                                 # addition: --sample-build / --sample-rng
                self.attacker.prepare_test_data(pairs=build, rng=rng)
            t = time.time()
            if getattr(a, "metrics_only", False):                 # addition: auc / ap from the device, no result file
                self.attacker.evaluate()
            elif a.attack_mode == "efficient":                    # gcn_trainer.py:326-337
                if a.sample_type == "balanced-full":
                    self.attacker.link_prediction_attack_efficient_balanced()
                else:
                    self.attacker.link_prediction_attack_efficient()
            elif a.attack_mode in ("baseline", "baseline-feat"):
                if a.sample_type == "balanced-full":
                    self.attacker.baseline_attack_balanced()
                else:
                    self.attacker.baseline_attack()
            elif a.attack_mode == "naive":                        # gcn_trainer.py:331-332
                self.attacker.link_prediction_attack()
            else:
                raise NotImplementedError(f"attack_mode = {a.attack_mode} not implemented!")
            print(f"attacks done using {time.time() - t} seconds!")
            if getattr(a, "recover", False):                      # addition (main.check_recover: efficient + unbalanced* only)
                belief = float(getattr(a, "density_belief", 0.0) or 0.0)
                chunk = int(getattr(a, "recover_chunk", 0) or 0)  # addition: --recover-chunk, 0 = the one-shot matrix
                self.attacker.recover_edges(beliefs=[belief] if belief > 0 else None, **({"chunk": chunk} if chunk > 0 else {}))
                self.attacker.save_recovered()
        if not self.worker.transfer:
            self._eval_split(output, mode)
            return
        labels = self.worker.labels_2
        loss_test = F.cross_entropy(output, labels.squeeze())
        acc = self.rare_class_f1(output, labels)
        info = f"[{mode}] Test set results: loss = {loss_test.item():.4f} "
        if acc != 0:
            info += f"rare_class_f1 = {acc[0]:.4f} prec = {acc[1]:.4f} reca = {acc[2]:.4f} ap_score = {acc[3]:.4f}"
        print(info)
        logging.info(info)

    def test(self, eval_degree=False):
        self.model.eval()
        with torch.no_grad():
            output = self.forward(mode="test")
        self.eval_output(output, "clean", eval_degree=eval_degree)

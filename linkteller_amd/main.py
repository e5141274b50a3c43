"""Command line of the reference (main.py:17-93, README.md:24-98) for the attack path:

    python -m linkteller_amd.main --mode vanilla-clean --dataset twitch/ES/RU --hidden 256 \
        --norm FirstOrderGCN --test --model-path model.pt --attack --attack-mode efficient \
        --sample-type unbalanced --n-test 500 [--influence-mode {full,sparse,delta}]

Every flag of the reference is accepted with its default.  ``--test`` runs inference + attack on a saved ``state_dict``;
``--train`` (an addition) trains the 2-layer GCN on the GPU as the reference does without ``--test``, saves
``model_<dataset>/<subdir>/model.pt``, then tests it and attacks it with ``--attack``:

    python -m linkteller_amd.main --train --mode vanilla --eps 5 --dataset twitch/ES/RU --hidden 256 \
        --norm FirstOrderGCN --attack --sample-type unbalanced --n-test 500

Without either switch the run is refused (a default run does not start a 500-epoch job by itself).  With ``--train``,
``--validate log | best | early`` (an addition, default ``off``) validates on the held-out graph after every epoch on the GPU:
``loss_val`` / ``acc_val`` in the log, the model of the best validation loss saved, and a stop after ``--patience`` epochs
without improvement.  ``--dataset flickr`` (one graph with a train / validation / test split of its nodes; ``reddit``,
``ppi``, ``ppi-large`` with ``--train-head wide``) trains on the induced training subgraph, is validated on ``idx_val`` of the full graph
after every epoch -- ``--early`` stops it as in the reference -- and is tested on ``idx_test`` with micro / macro / weighted F1.
``--train-setting transductive`` (an addition) trains such a dataset as the reference trains the datasets whose ``adj_train``
is the whole graph: the full graph is forwarded and the loss is taken over the rows ``idx_train`` only.
"""
from __future__ import annotations

import argparse
import logging
import random

import numpy as np
import torch

_NORMS = ["AugNormAdj", "FirstOrderGCN", "BingGeNormAdj", "NormAdj", "RWalk", "AugRWalk"]
_SAMPLE_TYPES = ["balanced", "unbalanced", "unbalanced-lo", "unbalanced-hi", "bfs", "balanced-full"]
_ATTACK_MODES = ["efficient", "naive", "baseline", "baseline-feat"]

# typed options: name -> (type, default[, choices]); argparse derives the reference's dest names
_OPTIONS = {
    "seed": (int, 42), "num-epochs": (int, 500), "lr": (float, 0.01), "weight_decay": (float, 5e-4),
    "hidden": (int, 16), "hidden1": (int, 16), "hidden2": (int, 16), "dropout": (float, 0.5),
    "dataset": (str, "cora"), "model-path": (str, ""), "mode": (str, "vanilla-clean"),
    "init-method": (str, "knn"), "cluster-method": (str, "hierarchical"), "scale": (str, "small"),
    "break-method": (str, "kmeans"), "norm": (str, "AugNormAdj", _NORMS),
    "sample-type": (str, "balanced", _SAMPLE_TYPES), "epsilon": (float, 0.1), "delta": (float, 1e-5),
    "influence": (float, 0.0001), "train-ratio": (float, 0.5), "patience": (int, 10),
    "n-clusters": (int, 10), "n-test": (int, 100), "n-layer": (int, 2), "break-ratio": (float, 1),
    "feature-size": (int, -1), "k": (float, 1), "noise-seed": (int, 42), "sample-seed": (int, 42),
    "cluster-seed": (int, 42), "knn": (int, -1), "noise-type": (str, "laplace"),
    "perturb-type": (str, "discrete", ["discrete", "continuous"]),
    "attack-mode": (str, "efficient", _ATTACK_MODES), "coeff": (float, 1), "degree": (int, 2),
    # additions (never renames): how lt_influence_rows evaluates a probe.  'delta' propagates the perturbation exactly
    # (scores / AUC / AP equal the reference evaluated in fp64); 'sparse' is the reference's fp32 finite difference
    # restricted to the rows a probe can change, bit-identical to 'full' (every probe a full forward); where ./data lives
    "influence-mode": (str, "delta", ["full", "sparse", "delta"]), "data-root": (str, "./data"),
    # addition: with --recover, a single density belief k > 0 instead of the ladder r/4 .. 4r (0 = the ladder)
    "density-belief": (float, 0.0),
    # addition: where the edge-DP noise of --mode vanilla comes from.  'numpy' is the reference's stream (a --noise-seed gives
    # the reference's graph; an N x N draw on the host); 'philox' is the per-cell stream of include/linkteller_hip.h,
    # evaluated on the GPU with no N x N matrix -- a different graph for the same seed, under the same result file name
    "noise-rng": (str, "numpy", ["numpy", "philox"]),
    # addition: where the DP graphs of --mode vanilla are assembled and normalised.  'host' is scipy, as the reference; 'device'
    # keeps the cells of --noise-rng philox on the GPU from the noise seed to the served graph (symmetric CSR, normaliser and
    # sparse tensor are built there: the same graph, the same float32 values)
    "dp-build": (str, "host", ["host", "device"]),
    # addition: where the attack's node pairs are enumerated and labelled.  'host' is numpy / scipy, as the reference; 'device'
    # keeps the label triangle of an unbalanced* sample (and, with --sample-rng philox, the balanced-full pair lists) on the GPU:
    # the same pairs, the same labels (Attacker.prepare_test_data)
    "sample-build": (str, "host", ["host", "device"]),
    # addition: where the non-edges of --sample-type balanced-full come from.  'numpy' is the reference's stream (a --sample-seed
    # gives the reference's pairs; a Python loop on the host); 'philox' is stream 3 of include/linkteller_hip.h, evaluated on the
    # GPU -- different pairs for the same seed, under the same result file name
    "sample-rng": (str, "numpy", ["numpy", "philox"]),
    # addition: where the baseline attacks (--attack-mode baseline / baseline-feat) score their pairs.  'host' is the reference's
    # fp32 torch arithmetic on the CPU; 'device' forms the correlations on the GPU in fp64 (lt_corr_square / lt_corr_pairs), writes
    # the same result file, and lets --metrics-only and --recover serve the baseline attacks; 'stream' is 'device' and also admits
    # --recover-chunk / --recover-nodes all: bands of the correlation square (lt_corr_rows) instead of the one-piece square
    "baseline-scores": (str, "host", ["host", "device", "stream"]),
    # addition: with --train, validate on the held-out graph (features_2, adj_2, labels_2) after every epoch, on the GPU
    # (gcn_trainer.py:167-174).  'log': loss_val / acc_val in every epoch's log tuple; 'best': as log, and the model of the best
    # validation loss is restored and saved; 'early': as best, and the run stops after --patience epochs without improvement
    # (utils/early_stopping.py, 'early stop at epoch {e}').  'off' (default): every record, log line and bit as without it
    "validate": (str, "off", ["off", "log", "best", "early"]),
    # addition: which class layer and loss head --train runs.  'narrow' (default): the fused class layer for a single label and
    # at most 8 classes, every check and every bit as before the flag existed; 'wide': up to 256 classes with cross-entropy or,
    # for a multi-label dataset, binary cross-entropy with logits (engine.GCN2Trainer(head="wide")): reddit, ppi, ppi-large
    "train-head": (str, "narrow", ["narrow", "wide"]),
    # addition: what --train forwards on a dataset with one graph and a split of its nodes.  'inductive' (default): the
    # subgraph induced by idx_train, every check and every bit as before the flag existed; 'transductive': the full graph, with
    # the loss over the rows idx_train only (gcn_trainer.py:150-156 where adj_train is the full graph;
    # engine.GCN2Trainer(train_rows=))
    "train-setting": (str, "inductive", ["inductive", "transductive"]),
    # additions: with --recover, form the score rows K probes at a time and select through engine.TopPairsStream instead of the
    # one-shot n x n matrix (0 = one shot: the same edge list either way); and which nodes are ranked -- 'sample', the sampled
    # subgraph as before, or 'all': every node of the attacked graph (Attacker.recover_graph; the sampled AUC attack is skipped,
    # the list goes to eval_<dataset>/recover_all_<result file>)
    "recover-chunk": (int, 0), "recover-nodes": (str, "sample", ["sample", "all"]),
}
_HELP = {
    "validate": "with --train: validate on the held-out graph after every epoch on the GPU.  log: loss_val / acc_val in the log; "
                "best: also restore and save the model of the best validation loss; early: also stop after --patience epochs "
                "without improvement.  Default off.",
    "patience": "epochs without improvement before --validate early stops (default 10)",
    "train-head": "with --train: narrow (default) trains a single label with at most 8 classes; wide trains up to 256 classes, "
                  "single- or multi-label (reddit, ppi, ppi-large), with the 2-layer GCN.",
    "train-setting": "with --train on flickr (reddit / ppi / ppi-large with --train-head wide): inductive (default) trains on the "
                     "subgraph induced by idx_train; transductive forwards the full graph and takes the loss over idx_train only.",
    "early": "with --train on flickr / reddit / ppi / ppi-large (one graph with a split of its nodes): stop after --patience "
             "epochs without improvement of the validation loss over idx_val and save the best model, as the reference does; a "
             "run that never stops saves the last model.  On transfer datasets (twitch/<A>/<B>) accepted and inert, as in the "
             "reference (it never reaches EarlyStopping there): early stopping is --validate early.",
}
_SWITCHES = ["no-cuda", "fastmode", "approx", "attack", "test", "break-down", "display", "same-size",
             "eval-degree", "trainable", "early", "fnormalize",
             # addition: train (as the reference does without --test), then test, and attack with --attack
             "train",
             # addition: after the efficient attack on an unbalanced* sample, recover the edge list under a density belief
             # (Attacker.recover_edges; the reference's attack_stats_all.py) and save it next to the result file
             "recover",
             # addition: with --attack and the efficient or naive attack, print auc / ap from the device-side metrics
             # (Attacker.evaluate) instead of running the attack method: no matrix on the host, no result file
             "metrics-only"]


def build_parser():
    p = argparse.ArgumentParser(description="LinkTeller attack path on MI355X")
    for name, spec in _OPTIONS.items():
        kw = dict(type=spec[0], default=spec[1])
        if len(spec) > 2:
            kw["choices"] = spec[2]
        if name in _HELP:
            kw["help"] = _HELP[name]
        p.add_argument(f"--{name}", **kw)
    for name in _SWITCHES:
        p.add_argument(f"--{name}", action="store_true", default=False, **({"help": _HELP[name]} if name in _HELP else {}))
    p.set_defaults(assign_seed=42)
    return p


def get_arguments(argv=None):
    return build_parser().parse_args(argv)


def init_distributed():
    """One process per GPU (``torchrun --nproc-per-node N -m linkteller_amd.main ...``): pin this rank's device
    BEFORE anything touches the GPU (Worker moves its tensors with ``.cuda()``) and join the process group, so
    that ``Attacker.influence_matrix`` shards the probes (linkteller_amd/dist.py) and only rank 0 writes the
    result file.  ``LT_DIST_BACKEND`` / ``LT_DIST_DEVICE`` are test hooks (gloo, all ranks on one device), and so is
    ``LT_FORCE_COLLECTIVES=1`` (a group and every collective even at world size 1: RCCL on a one-GPU box).
    Returns True when a group was created here (the caller destroys it)."""
    import os
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    force = os.environ.get("LT_FORCE_COLLECTIVES") == "1"       # dist.force_collectives(): the N > 1 path at world size 1
    if (world <= 1 and not force) or dist.is_initialized():
        return False
    rank = int(os.environ.get("RANK", "0"))
    if "MASTER_PORT" not in os.environ:
        if world > 1:      # (a port invented per rank would differ on every rank: the rendezvous would hang until the store timeout)
            raise RuntimeError("WORLD_SIZE > 1 but MASTER_PORT is not set: launch the ranks with torchrun "
                               "(python -m torch.distributed.run --nproc-per-node N -m linkteller_amd.main ...)")
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(s.getsockname()[1])
    local = int(os.environ.get("LT_DIST_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    backend = os.environ.get("LT_DIST_BACKEND", "nccl")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    return True


def _baseline_score_routes():
    """(device routes, of them the ones that admit the chunked recovery): one definition, shared with the trainer and the Attacker."""
    from .attacker import DEVICE_BASELINE_SCORES, STREAM_BASELINE_SCORES
    return DEVICE_BASELINE_SCORES, STREAM_BASELINE_SCORES


def check_recover(args):
    """``--recover`` is served after ``--attack --attack-mode efficient`` on an ``unbalanced*`` sample only (with
    ``--baseline-scores device`` also after the baseline attacks, whose square then lives on the device); anything else is
    refused here, before a Worker is built or the GPU is touched."""
    if not getattr(args, "recover", False):
        return
    # (--baseline-scores device: the baseline attacks' square is on the device too and is ranked like the efficient attack's)
    served = (("efficient", "baseline", "baseline-feat") if getattr(args, "baseline_scores", "host") in _baseline_score_routes()[0]
              else ("efficient",))
    if not (args.attack and args.attack_mode in served and str(args.sample_type).startswith("unbalanced")):
        raise NotImplementedError("--recover needs --attack --attack-mode efficient and --sample-type unbalanced / unbalanced-lo / "
                                  f"unbalanced-hi (got attack={args.attack}, attack-mode={args.attack_mode}, "
                                  f"sample-type={args.sample_type})")
    if args.density_belief < 0:
        raise ValueError(f"--density-belief {args.density_belief}: a density belief is > 0 (0 = the ladder around the true density)")


def check_recover_stream(args):
    """``--recover-chunk K`` / ``--recover-nodes all`` shape what ``--recover`` does: without it they are refused here, before a
    Worker is built or the GPU is touched; so are a negative K and, with the baseline attacks, anything but the defaults --
    unless ``--baseline-scores stream`` asks for their correlation square in bands of rows (``device`` forms it in one piece)."""
    chunk, nodes = int(getattr(args, "recover_chunk", 0)), getattr(args, "recover_nodes", "sample")
    if chunk == 0 and nodes == "sample":
        return
    if chunk < 0:
        raise ValueError(f"--recover-chunk {chunk}: the probes per chunk, > 0 (0 = the one-shot matrix)")
    if not getattr(args, "recover", False):
        raise NotImplementedError(f"--recover-chunk {chunk} / --recover-nodes {nodes} need --recover (they shape the edge recovery)")
    if args.attack_mode in ("baseline", "baseline-feat") and getattr(args, "baseline_scores", "host") in _baseline_score_routes()[1]:
        return
    if args.attack_mode != "efficient":
        raise NotImplementedError(f"--recover-chunk / --recover-nodes all need --attack-mode efficient (got {args.attack_mode}: "
                                  "the baseline attacks' correlation square is formed in one piece unless --baseline-scores stream)")


def check_metrics_only(args):
    """``--metrics-only`` serves the attacks whose scores are formed on the device (efficient, naive); the baseline attacks'
    scores are host arithmetic and are refused here, before a Worker is built or the GPU is touched -- unless
    ``--baseline-scores device`` forms them on the device too."""
    if not getattr(args, "metrics_only", False):
        return
    if args.attack_mode in ("baseline", "baseline-feat") and getattr(args, "baseline_scores", "host") not in _baseline_score_routes()[0]:
        raise NotImplementedError(f"--metrics-only needs --attack-mode efficient or naive (got attack-mode={args.attack_mode}: "
                                  "the baseline attacks score their pairs on the host)")


def check_baseline_scores(args):
    """``--baseline-scores device`` / ``stream`` moves the baseline attacks' scores to the GPU: it is refused here, before a Worker is built or
    the GPU is touched, unless ``--attack --attack-mode baseline`` / ``baseline-feat`` asks for such scores."""
    route = getattr(args, "baseline_scores", "host")
    if route not in _baseline_score_routes()[0]:
        return
    if not (args.attack and args.attack_mode in ("baseline", "baseline-feat")):
        raise NotImplementedError(f"--baseline-scores {route} needs --attack and --attack-mode baseline / baseline-feat "
                                  f"(got attack={args.attack}, attack-mode={args.attack_mode})")


def check_dp_build(args):
    """``--dp-build device`` assembles the graphs the philox stream generates on the device: it is refused here, before a Worker
    is built or the GPU is touched, unless ``--mode vanilla --noise-rng philox`` asks for such graphs."""
    if getattr(args, "dp_build", "host") != "device":
        return
    if not (args.mode == "vanilla" and args.noise_rng == "philox"):
        raise NotImplementedError("--dp-build device needs --mode vanilla and --noise-rng philox "
                                  f"(got mode={args.mode}, noise-rng={args.noise_rng}: those graphs are built on the host)")


def check_sample_build(args):
    """``--sample-build device`` / ``--sample-rng philox`` move the attack's pair preparation to the GPU: they are refused here,
    before a Worker is built or the GPU is touched, without ``--attack``, and the philox stream without ``--sample-type
    balanced-full`` (the node draw of the unbalanced* samples stays on numpy's stream)."""
    build, rng = getattr(args, "sample_build", "host"), getattr(args, "sample_rng", "numpy")
    if build == "host" and rng == "numpy":
        return
    if not args.attack:
        raise NotImplementedError(f"--sample-build {build} / --sample-rng {rng} need --attack (they prepare the attack's node pairs)")
    if rng == "philox" and args.sample_type != "balanced-full":
        raise NotImplementedError(f"--sample-rng philox needs --sample-type balanced-full (got sample-type={args.sample_type}: "
                                  "its nodes are drawn from numpy's stream)")


def check_validate(args):
    """``--validate log / best / early`` validates the epochs of ``--train``: anything but ``off`` is refused here, before a
    Worker is built or the GPU is touched, unless the run trains (``--train`` without ``--test``); ``early`` needs a
    ``--patience`` of at least 1."""
    mode = getattr(args, "validate", "off")
    if mode == "off":
        return
    if not args.train or args.test:
        raise NotImplementedError(f"--validate {mode} needs --train without --test (it validates the epochs of a training run)")
    if mode == "early" and args.patience < 1:
        raise ValueError(f"--validate early needs --patience >= 1 (got {args.patience})")


_SPLIT_DATASETS = ("reddit", "flickr", "ppi", "ppi-large")      # worker.GRAPHSAINT (not imported: no torch before the checks)
_SPLIT_MULTI_LABEL = ("reddit", "ppi", "ppi-large")              # these need --train's follow-up: a BCE head, more than 8 classes


def check_split_dataset(args):
    """``--train`` on a dataset with one graph and a split of its nodes: what the flags alone decide is refused here, before a
    Worker is built or the GPU is touched -- ``--fastmode`` (the reference then indexes the training subgraph's logits with
    ids of the full graph), a ``--patience`` below 1 with ``--early``, and the datasets whose published form is multi-label or
    wider than 8 classes (ppi, ppi-large: 121 labels per node; reddit: 41 classes), which load, test and attack from a saved
    model.  A dataset under one of the other names is judged by its own files in ``GCNTrainer.init_model``."""
    if args.dataset not in _SPLIT_DATASETS or not args.train or args.test:
        return
    if args.fastmode:
        raise NotImplementedError(f"--fastmode is refused on --dataset {args.dataset} (the reference then indexes the training "
                                  "subgraph's logits with ids of the full graph)")
    if args.early and args.patience < 1:
        raise ValueError(f"--early needs --patience >= 1 (got {args.patience})")
    if args.dataset in _SPLIT_MULTI_LABEL and getattr(args, "train_head", "narrow") != "wide":
        raise NotImplementedError(f"--train on --dataset {args.dataset}: training is implemented for a single label and at most 8 "
                                  "classes (flickr); this dataset loads, tests and attacks from a saved model (--test --model-path)")


def check_train_head(args):
    """``--train-head wide`` selects the wide class layer of ``--train``: it is refused here, before a Worker is built or the GPU
    is touched, without a training run and with ``--n-layer 3`` (``main`` trains the 2-layer GCN only; GCN3, with either head,
    is trained through the in-process ``GCNTrainer`` sequence of README)."""
    if getattr(args, "train_head", "narrow") != "wide":
        return
    if not args.train or args.test:
        raise NotImplementedError("--train-head wide needs --train without --test (it selects the class layer of a training run)")
    if args.n_layer != 2:
        raise NotImplementedError(f"--train-head wide is implemented for the 2-layer GCN only (got --n-layer {args.n_layer})")


def check_train_setting(args):
    """``--train-setting transductive`` forwards the full graph and lists the training rows: it is refused here, before a Worker
    is built or the GPU is touched, without a training run and on a dataset that has no split to list (a transfer dataset
    trains on one whole graph and tests on another).  ``main`` keeps its ``--n-layer 3`` refusal: GCN3 takes the setting
    through the in-process ``GCNTrainer`` sequence of README."""
    setting = getattr(args, "train_setting", "inductive")
    if setting == "inductive":
        return
    if setting != "transductive":
        raise ValueError(f"--train-setting {setting}: inductive or transductive")
    if not args.train or args.test:
        raise NotImplementedError("--train-setting transductive needs --train without --test (it selects the rows a training run "
                                  "takes its loss over)")
    if args.dataset not in _SPLIT_DATASETS:
        raise NotImplementedError(f"--train-setting transductive needs a dataset with one graph and a split of its nodes "
                                  f"({' / '.join(_SPLIT_DATASETS)}; got --dataset {args.dataset}: a transfer dataset trains on every "
                                  "node of its first graph, there is nothing to list)")


def main(argv=None):
    args = get_arguments(argv)
    check_validate(args)
    check_train_head(args)
    check_train_setting(args)
    check_split_dataset(args)
    check_baseline_scores(args)
    check_recover(args)
    check_recover_stream(args)
    check_metrics_only(args)
    check_dp_build(args)
    check_sample_build(args)
    import os
    if args.train and not args.test:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise NotImplementedError("--train runs on one GPU: launch it without torchrun / WORLD_SIZE > 1")
        if args.n_layer != 2:
            raise NotImplementedError("--train: training is implemented for the 2-layer GCN only (--n-layer 2)")
    owns_group = init_distributed()
    try:
        _run(args)
    except BaseException:
        # A rank that failed must NOT enter a barrier: its peers sit in the all-gather (or in the sharding policy's
        # collectives), the barrier would be a mismatched collective and the job would hang until the RCCL timeout with
        # the real exception hidden.  Re-raise at once; the launcher (torchrun) tears the other ranks down.
        raise
    else:
        if owns_group:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()


def _run(args):
    print(str(args))
    logging.info(str(args))
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(args.seed)
    if not args.test and args.train:
        _train(args)
        return
    if not args.test:
        raise NotImplementedError("only --test (inference + attack on a saved state_dict) is implemented; "
                                  "train with the reference")
    from .trainer import GCNTrainer
    from .worker import Worker
    worker = Worker(args, dataset=args.dataset, mode=args.mode, data_root=args.data_root)
    trainer = GCNTrainer(args, worker=worker)
    trainer.init_model(model_path=args.model_path)
    trainer.test(args.eval_degree)



def init_logger(log_path, log_file, level=logging.INFO):
    """utils/logging.py with print_log=False: INFO records go to ``<log_path>/<log_file>.log`` in the reference's format.
    The handler is added to the root logger (``logging.basicConfig`` would do nothing where a handler is installed already)."""
    import os
    os.makedirs(log_path, exist_ok=True)
    handler = logging.FileHandler("{0}/{1}.log".format(log_path, log_file))
    handler.setFormatter(logging.Formatter(
        "%(asctime)s [%(process)d] [%(threadName)-12.12s] [%(levelname)-5.5s]  %(message)s"))
    root = logging.getLogger()
    root.addHandler(handler)
    root.setLevel(level)
    return handler


def _train(args):
    """main.py:114-162 for the modes with a GCN (vanilla-clean, vanilla): subdir, log file, Worker, train, test."""
    import datetime
    cur_time = datetime.datetime.now().strftime("%m-%d-%H:%M:%S.%f")
    if args.mode == "vanilla-clean":
        subdir = "mode-{}_hidden-{}_lr-{}_decay-{}_dropout-{}_norm-{}_{}".format(
            args.mode, args.hidden, args.lr, args.weight_decay, args.dropout, args.norm, cur_time)
    elif args.mode == "vanilla":
        subdir = "mode-global_perturb-{}_eps-{}_{}".format(args.perturb_type, args.epsilon, cur_time)
    else:
        raise NotImplementedError("mode = {}: --train is implemented for vanilla-clean and vanilla".format(args.mode))
    print("subdir = {}".format(subdir))
    handler = init_logger("./logs_{}".format(args.dataset), subdir)
    try:
        from .trainer import GCNTrainer
        from .worker import Worker
        worker = Worker(args, dataset=args.dataset, mode=args.mode, data_root=args.data_root)
        trainer = GCNTrainer(args, subdir=subdir, worker=worker)
        trainer.init_model()
        trainer.train()
        trainer.test(args.eval_degree)
    finally:
        logging.getLogger().removeHandler(handler)
        handler.close()


if __name__ == "__main__":
    main()

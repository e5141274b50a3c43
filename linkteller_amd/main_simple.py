"""Command line of the reference's ``main_simple.py`` for the feature-only baselines: the model that sees node features and
no edges, the "no graph at all" utility line next to a DP GCN.

    python -m linkteller_amd.main_simple --mode mlp --depth 2 --hidden 16 --batch --dataset twitch/ES/RU
    python -m linkteller_amd.main_simple --mode mlp --depth 2 --hidden 16 --dataset twitch/ES/RU --test --model-path model.pt

Every flag of the reference is accepted with its default, and the run directory carries the reference's name
(``model_<dataset>/mode-mlp_hidden-.._lr-.._decay-.._dropout-.._bs-.._<time>/model.pt``).  Served: ``--mode mlp`` with
``--depth 1`` (``OneLayerMLP``) or ``2`` (``SingleHiddenLayerMLP``), ``--batch`` with ``--batch-size``, and ``--test
--model-path``.  Refused before any file is read or written: a dataset that is neither ``twitch/<A>/<B>`` nor of the GraphSAINT
family, the other modes (sgc and the cluster models), the DP-SGD trainer types (the
reference has the flags and no code), and the full-batch branch (no ``--batch``) on a dataset that is not a transfer dataset,
which cannot run in the reference either (it reads ``features_1``).  ``--data-root`` (an addition) says where ./data lives.
"""
from __future__ import annotations

import argparse
import logging

_OPTIONS = {
    "seed": (int, 42), "num-epochs": (int, 500), "lr": (float, 0.2), "weight_decay": (float, 5e-6), "hidden": (int, 16),
    "depth": (int, 1), "dropout": (float, 0.5), "dataset": (str, "cora"), "model-path": (str, ""), "mode": (str, "sgc"),
    "scale": (str, "small"), "normalization": (str, "AugNormAdj", ["AugNormAdj"]), "l2-norm-clip": (float, 1.0),
    "noise-multiplier": (float, 1.1), "microbatch-size": (int, 1), "minibatch-size": (int, 256), "l2-penalty": (float, 0.001),
    "epsilon": (float, 0.1), "delta": (float, 1e-5), "train-ratio": (float, 0.5), "patience": (int, 50),
    "batch-size": (int, 256), "k": (float, 1), "noise-seed": (int, 42), "cluster-seed": (int, 42),
    "noise-type": (str, "gaussian"),
    "trainer-type": (str, "mlp", ["mlp", "dp_mlp", "lr", "dp_lr", "multi_mlp", "dp_multi_mlp"]),
    "feature-size": (int, -1), "iterations": (int, 14000), "coeff": (float, 1), "degree": (int, 2),
    "data-root": (str, "./data"),      # addition
}
_SWITCHES = ["batch", "test", "display", "trainable", "early"]


def build_parser():
    p = argparse.ArgumentParser(description="feature-only MLP baselines on MI355X")
    for name, spec in _OPTIONS.items():
        kw = dict(type=spec[0], default=spec[1])
        if len(spec) > 2:
            kw["choices"] = spec[2]
        p.add_argument(f"--{name}", **kw)
    for name in _SWITCHES:
        p.add_argument(f"--{name}", action="store_true", default=False)
    p.set_defaults(assign_seed=42)
    return p


def get_arguments(argv=None):
    return build_parser().parse_args(argv)


def check_served(args):
    """What the flags alone decide is refused here, before any file is read or written or the GPU is touched."""
    from .worker import is_served, is_transfer      # (module import only: no data, no device)
    if args.mode != "mlp":
        raise NotImplementedError(f"--mode {args.mode}: main_simple serves --mode mlp (the feature-only baselines); sgc and the "
                                  "cluster models are out of scope")
    if args.depth not in (1, 2):
        raise NotImplementedError(f"--depth {args.depth}: 1 (OneLayerMLP) or 2 (SingleHiddenLayerMLP)")
    if args.trainer_type != "mlp":
        raise NotImplementedError(f"--trainer-type {args.trainer_type}: only mlp is served (the reference has the DP-SGD flags and "
                                  "no code behind them)")
    if not is_served(args.dataset):
        raise NotImplementedError(f"--dataset {args.dataset} not implemented! (served: twitch/<A>/<B>, reddit, flickr, ppi, ppi-large)")
    if args.test:
        if not args.model_path:
            raise ValueError("--test needs --model-path")
        return
    if not args.batch and not is_transfer(args.dataset):
        raise NotImplementedError(f"--dataset {args.dataset} without --batch: the full-batch branch reads features_1 and runs on "
                                  "transfer datasets only, in the reference too; pass --batch")
    if args.batch and args.batch_size < 1:
        raise ValueError(f"--batch-size {args.batch_size}: at least 1")
    if args.depth == 2 and not 1 <= args.hidden <= 256:
        raise NotImplementedError(f"--hidden {args.hidden}: the hidden width is at most 256")


def main(argv=None):
    args = get_arguments(argv)
    check_served(args)
    import datetime

    import numpy as np
    import torch

    from .main import init_logger
    from .mlp_trainer import MLPTrainer
    from .worker import FeatureData
    print(str(args))
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(args.seed)
    if args.test:
        worker = FeatureData(args.dataset, mode=args.mode, data_root=args.data_root)
        trainer = MLPTrainer(args, worker=worker, train=False)
        trainer.init_model(model_path=args.model_path)
        trainer.test()
        return trainer
    cur_time = datetime.datetime.now().strftime("%m-%d-%H:%M:%S.%f")
    subdir = "mode-{}_hidden-{}_lr-{}_decay-{}_dropout-{}_bs-{}_{}".format(args.mode, args.hidden, args.lr, args.weight_decay,
                                                                         args.dropout, args.batch_size, cur_time)
    print("subdir = {}".format(subdir))
    handler = init_logger("./logs_{}".format(args.dataset), subdir)
    try:
        logging.info(str(args))
        worker = FeatureData(args.dataset, mode=args.mode, data_root=args.data_root)
        trainer = MLPTrainer(args, subdir=subdir, worker=worker, train=True)
        trainer.init_model()
        trainer.train()
        trainer.test()
    finally:
        logging.getLogger().removeHandler(handler)
        handler.close()
    return trainer


if __name__ == "__main__":
    main()

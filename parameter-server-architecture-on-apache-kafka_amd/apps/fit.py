"""Fit a model to a training file until the optimiser converges.

Usage: python -m psx.apps.fit --train train.csv [--test test.csv] [--valid valid.csv | --valid_frac 0.1 --seed 0]
           [--reg_param 0] [--max_iter 100] [--tol 1e-6] [--init_checkpoint DIR] [--checkpoint_dir OUT]
           [--device ...] [--header auto|yes|no] [--label_col -1] [--num_classes K]
       python -m psx.apps.fit --train train.svm [--num_features F] [--sigmoid] [--zero_based] [...]

CSVs and binary row caches fit the dense model.  A LIBSVM file (``.svm``, ``.libsvm``,
``.svmlight``) fits the wide model over ``--num_features`` hashed features (default: the
largest training id + 1); ``--sigmoid`` selects the one-logit model with labels {0, 1},
``--zero_based`` files whose feature ids start at 0.  ``--valid`` / ``--valid_frac`` score
the iterates on held-out rows and keep the best one (``--patience N`` stops after N checks
without improvement).  ``--checkpoint_dir`` gets a ``server.ckpt`` that
``python -m psx.apps.predict`` reads.  stdout gets one JSON line: rows, features,
classes, iterations, evaluations, reason, objective, train log-loss, the test metrics
(through the Scorer) and the fit's seconds; a wide fit adds ``touched_features``.
``-h`` exits 0, stray arguments exit 2.
"""
from __future__ import annotations

import json
import sys

import torch

from .cli import _Parser, parse_or_exit


def fit_parser():
    ap = _Parser(prog="fit", add_help=False)
    ap.add_argument("-h", "--help", action="store_true", help="Show list of possible parameter")
    ap.add_argument("--train", default=None, help="training rows: CSV, binary cache or LIBSVM (wide model)")
    ap.add_argument("--test", default=None, help="rows to report accuracy / weighted F1 / log-loss on")
    ap.add_argument("--valid", default=None, help="validation rows (keeps the iterate with the lowest log-loss)")
    ap.add_argument("--valid_frac", type=float, default=0.0, help="hold this share of --train out for validation")
    ap.add_argument("--valid_every", type=int, default=1, help="accepted iterations between validation checks")
    ap.add_argument("--patience", type=int, default=None, help="stop after this many checks without improvement")
    ap.add_argument("--seed", type=int, default=0, help="seed of the --valid_frac split")
    ap.add_argument("--reg_param", type=float, default=0.0, help="L2 penalty on the standardised coefficients")
    ap.add_argument("--max_iter", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--init_checkpoint", default=None, help="warm start from this checkpoint directory")
    ap.add_argument("--checkpoint_dir", default=None, help="write server.ckpt here")
    ap.add_argument("--device", default=None, help="cpu | cuda | cuda:N (default: cuda if available)")
    ap.add_argument("--header", default="auto", choices=["auto", "yes", "no"])
    ap.add_argument("--label_col", type=int, default=-1)
    ap.add_argument("--num_classes", type=int, default=None, help="K (default: largest training label + 1)")
    ap.add_argument("--num_features", type=int, default=None, help="wide model: F (default: largest training id + 1)")
    ap.add_argument("--sigmoid", action="store_true", help="wide model: one logit, labels {0, 1}")
    ap.add_argument("--zero_based", action="store_true", help="LIBSVM feature ids start at 0")
    return ap


def _take_sparse(ds, rows):
    """The given rows of a SparseDataset, in that order."""
    from ..ops.sparse import SparseDataset

    cnt = (ds.indptr[1:] - ds.indptr[:-1])[rows]
    ip = torch.zeros(rows.numel() + 1, dtype=torch.int64)
    torch.cumsum(cnt, 0, out=ip[1:])
    src = torch.repeat_interleave(ds.indptr[rows] - ip[:-1], cnt) + torch.arange(int(ip[-1]))
    return SparseDataset(ip, ds.idx[src], ds.val[src], ds.y[rows], ds.num_features)


def main(argv=None) -> int:
    ap = fit_parser()
    a = parse_or_exit(ap, sys.argv[1:] if argv is None else argv)
    if not a.train:
        ap.error("--train is required")
    if a.valid and a.valid_frac:
        ap.error("--valid and --valid_frac exclude each other")
    if not 0.0 <= a.valid_frac < 1.0:
        ap.error("--valid_frac must be in [0, 1)")
    from ..models.logreg import ModelSpec
    from ..models.wide import WideSpec
    from ..ops.fit import BatchFitter, FitOptions
    from ..ops.score import Scorer
    from ..ops.wide_fit import WideFitter
    from ..utils import data as data_mod
    from ..utils.data import Dataset

    wide = data_mod.is_libsvm_path(a.train)
    if not wide and (a.num_features is not None or a.sigmoid or a.zero_based):
        ap.error("--num_features, --sigmoid and --zero_based go with a LIBSVM --train file (the wide model)")
    num_features = a.num_features

    def load(path):
        if wide:
            try:
                return data_mod.load_libsvm(path, num_features=num_features, zero_based=a.zero_based)
            except ValueError as e:
                ap.error(str(e))
        return data_mod.load_any(path, header=a.header, label_col=a.label_col)

    device = a.device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    train = load(a.train)
    num_features = train.num_features  # the other files must fit the model the training file sizes
    valid = load(a.valid) if a.valid else None
    if a.valid_frac > 0.0:
        g = torch.Generator().manual_seed(a.seed)
        perm = torch.randperm(train.rows, generator=g)
        nv = max(1, int(round(train.rows * a.valid_frac)))
        vi, ti = perm[:nv].sort().values, perm[nv:].sort().values
        if wide:
            valid, train = _take_sparse(train, vi), _take_sparse(train, ti)
        else:
            valid = Dataset(train.X[vi], train.y[vi], train.num_features, train.names)
            train = Dataset(train.X[ti], train.y[ti], train.num_features, train.names)
    if wide and a.sigmoid:
        K = 1
    else:
        K = a.num_classes if a.num_classes is not None else max(2, int(train.y.max()) + 1)
    spec = WideSpec(train.num_features, K) if wide else ModelSpec(train.num_features, K)
    w0 = None
    if a.init_checkpoint:
        init = Scorer.from_checkpoint(a.init_checkpoint, "cpu")
        if init.wide != wide or init.spec != spec:
            ap.error(f"--init_checkpoint holds {init.spec}, the data needs {spec}")
        w0 = init.w
    try:
        opts = FitOptions(max_iter=a.max_iter, tol=a.tol, reg_param=a.reg_param)
        fitter = WideFitter(spec, device, opts) if wide else BatchFitter(spec, device, opts)
        res = fitter.fit(train, w0=w0, valid=valid, valid_every=a.valid_every, patience=a.patience)
    except ValueError as e:
        ap.error(str(e))
    if a.checkpoint_dir:
        res.save(a.checkpoint_dir)
    line = {"rows": train.rows, "features": spec.F, "classes": spec.K, "iterations": res.iters,
            "evaluations": res.evals, "reason": res.reason, "objective": res.objective,
            "train_log_loss": res.log_loss, "reg_param": a.reg_param}
    if wide:
        line.update(touched_features=int(res.features.numel()))
    if valid is not None:
        line.update(valid_rows=valid.rows, best_iteration=res.best_iter,
                    valid_log_loss=min(v for _, v in res.valid_history))
    if a.test:
        sc = Scorer(spec, res.w, device).score(load(a.test))
        line.update(test_rows=sc.rows, test_accuracy=sc.accuracy, test_f1=sc.f1, test_log_loss=sc.log_loss)
    line.update(device=str(fitter.device), fit_seconds=res.seconds, pass_seconds=res.pass_seconds)
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())

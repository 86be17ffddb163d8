"""Score a data file with a trained model (a checkpoint of a parameter-server run).

Usage: python -m psx.apps.predict --checkpoint_dir DIR --data test.csv [--out preds.csv] [--proba]
           [--ignore_labels] [--chunk_rows N] [--device ...] [--header auto|yes|no] [--label_col -1]
           [--curves] [--curves_out FILE.json]

The data file is a CSV or a binary row cache for a dense model, LIBSVM text for a
wide one.  The loaders always parse a label column; a file without real labels
carries a placeholder there, and ``--ignore_labels`` leaves the metrics and the
per-row loss out.  ``--out`` gets one line per row, ``row,pred[,label,nll][,p0..]``;
stdout gets one JSON line (rows, metrics, the model's shape, rows per second).
``--curves`` counts the score histogram in the same pass and prints a second JSON
line after that one: ``auc_macro``, ``auc_weighted``, ``ap_macro``, ``ece`` and the
per-class one-vs-rest ROC AUC with its resolution; ``--curves_out`` writes the table
and everything derived from it (it implies ``--curves``).  Curves need labels: with
``--ignore_labels`` they exit 2.
``-h`` exits 0, stray arguments exit 2 (the other front ends' conventions).
"""
from __future__ import annotations

import json
import sys
import time

import numpy as np
import torch

from .cli import _Parser, parse_or_exit


def predict_parser():
    ap = _Parser(prog="predict", add_help=False)
    ap.add_argument("-h", "--help", action="store_true", help="Show list of possible parameter")
    ap.add_argument("--checkpoint_dir", default=None, help="checkpoint directory (or a server.ckpt file)")
    ap.add_argument("--data", default=None, help="rows to score: CSV / binary cache (dense model), LIBSVM (wide model)")
    ap.add_argument("--out", default=None, help="write one line per row: row,pred[,label,nll][,p0..p{C-1}]")
    ap.add_argument("--proba", action="store_true", help="also write the class probabilities")
    ap.add_argument("--ignore_labels", action="store_true",
                    help="the label column is a placeholder: no metrics, no per-row loss")
    ap.add_argument("--chunk_rows", type=int, default=1 << 20, help="rows moved to the device at a time")
    ap.add_argument("--device", default=None, help="cpu | cuda | cuda:N (default: cuda if available)")
    ap.add_argument("--header", default="auto", choices=["auto", "yes", "no"])
    ap.add_argument("--label_col", type=int, default=-1)
    ap.add_argument("--curves", action="store_true",
                    help="also print ROC AUC, average precision and calibration error (needs labels)")
    ap.add_argument("--curves_out", default=None, help="write the score histogram and the derived numbers as JSON")
    return ap


def _load(path: str, scorer, a):
    from ..utils import data as data_mod

    if scorer.wide:
        return data_mod.load_libsvm(path, num_features=scorer.spec.F)
    return data_mod.load_any(path, header=a.header, label_col=a.label_col)


def write_rows(path: str, res, labels: torch.Tensor | None) -> None:
    cols = [np.arange(res.rows, dtype=np.float64), res.pred.cpu().numpy().astype(np.float64)]
    names, fmts = ["row", "pred"], ["%d", "%d"]
    if res.nll is not None:
        cols += [labels.cpu().numpy().astype(np.float64), res.nll.cpu().numpy().astype(np.float64)]
        names += ["label", "nll"]
        fmts += ["%d", "%.6g"]
    if res.proba is not None:
        p = res.proba.cpu().numpy().astype(np.float64)
        cols += [p[:, c] for c in range(p.shape[1])]
        names += [f"p{c}" for c in range(p.shape[1])]
        fmts += ["%.6g"] * p.shape[1]
    with open(path, "w") as f:
        f.write(",".join(names) + "\n")
        np.savetxt(f, np.stack(cols, 1).reshape(res.rows, len(cols)), delimiter=",", fmt=fmts)


def _nums(v) -> list:
    """A float array as JSON: NaN (a class without both sides) becomes null."""
    return [None if x != x else float(x) for x in np.asarray(v, dtype=np.float64).tolist()]


def curves_line(res) -> dict:
    return {"auc_macro": res.auc_macro, "auc_weighted": res.auc_weighted, "ap_macro": res.ap_macro, "ece": res.ece,
            "auc": _nums(res.auc), "auc_resolution": _nums(res.auc_resolution)}


def write_curves(path: str, res) -> None:
    from ..utils import metrics as M

    h = res.hist.numpy()
    doc = curves_line(res)
    doc.update(ap=_nums(res.ap), ks=_nums(M.ks_statistic(h)), ece_per_class=_nums(M.ece(h)),
               bins=M.HIST_BINS, bins_per_unit_log_odds=M.HIST_PER_UNIT, hist=res.hist.tolist())
    with open(path, "w") as f:
        json.dump(doc, f)


def main(argv=None) -> int:
    ap = predict_parser()
    a = parse_or_exit(ap, sys.argv[1:] if argv is None else argv)
    if not a.checkpoint_dir or not a.data:
        ap.error("--checkpoint_dir and --data are required")
    curves = a.curves or a.curves_out is not None
    if curves and a.ignore_labels:
        ap.error("--curves needs labels: it cannot be combined with --ignore_labels")
    from ..ops.score import Scorer

    device = a.device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    scorer = Scorer.from_checkpoint(a.checkpoint_dir, device)
    ds = _load(a.data, scorer, a)
    labels = not a.ignore_labels
    t0 = time.perf_counter()
    res = scorer.score(ds, labels=labels, proba=a.proba, chunk_rows=a.chunk_rows, **({"curves": True} if curves else {}))
    if scorer.device.type == "cuda":
        torch.cuda.synchronize(scorer.device)
    dt = time.perf_counter() - t0
    if a.out:
        write_rows(a.out, res, ds.y if labels else None)
    spec = scorer.spec
    line = {"rows": res.rows, "rows_out_of_range": res.rows_out_of_range}
    if labels:
        line.update(accuracy=res.accuracy, f1=res.f1, log_loss=res.log_loss, confusion=res.confusion.tolist())
    line.update(model="wide" if scorer.wide else "dense", num_features=spec.F, num_classes=spec.K,
                device=str(scorer.device), rows_per_s=res.rows / dt if dt > 0 else 0.0)
    print(json.dumps(line))
    if curves:
        print(json.dumps(curves_line(res)))
        if a.curves_out:
            write_curves(a.curves_out, res)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Classification metrics with Spark MulticlassMetrics semantics.

Reference: Metrics.java:15-24 uses MulticlassClassificationEvaluator with metric
names "f1" (= weightedFMeasure) and "accuracy".  weightedFMeasure sums, over
the labels that occur in the data, (label count / total) * F1(label), where a
label's precision/recall is 0 when its denominator is 0.
"""
from __future__ import annotations

import numpy as np


def metrics_from_confusion(conf) -> tuple[float, float]:
    """(weighted F1, accuracy) from a confusion matrix [true][pred]."""
    c = np.asarray(conf, dtype=np.float64)
    total = c.sum()
    if total <= 0:
        return 0.0, 0.0
    tp = np.diag(c)
    true_count = c.sum(axis=1)
    pred_count = c.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(pred_count > 0, tp / pred_count, 0.0)
        rec = np.where(true_count > 0, tp / true_count, 0.0)
        f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
    wf1 = float((true_count / total * f1).sum())
    acc = float(tp.sum() / total)
    return wf1, acc


def confusion(y_true, y_pred, num_classes: int) -> np.ndarray:
    y_true = np.asarray(y_true, dtype=np.int64)
    y_pred = np.asarray(y_pred, dtype=np.int64)
    m = np.zeros((num_classes, num_classes), dtype=np.int64)
    np.add.at(m, (y_true, y_pred), 1)
    return m


# ---- ranking metrics from a score histogram ---------------------------------------
# The scoring pass (psx.ops.score, csrc/kernels/score_kernels.h) counts, per class c
# and label side, the one-vs-rest log-odds l_c = log(p_c / (1 - p_c)) of every row in
# HIST_BINS bins of width 1 / HIST_PER_UNIT: bin b holds the rows with
# round(HIST_PER_UNIT * l_c) == b - HIST_BINS / 2 (the end bins also hold everything
# beyond them).  hist[c, 1] counts the rows labelled c, hist[c, 0] all other rows.
# Everything below is a pure function of such a table ([Ch, 2, HIST_BINS], integers):
# tables of chunks, datasets or ranks add, and so nothing here is model-specific.
HIST_BINS = 512
HIST_SIDES = 2
HIST_PER_UNIT = 16


def _table(hist) -> np.ndarray:
    h = np.asarray(hist)
    if h.ndim != 3 or h.shape[1] != HIST_SIDES:
        raise ValueError(f"a score histogram is [classes, {HIST_SIDES}, bins], got {h.shape}")
    return h.astype(np.float64)


def bin_centres(nbins: int = HIST_BINS) -> np.ndarray:
    """Log-odds at the middle of each bin."""
    return (np.arange(nbins) - nbins // 2) / HIST_PER_UNIT


def bin_edges(nbins: int = HIST_BINS) -> np.ndarray:
    """The nbins + 1 log-odds between the bins (the two outer ones are nominal: the end bins are open)."""
    return (np.arange(nbins + 1) - nbins // 2 - 0.5) / HIST_PER_UNIT


def nanmean(v) -> float:
    v = np.asarray(v, dtype=np.float64)
    ok = ~np.isnan(v)
    return float(v[ok].mean()) if ok.any() else float("nan")


def roc_auc(hist) -> tuple[np.ndarray, np.ndarray]:
    """(auc [Ch], resolution [Ch]).  auc is the exact ROC AUC of the binned scores,
    ties inside a bin counting one half; the AUC of the unbinned scores lies within
    resolution of it (only pairs that share a bin are undecided).  NaN for a class
    without positive or without negative rows."""
    h = _table(hist)
    neg, pos = h[:, 0], h[:, 1]
    P, N = pos.sum(1), neg.sum(1)
    above = P[:, None] - np.cumsum(pos, 1)  # positives in the bins above b
    with np.errstate(divide="ignore", invalid="ignore"):
        auc = (neg * (above + 0.5 * pos)).sum(1) / (P * N)
        res = 0.5 * (pos * neg).sum(1) / (P * N)
    bad = (P == 0) | (N == 0)
    auc[bad] = np.nan
    res[bad] = np.nan
    return auc, res


def auc_summary(hist, auc=None) -> tuple[float, float]:
    """(macro, weighted): the mean of the per-class AUC over the classes that have both
    sides, and the same weighted by the classes' positives.  NaN when no class has both."""
    if auc is None:
        auc = roc_auc(hist)[0]
    P = _table(hist)[:, 1].sum(1)
    ok = ~np.isnan(auc)
    if not ok.any():
        return float("nan"), float("nan")
    return float(auc[ok].mean()), float((auc[ok] * P[ok]).sum() / P[ok].sum())


def _descending(h):
    """Cumulative (tp, fp) after each bin, from the highest bin down."""
    return np.cumsum(h[:, 1, ::-1], 1), np.cumsum(h[:, 0, ::-1], 1)


def average_precision(hist) -> np.ndarray:
    """[Ch] step-wise average precision, sum over descending bins of (recall step) x
    precision, a bin being one tie group: sklearn's definition applied to the bin
    centres.  NaN for a class without positive rows."""
    h = _table(hist)
    tp, fp = _descending(h)
    P = h[:, 1].sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(tp + fp > 0, tp / (tp + fp), 0.0)
        ap = (h[:, 1, ::-1] * prec).sum(1) / P
    ap[P == 0] = np.nan
    return ap


def roc_curve(hist, c: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(fpr, tpr, thresholds) of class c, one point per bin edge from the highest
    (nothing predicted positive: 0, 0) to the lowest (1, 1); a row is predicted
    positive when its log-odds lie above the threshold."""
    h = _table(hist)[c: c + 1]
    tp, fp = _descending(h)
    P, N = h[0, 1].sum(), h[0, 0].sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        tpr = np.concatenate([[0.0], tp[0] / P])
        fpr = np.concatenate([[0.0], fp[0] / N])
    return fpr, tpr, bin_edges(h.shape[2])[::-1].copy()


def pr_curve(hist, c: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(precision, recall, thresholds) of class c at the same thresholds as roc_curve;
    the precision of predicting nothing is 1 (sklearn's convention)."""
    h = _table(hist)[c: c + 1]
    tp, fp = _descending(h)
    P = h[0, 1].sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.concatenate([[1.0], np.where(tp[0] + fp[0] > 0, tp[0] / (tp[0] + fp[0]), 1.0)])
        rec = np.concatenate([[0.0], tp[0] / P])
    return prec, rec, bin_edges(h.shape[2])[::-1].copy()


def ks_statistic(hist) -> np.ndarray:
    """[Ch] Kolmogorov-Smirnov distance between the two sides' score distributions,
    the largest gap of their cumulative shares over the bin edges; NaN without both sides."""
    h = _table(hist)
    P, N = h[:, 1].sum(1), h[:, 0].sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ks = np.abs(np.cumsum(h[:, 1], 1) / P[:, None] - np.cumsum(h[:, 0], 1) / N[:, None]).max(1)
    ks[(P == 0) | (N == 0)] = np.nan
    return ks


def calibration(hist, c: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Reliability table of class c over its non-empty bins: (predicted probability
    sigmoid(bin centre), observed share of positive rows, rows)."""
    h = _table(hist)[c]
    n = h[0] + h[1]
    keep = n > 0
    pred = 1.0 / (1.0 + np.exp(-bin_centres(h.shape[1])))
    return pred[keep], h[1][keep] / n[keep], n[keep]


def ece(hist) -> np.ndarray:
    """[Ch] expected calibration error: the row-weighted mean of |observed - predicted|
    over calibration()'s bins; NaN for a class without rows."""
    h = _table(hist)
    out = np.full(h.shape[0], np.nan)
    for c in range(h.shape[0]):
        pred, obs, n = calibration(h, c)
        if n.size:
            out[c] = float((n * np.abs(obs - pred)).sum() / n.sum())
    return out

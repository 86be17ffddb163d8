"""Scoring a dataset with a trained model: per-row predictions, class
probabilities and loss, plus the confusion counts and the metrics the training
logs report.

GPU: every number comes from the fused kernels of ``csrc/kernels/score_kernels.hip``
(one pass over the rows and one launch per chunk; a missing extension is a hard
error).  CPU: the same class runs a PyTorch path on float32 margins, as the other
ops' CPU paths do.

The reference's own ``predict()`` was dead code; its only consumer of
trained weights was the evaluation inside the training loop.
"""
from __future__ import annotations

import os
import warnings
from dataclasses import dataclass

import numpy as np
import torch

from .. import _native
from ..models.logreg import ModelSpec, from_reference_layout
from ..models.wide import WideSpec
from ..utils.checkpoint import CKPT_NAME
from ..utils.data import Dataset
from ..utils import metrics as M
from ..utils.metrics import metrics_from_confusion
from .lr import Fragments, is_gpu, stream_handle
from .sparse import SparseDataset


@dataclass
class ScoreResult:
    """Per-row outputs live on the scorer's device; everything else on the host.

    Without labels ``nll``, ``confusion``, ``log_loss``, ``f1`` and ``accuracy``
    are None and ``rows_out_of_range`` is 0.  The fields from ``hist`` on are None
    unless the call asked for ``curves``: ``hist`` is the distribution of the
    one-vs-rest log-odds per class and label side (``Ch`` = K, the binary model: 1;
    bins and sides as in :mod:`psx.utils.metrics`), the rest is derived from it."""

    pred: torch.Tensor  # [T] int32
    proba: torch.Tensor | None  # [T, C] float32
    nll: torch.Tensor | None  # [T] float32; NaN where the label is outside [0, K)
    confusion: torch.Tensor | None  # [C, C] int64, [label][prediction]
    rows: int
    rows_out_of_range: int
    log_loss: float | None  # mean of the finite nll entries
    f1: float | None
    accuracy: float | None
    hist: torch.Tensor | None = None  # [Ch, 2, 512] int64, [class][side][bin]
    auc: np.ndarray | None = None  # [Ch] one-vs-rest ROC AUC of the binned scores; NaN without both sides
    auc_resolution: np.ndarray | None = None  # [Ch] the unbinned scores' AUC lies within it
    auc_macro: float | None = None  # mean over the classes that have both sides
    auc_weighted: float | None = None  # the same classes, weighted by their positives
    ap: np.ndarray | None = None  # [Ch] average precision
    ap_macro: float | None = None
    ece: float | None = None  # expected calibration error, the mean of the classes' one-vs-rest ECE


HIST_FORMS = {"auto": 0, "lds": 1, "global": 2}


def hist_form_from_env() -> int:
    """``PSX_SCORE_HIST_FORM``: the dense kernel's histogram form -- ``auto`` (the
    workgroup-private LDS table where it fits, else global atomics), ``lds`` or
    ``global``.  Both give the same table."""
    v = os.environ.get("PSX_SCORE_HIST_FORM", "auto").strip().lower()
    if v not in HIST_FORMS:
        raise ValueError(f"PSX_SCORE_HIST_FORM must be one of {sorted(HIST_FORMS)}, got {v!r}")
    return HIST_FORMS[v]


def _nan_to_none(v: float) -> float | None:
    return None if v != v else float(v)


def _row_order_sum(v: np.ndarray) -> float:
    return float(np.cumsum(v, dtype=np.float64)[-1]) if v.size else 0.0


class Scorer:
    """A trained model ready to score datasets.

    ``spec`` is a :class:`ModelSpec` (dense) or :class:`WideSpec` (wide; ``K == 1``
    is the binary sigmoid model); ``w`` the fp32 weights in that spec's device
    layout ``[P]``.  The scorer keeps its own copy of ``w`` on ``device``."""

    def __init__(self, spec, w: torch.Tensor, device):
        if not isinstance(spec, (ModelSpec, WideSpec)):
            raise TypeError(f"spec must be a ModelSpec or a WideSpec, not {type(spec).__name__}")
        if w.numel() != spec.P:
            raise ValueError(f"the model has {spec.P} weights in device layout, got {w.numel()}")
        self.spec = spec
        self.device = torch.device(device)
        self.wide = isinstance(spec, WideSpec)
        if not 1 <= spec.K <= 16 or (spec.K < 2 and not self.wide):
            raise ValueError(f"{spec.K} classes: the dense model scores 2..16, the wide model 1 (sigmoid)..16")
        self.w = w.detach().to(self.device, torch.float32).reshape(-1).clone()
        self.frag = None
        if is_gpu(self.device) and not self.wide:
            self.frag = Fragments(spec, self.device)
            self.frag.refresh(self.w)
        self._Wcpu = None
        self._hist_form = 0  # score(curves=True) reads PSX_SCORE_HIST_FORM

    # ---- constructors --------------------------------------------------------
    @classmethod
    def from_checkpoint(cls, path: str, device) -> "Scorer":
        """From a checkpoint directory or a ``server.ckpt`` file."""
        if os.path.isdir(path):
            path = os.path.join(path, CKPT_NAME)
        state = torch.load(path, map_location="cpu", weights_only=True)
        kind = state.get("model", "dense")
        F, K = int(state["num_features"]), int(state["num_classes"])
        if kind == "wide":
            spec = WideSpec(F, K)
        elif kind == "dense":
            spec = ModelSpec(F, K)
        else:
            raise ValueError(f"{path}: unknown model kind {kind!r}")
        if "w" in state:
            w = state["w"]
        elif kind == "dense" and "w_reference_layout" in state:
            w = from_reference_layout(spec, state["w_reference_layout"])
        else:
            raise ValueError(f"{path}: the checkpoint holds no weights")
        return cls(spec, w, device)

    @classmethod
    def from_engine(cls, engine) -> "Scorer":
        """A snapshot of the live server weights of a LocalEngine or of a DistEngine
        server rank, on that engine's device."""
        srv = getattr(engine, "server", None)
        if srv is None:
            raise ValueError(f"{type(engine).__name__} holds no whole server model on this rank: a key-range rank "
                             "stores only its slice of the weights, and a worker rank none (score from rank 0 of a "
                             "replicated schedule, or from a checkpoint)")
        if is_gpu(srv.device):
            torch.cuda.synchronize(srv.device)  # updates in flight on the engine's streams
        return cls(srv.spec, srv.w, srv.device)

    # ---- scoring ---------------------------------------------------------------
    def _check(self, ds):
        s = self.spec
        if self.wide:
            if not isinstance(ds, SparseDataset):
                raise ValueError(f"the wide model ({s.F} features, {s.K} classes) scores sparse rows "
                                 f"(SparseDataset), got {type(ds).__name__}")
            if ds.num_features > s.F:
                raise ValueError(f"the data has {ds.num_features} features, the model only {s.F}")
            if ds.nnz and (int(ds.idx.min()) < 0 or int(ds.idx.max()) >= s.F):
                raise ValueError(f"feature ids reach {int(ds.idx.max())} (lowest {int(ds.idx.min())}), the model "
                                 f"has {s.F} features")
            return
        if not isinstance(ds, Dataset):
            raise ValueError(f"the dense model ({s.F} features, {s.K} classes) scores dense rows (Dataset), "
                             f"got {type(ds).__name__}")
        if ds.num_features != s.F or ds.Fp != s.Fp:
            raise ValueError(f"the data is {ds.num_features} features wide (padded {ds.Fp}), the model "
                             f"{s.F} (padded {s.Fp})")

    def score(self, ds, labels: bool = True, proba: bool = False, chunk_rows: int = 1 << 20,
              curves: bool = False) -> ScoreResult:
        """Score every row of ``ds`` (a :class:`Dataset` for the dense model, a
        :class:`SparseDataset` for the wide one, on any device).  Rows move to the
        scorer's device ``chunk_rows`` at a time, so a set larger than device memory
        can be scored.  ``labels=False`` ignores ``ds.y``.  ``curves=True`` also counts
        the score histogram in the same pass (it needs labels) and derives ROC AUC,
        average precision and the calibration error from it."""
        if curves and not labels:
            raise ValueError("curves=True needs labels: the score histogram is kept per label side")
        self._check(ds)
        chunk_rows = int(chunk_rows)
        if not 1 <= chunk_rows < 1 << 31:
            raise ValueError(f"chunk_rows must be in [1, 2^31), got {chunk_rows}")
        s, dev = self.spec, self.device
        T, C = ds.rows, s.eval_classes
        pred = torch.empty(T, dtype=torch.int32, device=dev)
        pr = torch.empty(T, C, dtype=torch.float32, device=dev) if proba else None
        nll = torch.empty(T, dtype=torch.float32, device=dev) if labels else None
        counts = torch.zeros(257, dtype=torch.int32, device=dev)  # [16][16] confusion cells, then rows out of range
        hist = hist32 = None
        if curves:  # a chunk counts in int32 (under 2^31 rows), the chunks add up in int64
            hist = torch.zeros(s.K * M.HIST_SIDES * M.HIST_BINS, dtype=torch.int64, device=dev)
            hist32 = torch.zeros_like(hist, dtype=torch.int32)
            self._hist_form = hist_form_from_env()
        for r0 in range(0, T, chunk_rows):
            r1 = min(T, r0 + chunk_rows)
            out = (pred[r0:r1], pr[r0:r1] if proba else None, nll[r0:r1] if labels else None, hist32)
            if self.wide:
                part = ds.slice(r0, r1).to(dev)
                part = SparseDataset(part.indptr.to(torch.int64).contiguous(), part.idx.to(torch.int32).contiguous(),
                                     part.val.to(torch.bfloat16).contiguous(), part.y.to(torch.int32).contiguous(),
                                     part.num_features)
                (self._wide_gpu if is_gpu(dev) else self._wide_cpu)(part, labels, out, counts)
            else:
                X = ds.X[r0:r1].to(dev, torch.bfloat16).contiguous()  # dense rows are scored as bf16 (as EvalSet)
                y = ds.y[r0:r1].to(dev, torch.int32).contiguous()
                (self._dense_gpu if is_gpu(dev) else self._dense_cpu)(X, y, labels, out, counts)
            if curves:
                hist += hist32
                hist32.zero_()
        if not labels:
            return ScoreResult(pred, pr, None, None, T, 0, None, None, None)
        host = counts.cpu()
        conf = host[:256].view(16, 16)[:C, :C].to(torch.int64).clone()
        v = nll.cpu().numpy().astype(np.float64)
        v = v[np.isfinite(v)]
        f1, acc = metrics_from_confusion(conf.numpy())
        res = ScoreResult(pred, pr, nll, conf, T, int(host[256]), _row_order_sum(v) / v.size if v.size else None,
                          f1, acc)
        if curves:
            res.hist = hist.cpu().view(s.K, M.HIST_SIDES, M.HIST_BINS)
            h = res.hist.numpy()
            res.auc, res.auc_resolution = M.roc_auc(h)
            res.auc_macro, res.auc_weighted = (_nan_to_none(x) for x in M.auc_summary(h, res.auc))
            res.ap = M.average_precision(h)
            res.ap_macro = _nan_to_none(M.nanmean(res.ap))
            res.ece = _nan_to_none(M.nanmean(M.ece(h)))
        return res

    def predict(self, ds, chunk_rows: int = 1 << 20) -> torch.Tensor:
        return self.score(ds, labels=False, chunk_rows=chunk_rows).pred

    def predict_proba(self, ds, chunk_rows: int = 1 << 20) -> torch.Tensor:
        return self.score(ds, labels=False, proba=True, chunk_rows=chunk_rows).proba

    # ---- GPU: the fused kernels ------------------------------------------------
    @staticmethod
    def _ptrs(labels, out, counts):
        pred, pr, nll, hist = out
        p = dict(pred=pred.data_ptr(), proba=pr.data_ptr() if pr is not None else 0,
                 nll=nll.data_ptr() if nll is not None else 0, conf=counts.data_ptr() if labels else 0,
                 oor=counts.data_ptr() + 1024 if labels else 0)
        if hist is not None:  # a plain call passes what it always passed
            p["hist"] = hist.data_ptr()
        return p

    def _dense_gpu(self, X, y, labels, out, counts):
        s, f = self.spec, self.frag
        form = dict(hist_form=self._hist_form) if out[3] is not None else {}
        _native.hip().score(s.Fp, s.K, X.data_ptr(), y.data_ptr() if labels else 0, int(X.shape[0]), f.hi.data_ptr(),
                            f.lo.data_ptr(), f.b.data_ptr(), stream=stream_handle(self.device),
                            **self._ptrs(labels, out, counts), **form)

    def _wide_gpu(self, part, labels, out, counts):
        s = self.spec
        _native.hip().wide_score(s.K, s.KP, s.F, part.indptr.data_ptr(), part.idx.data_ptr(), part.val.data_ptr(),
                                 part.y.data_ptr() if labels else 0, part.rows, self.w.data_ptr(),
                                 stream=stream_handle(self.device), **self._ptrs(labels, out, counts))

    # ---- CPU: PyTorch on float32 margins -----------------------------------------
    def _dense_cpu(self, X, y, labels, out, counts):
        s = self.spec
        z = X[:, : s.F].float() @ s.coef(self.w).t() + s.intercept(self.w)
        self._finish_cpu(z, y, labels, out, counts)

    def _wide_cpu(self, part, labels, out, counts):
        s = self.spec
        if self._Wcpu is None:
            self._Wcpu = self.w[: s.F * s.KP].view(s.F, s.KP)[:, : s.K].contiguous()
        with warnings.catch_warnings():  # "sparse CSR support is in beta"
            warnings.simplefilter("ignore", UserWarning)
            csr = torch.sparse_csr_tensor(part.indptr, part.idx.long(), part.val.float(), size=(part.rows, s.F))
        z = (csr @ self._Wcpu) + s.intercept(self.w)
        self._finish_cpu(z, part.y, labels, out, counts)

    def _hist_cpu(self, z, yl, hist):
        """The kernels' table from the CPU path's own fp32 margins: the same formula
        (the other classes summed directly), the same clamp in float (NaN: bin 0)."""
        K = self.spec.K
        if K == 1:
            l = z[:, :1]
            side = (yl > 0).long().view(-1, 1)
            ok = torch.ones_like(yl, dtype=torch.bool)
        else:
            zm = z - z.max(1, keepdim=True).values
            e = torch.exp(zm)
            so = torch.stack([e[:, [j for j in range(K) if j != c]].sum(1) for c in range(K)], 1)
            l = zm - torch.log(so)
            side = (yl.view(-1, 1) == torch.arange(K).view(1, -1)).long()
            ok = (yl >= 0) & (yl < K)
        lo, hi = torch.tensor(-256.0), torch.tensor(255.0)
        b = M.HIST_BINS // 2 + torch.fmin(torch.fmax(torch.round(16.0 * l), lo), hi).long()
        cell = (torch.arange(K).view(1, -1) * M.HIST_SIDES + side) * M.HIST_BINS + b
        cell = cell[ok].reshape(-1)
        hist.index_add_(0, cell, torch.ones_like(cell, dtype=torch.int32))

    def _finish_cpu(self, z, y, labels, out, counts):
        pred, pr, nll, hist = out
        K = self.spec.K
        binary = K == 1
        if binary:
            z0 = z[:, 0]
            p = (z0 > 0).to(torch.int32)
            if pr is not None:
                pr.copy_(torch.stack([torch.sigmoid(-z0), torch.sigmoid(z0)], 1))
        else:
            p = z.argmax(1).to(torch.int32)  # the first maximum: the lowest class wins a tie
            if pr is not None:
                pr.copy_(torch.softmax(z, 1))
        pred.copy_(p)
        if not labels:
            return
        yl = y.long()
        if binary:
            yb = (yl > 0)
            nll.copy_(torch.nn.functional.softplus(z0) - yb.float() * z0)
            cl = yb.long()
        else:
            ok = (yl >= 0) & (yl < K)
            v = torch.logsumexp(z, 1) - z.gather(1, yl.clamp(0, K - 1).view(-1, 1)).view(-1)
            nll.copy_(torch.where(ok, v, torch.full_like(v, float("nan"))))
            counts[256] += int((~ok).sum())
            cl = yl.clamp(0, 15)
        counts[:256].index_add_(0, cl * 16 + p.long(), torch.ones_like(cl, dtype=torch.int32))
        if hist is not None:
            self._hist_cpu(z, yl, hist)


__all__ = ["Scorer", "ScoreResult"]

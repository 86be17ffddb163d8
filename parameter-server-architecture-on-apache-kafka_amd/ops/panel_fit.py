"""Fit and score the dense model on rows wider than 2,048 features: the panel family.

Multinomial LR on embedding rows of 3,072 .. 16,384 features, every entry non-zero, is
neither the dense model (:class:`psx.models.logreg.ModelSpec`, whose kernels keep a whole
32-row tile in LDS and stop at 2,048) nor the wide one (CSR rows: 4 B of index per 2 B of
value, and no MFMA tile).  A :class:`PanelSpec` covers ``2048 < F <= 16384``, padded to
``Fp`` in {4096, 8192, 16384}; the objective, the optimiser and the result are those of
:mod:`psx.ops.fit`.

GPU: ``csrc/kernels/panel_fit.hip`` driven by ``csrc/solver/panel_fit.hip`` (a missing
extension is a hard error).  The rows are processed in feature panels of 1,024 columns on a
2-D grid (row blocks x panels); one evaluation reads the rows twice.  CPU: the float64
reference (:func:`psx.models.reference.fit_reference`), as :class:`psx.ops.fit.BatchFitter`.

Row weights, ``fit_many`` / ``loss_grad_many``, ``cross_validate`` and the score histogram
(``curves=True``) are not implemented for this family.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import _native
from ..models.logreg import SUPPORTED_FP, ModelSpec
from ..models.reference import multinomial_loss_grad
from ..utils.data import Dataset
from ..utils.metrics import metrics_from_confusion
from .fit import BatchFitter, FitOptions
from .lr import is_gpu, stream_handle
from .score import ScoreResult, _row_order_sum

PANEL_FP = (4096, 8192, 16384)


@dataclass(frozen=True)
class PanelSpec:
    """The dense model at ``2048 < num_features <= 16384``; the members of ``ModelSpec``, with the
    same device layout (``[K][Fp]`` coefficients, then ``K`` intercepts)."""
    num_features: int
    num_classes: int

    def __post_init__(self):
        if self.num_features <= SUPPORTED_FP[-1]:
            raise ValueError(f"{self.num_features} features: up to {SUPPORTED_FP[-1]} the model is a ModelSpec, "
                             "fitted by BatchFitter")
        if self.num_features > PANEL_FP[-1]:
            raise ValueError(f"the panel model supports up to {PANEL_FP[-1]} features (got {self.num_features})")

    F = ModelSpec.F
    K = ModelSpec.K
    P = ModelSpec.P
    P_ref = ModelSpec.P_ref
    eval_classes = ModelSpec.eval_classes
    coef = ModelSpec.coef
    intercept = ModelSpec.intercept
    pack = ModelSpec.pack
    init = ModelSpec.init

    @property
    def Fp(self) -> int:
        return next(fp for fp in PANEL_FP if self.num_features <= fp)


@dataclass
class PanelDataset(Dataset):
    """``X`` [Npad, Fp] bf16 and ``y`` [Npad] int32 with ``Npad`` = ``n`` rounded up to 32: the
    kernels' container (padding rows and columns zero)."""
    n: int = 0

    @property
    def rows(self) -> int:
        return self.n

    def to(self, device) -> "PanelDataset":
        return PanelDataset(self.X.to(device), self.y.to(device), self.num_features, self.names, self.n)


def panel_dataset(x: torch.Tensor, y: torch.Tensor) -> PanelDataset:
    """``x`` [N, F] floats and ``y`` [N] labels -> the padded bf16 container."""
    if x.dim() != 2 or y.numel() != x.shape[0] or x.shape[0] < 1:
        raise ValueError(f"rows [N, F] and N labels are needed, got {tuple(x.shape)} and {tuple(y.shape)}")
    n, F = int(x.shape[0]), int(x.shape[1])
    Fp, npad = PanelSpec(F, 2).Fp, (n + 31) // 32 * 32
    X = torch.zeros(npad, Fp, dtype=torch.bfloat16, device=x.device)
    X[:n, :F] = x.to(torch.bfloat16)
    yp = torch.zeros(npad, dtype=torch.int32, device=x.device)
    yp[:n] = y.reshape(-1).to(x.device, torch.int32)
    return PanelDataset(X, yp, F, None, n)


def _check_spec(spec):
    if not isinstance(spec, PanelSpec):
        raise ValueError(f"the panel fit trains the panel model (PanelSpec), not {type(spec).__name__}")
    if not 2 <= spec.K <= 16:
        raise ValueError(f"{spec.K} classes: the panel model has 2..16")


def _check_rows(spec, ds, min_rows):
    if not isinstance(ds, PanelDataset):
        raise ValueError(f"the panel model ({spec.F} features, {spec.K} classes) takes a PanelDataset "
                         f"(panel_dataset(x, y)), got {type(ds).__name__}")
    if ds.num_features != spec.F or ds.Fp != spec.Fp:
        raise ValueError(f"the data is {ds.num_features} features wide (padded {ds.Fp}), the model "
                         f"{spec.F} (padded {spec.Fp})")
    if not min_rows <= ds.rows < (1 << 31) - 64:
        raise ValueError(f"{ds.rows} rows: {min_rows} .. 2^31 - 65 are needed")
    if ds.X.shape[0] != (ds.rows + 31) // 32 * 32 or ds.y.numel() != ds.X.shape[0]:
        raise ValueError(f"{ds.rows} rows must be padded to a multiple of 32, got {tuple(ds.X.shape)}")


def _check_data(spec, ds, min_rows):
    _check_rows(spec, ds, min_rows)
    lo, hi = int(ds.y[: ds.rows].min()), int(ds.y[: ds.rows].max())
    if lo < 0 or hi >= spec.K:
        raise ValueError(f"labels span [{lo}, {hi}], the model has classes [0, {spec.K})")


class _Resident:
    """The container on the device as the kernels read it."""

    def __init__(self, ds: PanelDataset, device):
        self.src, self.N, self.Npad = ds, ds.rows, int(ds.X.shape[0])
        self.wcache, self.applied = {}, None
        self.X = ds.X.to(device, torch.bfloat16).contiguous()
        self.y = ds.y.to(device, torch.int32).contiguous()


class PanelScorer:
    """``ds`` resident on ``device``, scored with any number of weight vectors."""

    def __init__(self, spec: PanelSpec, ds: PanelDataset, device, max_wg: int | None = None):
        _check_spec(spec)
        _check_rows(spec, ds, 1)
        self.spec, self.device = spec, torch.device(device)
        self.data = _Resident(ds, self.device)
        self._native = None
        if is_gpu(self.device):
            with torch.cuda.device(self.device):
                self._native = _native.hip().PanelBatchFitter(spec.K, spec.F, spec.Fp, 1, max_wg or 0)
                self._native.set_data(self.data.X.data_ptr(), self.data.y.data_ptr(), self.data.N, self.data.Npad,
                                      False, stream_handle(self.device))

    def score(self, w: torch.Tensor, proba: bool = False, curves: bool = False) -> ScoreResult:
        if curves:
            raise NotImplementedError("the panel scorer has no score histogram (curves=True)")
        s, d, dev = self.spec, self.data, self.device
        if w.numel() != s.P:
            raise ValueError(f"the model has {s.P} weights in device layout, got {w.numel()}")
        T, K = d.N, s.K
        if self._native is None:  # float64 margins of the bf16 rows
            wc = w.detach().double().cpu().reshape(-1)
            z = d.X[:T, : s.F].double() @ s.coef(wc).t() + s.intercept(wc)
            yl = d.y[:T].long()
            ok = (yl >= 0) & (yl < K)
            pred = z.argmax(1).to(torch.int32)
            pr = torch.softmax(z, 1).float() if proba else None
            v = torch.logsumexp(z, 1) - z.gather(1, yl.clamp(0, K - 1).view(-1, 1)).view(-1)
            nll = torch.where(ok, v, torch.full_like(v, float("nan"))).float()
            counts = torch.zeros(257, dtype=torch.int32)
            counts[:256].index_add_(0, yl.clamp(0, 15) * 16 + pred.long(), torch.ones(T, dtype=torch.int32))
            counts[256] = int((~ok).sum())
        else:
            with torch.cuda.device(dev):
                wd = w.detach().to(dev, torch.float32).reshape(-1).contiguous()
                pred = torch.empty(T, dtype=torch.int32, device=dev)
                pr = torch.empty(T, K, dtype=torch.float32, device=dev) if proba else None
                nll = torch.empty(T, dtype=torch.float32, device=dev)
                counts = torch.zeros(257, dtype=torch.int32, device=dev)
                self._native.score(wd.data_ptr(), pred.data_ptr(), pr.data_ptr() if proba else 0, nll.data_ptr(),
                                   counts.data_ptr(), counts.data_ptr() + 1024, stream_handle(dev))
        host = counts.cpu()
        conf = host[:256].view(16, 16)[:K, :K].to(torch.int64).clone()
        v = nll.cpu().numpy().astype(np.float64)
        v = v[np.isfinite(v)]
        f1, acc = metrics_from_confusion(conf.numpy())
        return ScoreResult(pred, pr, nll, conf, T, int(host[256]), _row_order_sum(v) / v.size if v.size else None,
                           f1, acc)


def panel_score(spec: PanelSpec, w: torch.Tensor, ds: PanelDataset, device, proba: bool = False,
                curves: bool = False) -> ScoreResult:
    """Predictions, per-row loss, probabilities, confusion, log-loss and accuracy of ``w`` on ``ds``."""
    return PanelScorer(spec, ds, device).score(w, proba, curves)


class PanelFitter(BatchFitter):
    """Full-batch L-BFGS trainer of one panel model on one device: :class:`BatchFitter`'s
    ``fit`` / ``loss_grad`` and its :class:`FitResult`, on the panel kernels."""

    _check_spec = staticmethod(_check_spec)
    _check_data = staticmethod(_check_data)

    def _new_native(self, hip):
        s = self.spec
        return hip.PanelBatchFitter(s.K, s.F, s.Fp, self.opts.hist, self.opts.max_wg or 0)

    def _load(self, ds):
        data = _Resident(ds, self.device)
        self._native.set_data(data.X.data_ptr(), data.y.data_ptr(), data.N, data.Npad, True,
                              stream_handle(self.device))
        self._data = data  # the native fitter reads these buffers until the next set_data
        return data

    def _rows64(self, ds):
        return ds.X[: ds.rows, : self.spec.F].to(torch.bfloat16).double().cpu(), ds.y[: ds.rows].long().cpu()

    def _loss_grad_cpu(self, ds, w, resident):
        s = self.spec
        X, y = self._rows64(ds)
        wc = w.detach().double().cpu()
        loss, gc, gb = multinomial_loss_grad(X, y, s.coef(wc), s.intercept(wc))
        return float(loss), s.pack(gc, gb, device=self.device)

    def _validator(self, valid):
        sc = PanelScorer(self.spec, valid, self.device)
        return lambda w: float(sc.score(w).log_loss)

    def fit(self, train, w0=None, valid=None, valid_every: int = 1, patience=None, weights=None):
        if weights is not None:
            raise NotImplementedError("row weights are not implemented for the panel model")
        return super().fit(train, w0, valid, valid_every, patience)

    def loss_grad(self, ds, w, weights=None):
        if weights is not None:
            raise NotImplementedError("row weights are not implemented for the panel model")
        return super().loss_grad(ds, w)

    def _unsupported(self, *a, **k):
        raise NotImplementedError("batched fits and held-out folds are not implemented for the panel model")

    fit_many = loss_grad_many = holdout_loss = _unsupported


__all__ = ["PANEL_FP", "PanelDataset", "PanelFitter", "PanelScorer", "PanelSpec", "panel_dataset", "panel_score",
           "FitOptions"]

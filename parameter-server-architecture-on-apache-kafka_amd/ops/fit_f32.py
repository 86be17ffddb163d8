"""Fit and score the dense model on fp32 rows: the fp32-row family (padded widths up to 1,024).

:class:`psx.ops.fit.BatchFitter` and :class:`psx.ops.score.Scorer` round every row to bf16
when they load it.  The fit standardises by sigma and does not centre, so a feature whose
variation is small next to its magnitude (a price, a timestamp, a counter at 100 +- 1) loses
most of its information in bf16's 8-bit mantissa before the optimiser sees it.
:class:`F32Fitter` / :class:`F32Scorer` take a :class:`psx.utils.data.Dataset` whose ``X`` is
``torch.float32 [N, Fp]`` and keep it in fp32; the model is the ordinary
:class:`psx.models.logreg.ModelSpec` with ``Fp <= 1024`` (the streaming solver's limit for
fp32 rows), and the objective, the optimiser, the result and the checkpoint are those of
:mod:`psx.ops.fit`.  Any other dtype is an error -- no silent rounding in either direction.

GPU: ``csrc/kernels/fit_f32.hip`` driven by ``csrc/solver/fit_f32.hip`` (a missing extension
is a hard error): a tile is read once and staged as two bf16 images, hi and lo, and every
product runs on the bf16 MFMA against operands split the same way; the statistics widen each
element to double.  CPU: the float64 reference on the fp32 rows as stored
(:func:`psx.models.reference.fit_reference`, ``multinomial_loss_grad``).

Centred mode (``F32Fitter(..., center=True)``, ``F32Scorer(..., center=c)``; off by default).  The
fit standardises by sigma and does not centre, so a column at mean / sigma = m gives a Hessian whose
condition number grows like m^2: at 100 +- 1 the relative-decrease test stops the optimiser hundreds
of iterations early, in float64 as on the GPU, and the trial weights' 16 bits turn into intercept
shifts the line search cannot resolve.  With ``center=True`` every kernel multiplies ``x - c_f`` (``c``
the columns' fp32 means from the statistics pass, a constant column's own value) and the optimiser
runs in ``(beta, b')``, ``b' = b + sum_f c_f w_f``.  The intercept is free and unpenalised, so this is
a reparametrisation: the objective and its minimum are the same, and ``fit`` / ``loss_grad`` / ``score``
keep taking and returning RAW ``(w, b)``, valid for every scorer.  ``FitResult.center`` is the centre.
CPU: the float64 reference on ``X - c``, intercepts mapped back.

Not implemented for this family (``NotImplementedError``): row weights (``weights=``),
``fit_many`` / ``loss_grad_many`` / ``holdout_loss``, ``cross_validate`` and the score
histogram (``curves=True``).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from ..models.logreg import ModelSpec
from ..models.reference import multinomial_loss_grad
from ..utils.data import Dataset
from ..utils.metrics import metrics_from_confusion
from . import fit as _fit
from .fit import BatchFitter, FitOptions
from .lr import is_gpu, stream_handle
from .score import ScoreResult, _row_order_sum

F32_MAX_FP = 1024


def _check_spec(spec):
    _fit._check_spec(spec)
    if spec.Fp > F32_MAX_FP:
        raise ValueError(f"fp32 rows are supported up to a padded width of {F32_MAX_FP} (two tile images of wider "
                         f"rows do not fit the LDS), got {spec.F} features (padded {spec.Fp})")


def _check_rows(spec, ds, min_rows):
    if not isinstance(ds, Dataset):
        raise ValueError(f"the dense model ({spec.F} features, {spec.K} classes) fits dense rows (Dataset), "
                         f"got {type(ds).__name__}")
    if ds.X.dtype != torch.float32:
        raise ValueError(f"the fp32-row family takes float32 rows, got {ds.X.dtype}: bf16 rows are BatchFitter's "
                         "and Scorer's (Dataset.as_dtype converts explicitly)")
    if ds.num_features != spec.F or ds.Fp != spec.Fp:
        raise ValueError(f"the data is {ds.num_features} features wide (padded {ds.Fp}), the model "
                         f"{spec.F} (padded {spec.Fp})")
    if not min_rows <= ds.rows < (1 << 31) - 64:
        raise ValueError(f"{ds.rows} rows: {min_rows} .. 2^31 - 65 are needed")


def _check_data(spec, ds, min_rows):
    _check_rows(spec, ds, min_rows)
    lo, hi = int(ds.y.min()), int(ds.y.max())
    if lo < 0 or hi >= spec.K:
        raise ValueError(f"labels span [{lo}, {hi}], the model has classes [0, {spec.K})")


def _center_of(X32):
    """The fp32 centre [F] of the rows ``X32`` [N, F] as the statistics pass forms it: the float64 mean rounded
    to fp32, a constant column's value itself."""
    X = X32.double().cpu()
    const = X.max(0).values == X.min(0).values
    return torch.where(const, X[0], X.mean(0)).float()


def _check_center(spec, center):
    if not isinstance(center, torch.Tensor) or center.dtype != torch.float32 or center.numel() != spec.F:
        raise ValueError(f"the centre is a float32 tensor of the model's {spec.F} features, got "
                         f"{tuple(center.shape) if isinstance(center, torch.Tensor) else type(center).__name__}"
                         f"{' ' + str(center.dtype) if isinstance(center, torch.Tensor) else ''}")
    return center.detach().reshape(-1)


class _Resident:
    """fp32 rows and int32 labels on the device, padded with zero rows to a multiple of 32."""

    def __init__(self, ds: Dataset, device):
        self.src = ds
        n = ds.rows
        npad = (n + 31) // 32 * 32
        self.N, self.Npad = n, npad
        self.wcache, self.applied = {}, None
        if (npad == n and ds.X.device == device and ds.X.is_contiguous()
                and ds.y.device == device and ds.y.dtype == torch.int32 and ds.y.is_contiguous()):
            self.X, self.y = ds.X, ds.y  # already resident in the kernels' layout: no second copy
            return
        self.X = torch.zeros(npad, ds.Fp, dtype=torch.float32, device=device)
        self.X[:n] = ds.X.to(device)
        self.y = torch.zeros(npad, dtype=torch.int32, device=device)
        self.y[:n] = ds.y.to(device, torch.int32)


class F32Scorer:
    """``ds`` (fp32 rows, labels required) resident on ``device``, scored with any number of weight vectors.

    ``center`` (float32 ``[F]``, a fit's ``FitResult.center``): the kernel stages ``x - c`` and adds
    ``sum_f c_f w_f`` to the intercepts; the weights passed to ``score`` stay raw.  The CPU path computes
    float64 margins, where the two are the same number."""

    def __init__(self, spec: ModelSpec, ds: Dataset, device, max_wg: int | None = None, center=None):
        _check_spec(spec)
        _check_rows(spec, ds, 1)
        if center is not None:
            center = _check_center(spec, center)
        self.spec, self.device = spec, torch.device(device)
        self._native = None
        if is_gpu(self.device):
            self.data = _Resident(ds, self.device)
            with torch.cuda.device(self.device):
                st = stream_handle(self.device)
                self._native = _native.hip().F32BatchFitter(spec.K, spec.F, spec.Fp, 1, max_wg or 0, center is not None)
                self._native.set_data(self.data.X.data_ptr(), self.data.y.data_ptr(), self.data.N, self.data.Npad,
                                      False, st)
                if center is not None:
                    c = torch.zeros(spec.Fp, dtype=torch.float32, device=self.device)
                    c[: spec.F] = center.to(self.device)
                    self._native.set_center(c.data_ptr(), st)  # (copied)
        else:
            self.data = ds

    def score(self, w: torch.Tensor, proba: bool = False, curves: bool = False) -> ScoreResult:
        if curves:
            raise NotImplementedError("the fp32-row scorer has no score histogram (curves=True)")
        s, d, dev = self.spec, self.data, self.device
        if w.numel() != s.P:
            raise ValueError(f"the model has {s.P} weights in device layout, got {w.numel()}")
        K = s.K
        if self._native is None:  # float64 margins of the fp32 rows as stored
            T = d.rows
            wc = w.detach().double().cpu().reshape(-1)
            z = d.X[:, : s.F].double().cpu() @ s.coef(wc).t() + s.intercept(wc)
            yl = d.y.long().cpu()
            ok = (yl >= 0) & (yl < K)
            pred = z.argmax(1).to(torch.int32)
            pr = torch.softmax(z, 1).float() if proba else None
            v = torch.logsumexp(z, 1) - z.gather(1, yl.clamp(0, K - 1).view(-1, 1)).view(-1)
            nll = torch.where(ok, v, torch.full_like(v, float("nan"))).float()
            counts = torch.zeros(257, dtype=torch.int32)
            counts[:256].index_add_(0, yl.clamp(0, 15) * 16 + pred.long(), torch.ones(T, dtype=torch.int32))
            counts[256] = int((~ok).sum())
        else:
            T = d.N
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


def f32_score(spec: ModelSpec, w: torch.Tensor, ds: Dataset, device, proba: bool = False,
              curves: bool = False, center=None) -> ScoreResult:
    """Predictions, per-row loss, probabilities, confusion, log-loss and accuracy of ``w`` on the fp32 rows ``ds``."""
    return F32Scorer(spec, ds, device, center=center).score(w, proba, curves)


class F32Fitter(BatchFitter):
    """Full-batch L-BFGS trainer of one dense model on fp32 rows: :class:`BatchFitter`'s ``fit`` /
    ``loss_grad`` and its :class:`FitResult` (``save`` writes the ordinary dense checkpoint), on the
    two-image kernels.  ``center=True``: the centred mode of the module docstring."""

    _check_spec = staticmethod(_check_spec)
    _check_data = staticmethod(_check_data)
    _shift = None  # float64 [F]: the centre of the centred CPU fit in progress

    def __init__(self, spec, device, opts: FitOptions | None = None, center: bool = False):
        self.center = bool(center)
        super().__init__(spec, device, opts)

    def _new_native(self, hip):
        s = self.spec
        return hip.F32BatchFitter(s.K, s.F, s.Fp, self.opts.hist, self.opts.max_wg or 0, self.center)

    def _load(self, ds):
        data = _Resident(ds, self.device)
        self._native.set_data(data.X.data_ptr(), data.y.data_ptr(), data.N, data.Npad, True,
                              stream_handle(self.device))
        self._data = data  # the native fitter reads these buffers until the next set_data
        return data

    def _rows64(self, ds):
        X = ds.X[:, : self.spec.F].double().cpu()
        return (X if self._shift is None else X - self._shift), ds.y.long().cpu()

    def _train_center(self, padded=False):
        """The centre [F] of the rows the fitter holds (None with the mode off); padded: [Fp], the kernels' vector."""
        if not self.center:
            return None
        if self._native is None:
            return self._shift.float()
        c = torch.empty(self.spec.Fp, dtype=torch.float32, device=self.device)
        self._native.read_center(c.data_ptr(), stream_handle(self.device))
        return c if padded else c[: self.spec.F].clone()

    def _move_intercepts(self, w, c, sign):
        """``(w, b + sign * W c)`` in float64, packed; back to raw (sign -1) the intercepts are centred again."""
        s = self.spec
        wc = w.detach().double().cpu().reshape(-1)
        b = s.intercept(wc) + sign * (s.coef(wc) @ c.double().cpu())
        return s.pack(s.coef(wc), b - b.mean() if sign < 0 else b, device=self.device)

    def _fit_cpu(self, train, w0, valid, valid_every, patience):
        if not self.center:
            return super()._fit_cpu(train, w0, valid, valid_every, patience)
        c = _center_of(train.X[:, : self.spec.F])
        self._shift = c.double()  # _rows64 hands the reference X - c; the validator maps its iterates back
        try:
            res = super()._fit_cpu(train, None if w0 is None else self._move_intercepts(w0, c, +1), valid, valid_every,
                                   patience)
        finally:
            self._shift = None
        res.w, res.center = self._move_intercepts(res.w, c, -1), c.to(self.device)
        return res

    def loss_grad_centred(self, ds, w):
        """``(loss, gradient with respect to (w, b'), centre)`` at the raw weights ``w``: the evaluation the
        centred optimiser sees; the centre is ``[Fp]`` like a row of the gradient, zero in the padding.
        ``loss_grad`` returns the gradient with respect to raw ``(w, b)``."""
        s = self.spec
        if not self.center:
            raise ValueError("loss_grad_centred needs F32Fitter(..., center=True)")
        self._check_data(s, ds, 1)
        if w.numel() != s.P:
            raise ValueError(f"the model has {s.P} weights in device layout, got {w.numel()}")
        if self._native is None:
            c = _center_of(ds.X[:, : s.F])
            wc = self._move_intercepts(w, c, +1).double().cpu()
            X, y = self._rows64(ds)
            loss, gc, gb = multinomial_loss_grad(X - c.double(), y, s.coef(wc), s.intercept(wc))
            return float(loss), s.pack(gc, gb, device=self.device), torch.nn.functional.pad(c, (0, s.Fp - s.F))
        with torch.cuda.device(self.device):
            if self._data is None or self._data.src is not ds:
                self._load(ds)
            wd = w.detach().to(self.device, torch.float32).reshape(-1).contiguous()
            g = torch.empty(s.P, dtype=torch.float32, device=self.device)
            loss = self._native.loss_grad_centred(wd.data_ptr(), g.data_ptr(), stream_handle(self.device))
            return float(loss), g, self._train_center(padded=True)

    def _loss_grad_cpu(self, ds, w, resident):
        s = self.spec
        X, y = self._rows64(ds)
        wc = w.detach().double().cpu()
        loss, gc, gb = multinomial_loss_grad(X, y, s.coef(wc), s.intercept(wc))
        return float(loss), s.pack(gc, gb, device=self.device)

    def _validator(self, valid):
        sc = F32Scorer(self.spec, valid, self.device, center=self._train_center())  # the TRAINING set's centre
        if self._shift is None:
            return lambda w: float(sc.score(w).log_loss)
        c = self._shift
        return lambda w: float(sc.score(self._move_intercepts(w, c, -1)).log_loss)

    def fit(self, train, w0=None, valid=None, valid_every: int = 1, patience=None, weights=None):
        if weights is not None:
            raise NotImplementedError("row weights are not implemented for fp32 rows")
        res = super().fit(train, w0, valid, valid_every, patience)
        if self.center and self._native is not None:
            with torch.cuda.device(self.device):
                res.center = self._train_center()
        return res

    def loss_grad(self, ds, w, weights=None):
        if weights is not None:
            raise NotImplementedError("row weights are not implemented for fp32 rows")
        return super().loss_grad(ds, w)

    def _unsupported(self, *a, **k):
        raise NotImplementedError("batched fits, held-out folds and cross_validate are not implemented for fp32 rows")

    fit_many = loss_grad_many = holdout_loss = cross_validate = _unsupported


__all__ = ["F32_MAX_FP", "F32Fitter", "F32Scorer", "f32_score", "FitOptions"]

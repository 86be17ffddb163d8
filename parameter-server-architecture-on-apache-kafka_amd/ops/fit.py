"""Fit the dense model to a dataset until the optimiser converges, optionally with
an L2 penalty -- the offline ground truth of BASELINE.md, on the GPU.

The objective is Spark's ``LogisticRegression.fit`` with ``standardization=true``,
``elasticNetParam=0``: features are scaled by 1/sigma (sample std, not centred; a
constant feature is excluded and gets coefficient 0), ``beta = coef * sigma`` and

    f(beta, b) = mean cross entropy + 0.5 * reg_param * sum(beta^2)

with unpenalised intercepts, minimised by the project's L-BFGS (history 10, strong
Wolfe c1 = 1e-4 / c2 = 0.9, first step 1/||g||, growth x1.5, cubic zoom, the stopping
tests of ``ctrl_accept``).  Intercepts are always centred over the classes;
coefficients only when ``reg_param == 0`` (a penalised optimum is centred by itself).

GPU: every per-row number comes from ``csrc/kernels/fit_kernels.hip`` driven by
``csrc/solver/fit.hip`` (a missing extension is a hard error); the whole dataset is
resident in HBM as bf16 rows.  CPU: :func:`psx.models.reference.fit_reference`.

fp32 rows are converted to bf16, as :class:`psx.ops.score.Scorer` does: the fit sees
the rounded features.

``FitResult.save`` writes a ``server.ckpt`` that ``Scorer.from_checkpoint`` and
``python -m psx.apps.predict`` read.  Resuming a STREAMING run from a fitted
checkpoint is out of scope: ``restore_server`` wants the tracker state a fit does
not have.
"""
from __future__ import annotations

import os
import statistics
import time
from dataclasses import asdict, dataclass, field

import torch

from .. import _native
from ..models.logreg import ModelSpec, to_reference_layout
from ..models.reference import fit_reference
from ..models.wide import WideSpec
from ..utils.checkpoint import CKPT_NAME, FORMAT, _atomic_save
from ..utils.data import Dataset
from .lr import is_gpu, stream_handle


@dataclass
class FitOptions:
    max_iter: int = 100
    tol: float = 1e-6
    reg_param: float = 0.0
    hist: int = 10
    ls_max: int = 20
    zero_const: bool = True
    max_wg: int | None = None  # workgroups of one evaluation (default: two per compute unit)


@dataclass
class FitResult:
    spec: ModelSpec
    w: torch.Tensor  # [P] fp32, device layout, on the fitter's device
    objective: float
    log_loss: float  # the unregularised part of ``objective``
    history: list  # objective at the start and after every accepted iteration
    iters: int
    evals: int
    reason: str  # tol | max_iter | line_search | no_descent | early_stop
    std: torch.Tensor  # [F] feature sigma (0: excluded)
    seconds: float
    pass_seconds: float  # median evaluation
    options: FitOptions = field(default_factory=FitOptions)
    valid_history: list = field(default_factory=list)  # (accepted iterations, validation log-loss)
    best_iter: int | None = None  # the iterate ``w`` holds when a validation set chose it
    ls_fail: int = 0  # line searches that spent their budget (settled for sufficient decrease, or ended the fit)
    # a wide fit (psx/ops/wide_fit.py): ``spec`` is a WideSpec, ``features`` int32 [U] the sorted features the
    # training set touches and ``std`` their [U] sigmas (every other feature is excluded: sigma 0, coefficient 0)
    features: torch.Tensor | None = None

    def save(self, path_dir: str) -> str:
        """Write ``server.ckpt`` into ``path_dir`` (for ``Scorer.from_checkpoint`` /
        ``psx.apps.predict``; not a resumable streaming checkpoint)."""
        os.makedirs(path_dir, exist_ok=True)
        w = self.w.detach().float().cpu().clone()
        fit = {k: (v if v is not None else -1) for k, v in asdict(self.options).items()}
        fit.update(objective=float(self.objective), log_loss=float(self.log_loss), iters=int(self.iters),
                   evals=int(self.evals), ls_fail=int(self.ls_fail), reason=str(self.reason),
                   seconds=float(self.seconds), history=[float(v) for v in self.history])
        state = {"format": FORMAT, "model": "dense", "num_features": int(self.spec.F),
                 "num_classes": int(self.spec.K), "w": w, "fit": fit}
        if isinstance(self.spec, WideSpec):  # the wide layout is the reference's own flat order: no second copy
            state["model"] = "wide"
        else:
            state["w_reference_layout"] = to_reference_layout(self.spec, w)
        return _atomic_save(state, os.path.join(path_dir, CKPT_NAME))


def _check_options(o: FitOptions):
    if not o.reg_param >= 0:
        raise ValueError(f"reg_param must be >= 0, got {o.reg_param}")
    if o.max_iter < 0 or o.ls_max < 1 or not o.tol >= 0:
        raise ValueError(f"max_iter >= 0, ls_max >= 1 and tol >= 0 are needed, got {o.max_iter}, {o.ls_max}, {o.tol}")
    if not 1 <= o.hist <= 16:
        raise ValueError(f"hist must be in [1, 16], got {o.hist}")
    if o.max_wg is not None and o.max_wg < 1:
        raise ValueError(f"max_wg must be >= 1, got {o.max_wg}")


def _check_spec(spec):
    if not isinstance(spec, ModelSpec):
        raise ValueError(f"the full-batch fit trains the dense model (ModelSpec), not {type(spec).__name__}")
    if not 2 <= spec.K <= 16:
        raise ValueError(f"{spec.K} classes: the dense model has 2..16")


def _check_data(spec: ModelSpec, ds, min_rows: int):
    if not isinstance(ds, Dataset):
        raise ValueError(f"the dense model ({spec.F} features, {spec.K} classes) fits dense rows (Dataset), "
                         f"got {type(ds).__name__}")
    if ds.num_features != spec.F or ds.Fp != spec.Fp:
        raise ValueError(f"the data is {ds.num_features} features wide (padded {ds.Fp}), the model "
                         f"{spec.F} (padded {spec.Fp})")
    if ds.rows < min_rows:
        raise ValueError(f"{ds.rows} rows: at least {min_rows} needed")
    if ds.rows >= (1 << 31) - 64:
        raise ValueError(f"{ds.rows} rows: at most 2^31 - 65")
    lo, hi = int(ds.y.min()), int(ds.y.max())
    if lo < 0 or hi >= spec.K:
        raise ValueError(f"labels span [{lo}, {hi}], the model has classes [0, {spec.K})")


def _run_native(nat, st, w, check, valid_every, patience):
    """Drive a native fitter (begun) to its end, finalising the iterate into ``w``;
    with ``check`` the iterate is scored every ``valid_every`` accepted iterations.
    -> (best, validation history, ``early_stop`` or None); best = (validation
    log-loss, accepted iterations, weights, objective, log-loss) or None."""
    best, vhist, bad = None, [], 0
    while True:
        ended = nat.run(valid_every if check else (1 << 30), st)
        nat.current(w.data_ptr(), st)
        if check:
            v = check(w)
            vhist.append((int(nat.accepted), v))
            if best is None or v < best[0]:
                best, bad = (v, int(nat.accepted), w.clone(), float(nat.objective), float(nat.log_loss)), 0
            else:
                bad += 1
                if patience is not None and bad >= patience and not ended:
                    return best, vhist, "early_stop"
        if ended:
            return best, vhist, None


def _validate_oracle(res, ref, run, pack, check, valid_every, patience):
    """Validation of a CPU fit.  The oracle is deterministic: its iterate after i
    accepted iterations is the fit capped at i (``run(i)``)."""
    best, bad = None, 0
    marks = list(range(valid_every, ref.iters, valid_every)) + [ref.iters]
    for i in marks:
        r = ref if i == ref.iters else run(i)
        w = pack(r)
        v = check(w)
        res.valid_history.append((i, v))
        if best is None or v < best[0]:
            best, bad = (v, i, w, r.objective, r.log_loss), 0
        else:
            bad += 1
            if patience is not None and bad >= patience and i != ref.iters:
                res.reason = "early_stop"
                res.iters, res.history = i, list(ref.history[: i + 1])
                break
    res.w, res.best_iter, res.objective, res.log_loss = best[2], best[1], best[3], best[4]


class _Resident:
    """bf16 rows and int32 labels on the device, padded with zero rows to a multiple of 32."""

    def __init__(self, ds: Dataset, device):
        self.src = ds
        n = ds.rows
        npad = (n + 31) // 32 * 32
        self.N, self.Npad = n, npad
        if (npad == n and ds.X.device == device and ds.X.dtype == torch.bfloat16 and ds.X.is_contiguous()
                and ds.y.device == device and ds.y.dtype == torch.int32 and ds.y.is_contiguous()):
            self.X, self.y = ds.X, ds.y  # already resident in the kernels' layout: no second copy
            return
        self.X = torch.zeros(npad, ds.Fp, dtype=torch.bfloat16, device=device)
        self.X[:n] = ds.X.to(device, torch.bfloat16)
        self.y = torch.zeros(npad, dtype=torch.int32, device=device)
        self.y[:n] = ds.y.to(device, torch.int32)


class _FitterBase:
    """What the dense and the wide trainer share: one native fitter per object, the
    resident dataset, :meth:`fit`, :meth:`loss_grad` and the GPU path of both.  A
    subclass supplies ``_check_spec`` / ``_check_data``, ``_new_native``, ``_load``,
    ``_result_vector``, ``_std_features`` and its CPU paths (``_fit_cpu``,
    ``_loss_grad_cpu``)."""

    def __init__(self, spec, device, opts: FitOptions | None = None):
        self._check_spec(spec)
        self.spec = spec
        self.device = torch.device(device)
        self.opts = opts or FitOptions()
        _check_options(self.opts)
        self._native = None
        if is_gpu(self.device):
            with torch.cuda.device(self.device):
                self._native = self._new_native(_native.hip())
        self._data = None

    # ---- one evaluation ------------------------------------------------------
    def loss_grad(self, ds, w: torch.Tensor):
        """Mean loss of ``w`` (device layout ``[P]``) over ``ds`` and its gradient in
        the same layout (zero for every feature a sparse ``ds`` does not touch):
        original feature space, no standardisation, no penalty.  Calls in a row with
        the same ``ds`` object reuse its resident copy (and skip the checks): do not
        change its tensors in between."""
        s = self.spec
        resident = self._data is not None and self._data.src is ds
        if not resident:
            self._check_data(s, ds, 1)
        if w.numel() != s.P:
            raise ValueError(f"the model has {s.P} weights in device layout, got {w.numel()}")
        if self._native is None:
            return self._loss_grad_cpu(ds, w, resident)
        with torch.cuda.device(self.device):
            if not resident:
                self._load(ds)
            wd = w.detach().to(self.device, torch.float32).reshape(-1).contiguous()
            g = torch.empty(s.P, dtype=torch.float32, device=self.device)
            loss = self._native.loss_grad(wd.data_ptr(), g.data_ptr(), stream_handle(self.device))
        return float(loss), g

    # ---- the fit ---------------------------------------------------------------
    def fit(self, train, w0: torch.Tensor | None = None, valid=None, valid_every: int = 1,
            patience: int | None = None) -> FitResult:
        """Fit ``train`` from zeros or from ``w0`` (device layout, a warm start).

        With ``valid`` the current iterate is scored with :class:`Scorer` every
        ``valid_every`` accepted iterations; the result carries the iterate with the
        lowest validation log-loss, and ``patience`` checks in a row without
        improvement end the fit with reason ``early_stop``."""
        s = self.spec
        self._check_data(s, train, 2)
        if valid is not None:
            self._check_data(s, valid, 1)
            if valid_every < 1 or (patience is not None and patience < 1):
                raise ValueError("valid_every and patience must be >= 1")
        if w0 is not None and w0.numel() != s.P:
            raise ValueError(f"the model has {s.P} weights in device layout, got {w0.numel()}")
        t0 = time.perf_counter()
        if self._native is None:
            res = self._fit_cpu(train, w0, valid, valid_every, patience)
        else:
            with torch.cuda.device(self.device):
                res = self._fit_gpu(train, w0, valid, valid_every, patience)
        res.seconds = time.perf_counter() - t0
        return res

    def _validator(self, valid):
        from .score import Scorer

        vds = valid.to(self.device)

        def check(w):
            return float(Scorer(self.spec, w, self.device).score(vds).log_loss)

        return check

    def _fit_gpu(self, train, w0, valid, valid_every, patience) -> FitResult:
        s, o, nat, dev = self.spec, self.opts, self._native, self.device
        st = stream_handle(dev)
        data = self._load(train)
        w0d = None
        if w0 is not None:
            w0d = w0.detach().to(dev, torch.float32).reshape(-1).contiguous()
        nat.begin(w0d.data_ptr() if w0d is not None else 0, int(o.max_iter), float(o.tol), float(o.reg_param),
                  int(o.ls_max), bool(o.zero_const), st)
        w = self._result_vector(w0)
        check = self._validator(valid) if valid is not None else None
        best, vhist, reason = _run_native(nat, st, w, check, valid_every, patience)
        std, features = self._std_features(data, st)
        ev = list(nat.eval_seconds)
        res = FitResult(spec=s, w=w, objective=float(nat.objective), log_loss=float(nat.log_loss),
                        history=list(nat.history), iters=int(nat.accepted), evals=int(nat.evals),
                        reason=reason or str(nat.reason), std=std, seconds=0.0,
                        pass_seconds=statistics.median(ev) if ev else 0.0, options=o, valid_history=vhist,
                        ls_fail=int(nat.ls_fail), features=features)
        if best is not None:
            res.w, res.best_iter, res.objective, res.log_loss = best[2], best[1], best[3], best[4]
        return res


class BatchFitter(_FitterBase):
    """Full-batch L-BFGS trainer of one dense model on one device.

    ``fit`` may be called any number of times (each call loads its dataset); no
    state of one fit reaches the next."""

    _check_spec = staticmethod(_check_spec)
    _check_data = staticmethod(_check_data)

    def _new_native(self, hip):
        s = self.spec
        return hip.BatchFitter(s.K, s.F, s.Fp, self.opts.hist, self.opts.max_wg or 0)

    def _load(self, ds: Dataset) -> _Resident:
        data = _Resident(ds, self.device)
        self._native.set_data(data.X.data_ptr(), data.y.data_ptr(), data.N, data.Npad, stream_handle(self.device))
        self._data = data  # the native fitter reads these buffers until the next set_data
        return data

    def _result_vector(self, w0):
        return torch.empty(self.spec.P, dtype=torch.float32, device=self.device)  # finalize writes all of it

    def _std_features(self, data, st):
        std = torch.empty(self.spec.Fp, dtype=torch.float32, device=self.device)
        self._native.read_std(std.data_ptr(), st)
        return std[: self.spec.F].clone(), None

    def _loss_grad_cpu(self, ds, w, resident):
        from ..models.reference import multinomial_loss_grad

        s = self.spec
        X = ds.X[:, : s.F].to(torch.bfloat16).double().cpu()
        wc = w.detach().double().cpu()
        loss, gc, gb = multinomial_loss_grad(X, ds.y.long().cpu(), s.coef(wc), s.intercept(wc))
        return float(loss), s.pack(gc, gb, device=self.device)

    def _fit_cpu(self, train, w0, valid, valid_every, patience) -> FitResult:
        s, o = self.spec, self.opts
        X = train.X[:, : s.F].to(torch.bfloat16).double().cpu()
        y = train.y.long().cpu()
        c0 = b0 = None
        if w0 is not None:
            wc = w0.detach().float().cpu().reshape(-1)
            c0, b0 = s.coef(wc).double(), s.intercept(wc).double()

        def run(max_iter):
            return fit_reference(X, y, c0, b0, num_classes=s.K, reg_param=o.reg_param, max_iter=max_iter, tol=o.tol,
                                 hist=o.hist, ls_max=o.ls_max, zero_const=o.zero_const)

        t0 = time.perf_counter()
        ref = run(o.max_iter)
        dt = time.perf_counter() - t0
        res = FitResult(spec=s, w=s.pack(ref.coef, ref.intercept, device=self.device), objective=ref.objective,
                        log_loss=ref.log_loss, history=list(ref.history), iters=ref.iters, evals=ref.evals,
                        reason=ref.reason, std=ref.std.float(), seconds=0.0, pass_seconds=dt / max(1, ref.evals),
                        options=o, ls_fail=ref.ls_fail)
        if valid is not None:
            _validate_oracle(res, ref, run, lambda r: s.pack(r.coef, r.intercept, device=self.device),
                             self._validator(valid), valid_every, patience)
        return res


def loss_grad(spec: ModelSpec, ds: Dataset, w: torch.Tensor, device, max_wg: int | None = None):
    """One evaluation: ``(mean cross entropy, gradient [P] in device layout)`` of
    ``w`` over ``ds`` in the original feature space -- no standardisation, no penalty."""
    return BatchFitter(spec, device, FitOptions(max_wg=max_wg)).loss_grad(ds, w)


__all__ = ["BatchFitter", "FitOptions", "FitResult", "loss_grad"]

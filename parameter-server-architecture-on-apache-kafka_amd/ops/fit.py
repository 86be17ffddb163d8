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

Row weights and a held-out fold (:class:`FitWeights`, ``weights=`` of
:meth:`BatchFitter.fit` / :meth:`BatchFitter.loss_grad`): with ``u_i = sample_weight_i *
class_weight[y_i]`` and ``train = {i : fold_i != holdout}`` the mean cross entropy
becomes ``(1/W) sum_train u_i CE_i``, ``W = sum_train u_i``, sigma the weighted sample
std over the training rows, and the same read of the rows sums the held-out rows'
weighted mean loss (``FitResult.holdout_log_loss``).  GPU:
``csrc/kernels/fit_weighted.hip``; the weights are formed per tile, so another held-out
fold costs one statistics pass and no copy -- :func:`cross_validate` chooses
``reg_param`` that way.

Many fits per read of the rows (:class:`FitJob`, :meth:`BatchFitter.fit_many`,
``cross_validate(batch=...)``): the fits of a grid share the rows, the labels and the
weight streams and differ in the held-out fold, the penalty and the iterate, so one
staged tile serves several of them -- ``csrc/kernels/fit_many.hip`` packs the models into
the MFMA columns a single ``K``-class model leaves empty and ``csrc/solver/fit_many.hip``
advances all fits in lockstep, one evaluation round at a time.  The wide model
(:class:`psx.ops.wide_fit.WideFitter`) has the same calls: ``csrc/kernels/wide_fit_many.hip``
lays ``32 / KP`` models side by side in each feature's 128-byte line, so one gather, one
read of the rows, of the inverted index and of the work items serves all of them.

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
from dataclasses import asdict, dataclass, field, replace

import torch

from .. import _native
from ..models.logreg import ModelSpec, to_reference_layout
from ..models.reference import fit_reference, weighted_feature_std, weighted_loss_grad
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
    holdout_log_loss: float | None = None  # weighted mean loss of the held-out fold at ``w`` (FitWeights.holdout)
    center: torch.Tensor | None = None  # [F] fp32 centre of a centred fp32-row fit (psx/ops/fit_f32.py); ``w`` is raw

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


@dataclass
class FitWeights:
    """Row weights of a fit: ``u_i = sample_weight_i * class_weight[y_i]``; rows
    with ``fold_i == holdout`` are left out of the fit and scored separately.

    Weighted calls in a row with the same dataset object reuse its resident copy, and
    the device copies of ``sample_weight`` / ``fold`` are reused while the same tensor
    OBJECTS are passed: do not change ``ds.X``, ``ds.y``, ``sample_weight`` or ``fold``
    in place between such calls (pass new tensors instead) -- an edit is not seen.
    The one-logit wide model (``K == 1``) has a two-entry class table, labels 0 and 1."""
    sample_weight: torch.Tensor | None = None  # [N], finite, >= 0
    class_weight: torch.Tensor | str | None = None  # [K], or "balanced": N_train / (K_present * count_c)
    fold: torch.Tensor | None = None  # [N] fold ids in 0..255
    holdout: int | None = None


@dataclass
class FitJob:
    """One fit of :meth:`BatchFitter.fit_many`: its penalty, its held-out fold (a fold id of
    the shared ``FitWeights.fold``) and its start (device layout ``[P]``; None: zeros)."""
    reg_param: float
    holdout: int | None = None
    w0: torch.Tensor | None = None


class _Weights:
    """``FitWeights`` checked against a dataset (ValueError before any launch): fp32
    ``sw`` / ``cw`` and uint8 ``fold`` as the kernels read them (or None), and the
    float64 effective training / held-out weights ``u`` / ``h`` of every row."""

    def __init__(self, spec, ds, wts: FitWeights):
        N, K = ds.rows, max(2, spec.K)  # (the one-logit model has labels 0 and 1)
        y = ds.y.long().cpu()
        self.src = wts
        self.sw = self.cw = self.fold = None
        self.holdout = -1
        if wts.sample_weight is not None:
            self.sw = wts.sample_weight.detach().to("cpu", torch.float32).reshape(-1)
            if self.sw.numel() != N:
                raise ValueError(f"{self.sw.numel()} sample weights for {N} rows")
            if not bool(torch.isfinite(self.sw).all()) or bool((self.sw < 0).any()):
                raise ValueError("sample weights must be finite and >= 0")
        if wts.fold is not None:
            f = wts.fold.detach().cpu().reshape(-1)
            if f.numel() != N:
                raise ValueError(f"{f.numel()} fold ids for {N} rows")
            if f.is_floating_point() or int(f.min()) < 0 or int(f.max()) > 255:
                raise ValueError("fold ids must be integers in [0, 255]")
            self.fold = f.to(torch.uint8)
        if wts.holdout is not None:
            if self.fold is None or not 0 <= int(wts.holdout) <= 255:
                raise ValueError("a held-out fold needs fold ids and a fold in [0, 255]")
            self.holdout = int(wts.holdout)
        held = self.fold == self.holdout if self.holdout >= 0 else torch.zeros(N, dtype=torch.bool)
        cw = wts.class_weight
        if isinstance(cw, str):
            if cw != "balanced":
                raise ValueError(f"class_weight is a [K] tensor or 'balanced', got {cw!r}")
            cnt = torch.bincount(y[~held], minlength=K).double()
            cw = torch.where(cnt > 0, float((~held).sum()) / (float((cnt > 0).sum()) * cnt.clamp_min(1)), cnt * 0)
        if cw is not None:
            self.cw = cw.detach().to("cpu", torch.float32).reshape(-1)
            if self.cw.numel() != K:
                raise ValueError(f"{self.cw.numel()} class weights for {K} classes")
            if not bool(torch.isfinite(self.cw).all()) or bool((self.cw < 0).any()):
                raise ValueError("class weights must be finite and >= 0")
        v = torch.ones(N) if self.sw is None else self.sw
        if self.cw is not None:
            v = v * self.cw[y]  # the fp32 product the kernels form
        v = v.double()
        self.u, self.h = torch.where(held, v * 0, v), torch.where(held, v, v * 0)
        if not float(self.u.sum()) > 1.0 or int((self.u > 0).sum()) < 2:
            raise ValueError("the training rows need a weight sum > 1 and two rows of positive weight")
        if self.holdout >= 0 and not float(self.h.sum()) > 0.0:
            raise ValueError(f"the held-out fold {self.holdout} holds no weight")


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
        self.wcache = {}  # padded device copies of a weighted call's sample weights / fold ids
        self.applied = None  # the checked weights the native fitter holds for these rows
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
    ``_loss_grad_cpu``, ``_eval_weighted_cpu``).  The resident dataset a ``_load`` returns
    has ``src``, ``N``, ``Npad`` (the length of the weight streams), ``wcache`` and ``applied``."""

    _wts: _Weights | None = None  # of the weighted call in progress

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

    # ---- weights -------------------------------------------------------------
    def _weighted(self, ds, weights, min_rows):
        self._check_data(self.spec, ds, min_rows)
        return _Weights(self.spec, ds, weights)

    def _streams(self, data, wts):
        """The padded device copies of ``wts``'s sample weights and fold ids (or None): one copy per source tensor."""
        def padded(v, src, dtype):  # [Npad] on the device
            if v is None:
                return None
            if data.wcache.get(dtype, (None, None))[0] is not src:
                t = torch.zeros(data.Npad, dtype=dtype, device=self.device)
                t[: data.N] = v.to(self.device)
                data.wcache[dtype] = (src, t)
            return data.wcache[dtype][1]

        return padded(wts.sw, wts.src.sample_weight, torch.float32), padded(wts.fold, wts.src.fold, torch.uint8)

    def _apply_weights(self, data, wts):
        """Hand ``wts`` to the native fitter for the resident ``data`` (a statistics pass, no copy of the rows)."""
        sw, fold = self._streams(data, wts)
        self._native.set_weights(sw.data_ptr() if sw is not None else 0,
                                 wts.cw.tolist() if wts.cw is not None else [],
                                 fold.data_ptr() if fold is not None else 0, wts.holdout, stream_handle(self.device))
        data.applied = wts

    def _eval_weighted(self, ds, w, wts):
        """(training loss, gradient, held-out loss) of one raw evaluation under ``wts``."""
        s = self.spec
        if w.numel() != s.P:
            raise ValueError(f"the model has {s.P} weights in device layout, got {w.numel()}")
        self._wts = wts
        try:
            if self._native is None:
                return self._eval_weighted_cpu(ds, w, wts)
            with torch.cuda.device(self.device):
                self._load(ds)
                st = stream_handle(self.device)
                wd = w.detach().to(self.device, torch.float32).reshape(-1).contiguous()
                g = torch.empty(s.P, dtype=torch.float32, device=self.device)
                loss = self._native.loss_grad(wd.data_ptr(), g.data_ptr(), st)
                return float(loss), g, float(self._native.holdout_loss(st))
        finally:
            self._wts = None

    def holdout_loss(self, ds, w: torch.Tensor, weights: FitWeights) -> float:
        """The held-out fold's weighted mean loss at ``w``: one raw evaluation."""
        wts = self._weighted(ds, weights, 1)
        if wts.holdout < 0:
            raise ValueError("holdout_loss needs FitWeights.holdout")
        return self._eval_weighted(ds, w, wts)[2]

    # ---- one evaluation ------------------------------------------------------
    def loss_grad(self, ds, w: torch.Tensor, weights: FitWeights | None = None):
        """Mean loss of ``w`` (device layout ``[P]``) over ``ds`` and its gradient in
        the same layout (zero for every feature a sparse ``ds`` does not touch):
        original feature space, no standardisation, no penalty.  Calls in a row with
        the same ``ds`` object reuse its resident copy (and skip the checks): do not
        change its tensors in between.  With ``weights`` the weighted mean loss of the
        training rows and its gradient."""
        if weights is not None:
            return self._eval_weighted(ds, w, self._weighted(ds, weights, 1))[:2]
        if self._native is not None and self._native.weighted:  # the resident rows keep their statistics pass
            with torch.cuda.device(self.device):
                self._native.set_weights(stream=stream_handle(self.device))
            if self._data is not None:
                self._data.applied = None
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

    # ---- many fits per read of the rows ----------------------------------------------
    def _many_setup(self, ds, weights, holdouts, min_rows):
        """Checks of a batched call (ValueError before any launch) -> the checked weights of every distinct
        held-out fold, in the jobs' order."""
        weights = weights or FitWeights()
        if weights.holdout is not None:
            raise ValueError("the shared FitWeights of a batched call hold no fold out: every job names its own")
        if not holdouts:
            raise ValueError("a batched call needs at least one job")
        if isinstance(weights.class_weight, str) and len(set(holdouts)) > 1:
            raise ValueError("'balanced' class weights depend on the held-out fold; a batched call shares one table")
        return [self._weighted(ds, replace(weights, holdout=h), min_rows) for h in dict.fromkeys(holdouts)]

    def _many_resident(self, ds, wts):
        """The resident rows of ``ds`` and the native arguments of the shared streams."""
        if self._data is None or self._data.src is not ds:
            self._load(ds)
        data = self._data
        sw, fold = self._streams(data, wts)
        return data, (sw.data_ptr() if sw is not None else 0, wts.cw.tolist() if wts.cw is not None else [],
                      fold.data_ptr() if fold is not None else 0)

    def _many_outputs(self, data, jobs):
        """The device buffers a batched fit writes: weights ``[M, P]`` and sigmas ``[M, width]``."""
        M, s = len(jobs), self.spec
        return (torch.empty(M, s.P, dtype=torch.float32, device=self.device),  # finalize writes all of it
                torch.empty(M, s.Fp, dtype=torch.float32, device=self.device))

    def _many_std_features(self, data, std_m):
        """``FitResult.std`` / ``features`` of one job from its row of the sigma buffer."""
        return std_m[: self.spec.F].clone(), None

    def loss_grad_many(self, ds, ws, weights: FitWeights | None, holdouts):
        """One raw evaluation of the M weight vectors ``ws`` (``[M, P]``, device layout; no standardisation,
        no penalty), vector m with fold ``holdouts[m]`` (or None) held out, on ONE read of the rows per
        ``many_capacity`` vectors -> ``(losses [M], grads [M, P], holdout_losses [M])``."""
        holdouts = list(holdouts)
        checked = self._many_setup(ds, weights, holdouts, 1)
        ws = torch.stack(list(ws)) if not isinstance(ws, torch.Tensor) else ws
        if ws.dim() != 2 or ws.shape != (len(holdouts), self.spec.P):
            raise ValueError(f"{len(holdouts)} weight vectors of {self.spec.P} are needed, got {tuple(ws.shape)}")
        if self._native is None:
            by = dict(zip(dict.fromkeys(holdouts), checked))
            rows = [self._eval_weighted(ds, w, by[h]) for w, h in zip(ws, holdouts)]
            return (torch.tensor([r[0] for r in rows], dtype=torch.float64), torch.stack([r[1] for r in rows]),
                    torch.tensor([r[2] for r in rows], dtype=torch.float64))
        with torch.cuda.device(self.device):
            _, streams = self._many_resident(ds, checked[0])
            wd = ws.detach().to(self.device, torch.float32).contiguous()
            g = torch.empty_like(wd)
            loss, ho = self._native.loss_grad_many(*streams, wd.data_ptr(), [-1 if h is None else int(h) for h in holdouts],
                                                   g.data_ptr(), stream_handle(self.device))
        return torch.tensor(loss, dtype=torch.float64), g, torch.tensor(ho, dtype=torch.float64)

    @property
    def many_capacity(self) -> int:
        """Models one read of the rows serves on the GPU: a function of the padded width and the class count
        (dense), of the padded class count alone (wide: ``32 // KP``)."""
        return int(self._native.many_capacity)

    def fit_many(self, train, jobs, weights: FitWeights | None = None) -> list:
        """Fit every :class:`FitJob` on ``train``: result i is what ``fit(train, w0=jobs[i].w0,
        weights=FitWeights(..., holdout=jobs[i].holdout))`` returns under ``reg_param = jobs[i].reg_param``.
        ``weights`` carries the shared ``sample_weight``, ``class_weight`` and ``fold`` (its own ``holdout``
        stays None); the other options are the fitter's.  On the GPU all fits advance in lockstep, each
        evaluation round reading the rows once per ``many_capacity`` unfinished jobs; a job's result does
        not depend on the jobs beside it.  ``FitResult.seconds`` is the whole batch's."""
        jobs = list(jobs)
        checked = self._many_setup(train, weights, [j.holdout for j in jobs], 2)
        s, o = self.spec, self.opts
        for j in jobs:
            _check_options(replace(o, reg_param=float(j.reg_param)))
            if j.w0 is not None and j.w0.numel() != s.P:
                raise ValueError(f"the model has {s.P} weights in device layout, got {j.w0.numel()}")
        if self._native is None:
            out = []
            try:
                for j in jobs:
                    self.opts = replace(o, reg_param=float(j.reg_param))
                    out.append(self.fit(train, w0=j.w0, weights=replace(weights or FitWeights(), holdout=j.holdout)))
            finally:
                self.opts = o
            return out
        t0 = time.perf_counter()
        with torch.cuda.device(self.device):
            st, nat, M = stream_handle(self.device), self._native, len(jobs)
            data, streams = self._many_resident(train, checked[0])
            w0s = [None if j.w0 is None else j.w0.detach().to(self.device, torch.float32).reshape(-1).contiguous()
                   for j in jobs]
            holds = [-1 if j.holdout is None else int(j.holdout) for j in jobs]
            w, std = self._many_outputs(data, jobs)
            rows = nat.fit_many(*streams, [float(j.reg_param) for j in jobs], holds,
                                [0 if t is None else t.data_ptr() for t in w0s], int(o.max_iter), float(o.tol),
                                int(o.ls_max), bool(o.zero_const), w.data_ptr(), std.data_ptr(), st)
            ev = list(nat.many_round_seconds)
            ho = None
            if any(h >= 0 for h in holds):  # one more round: every job's held-out loss at its returned weights
                ho = nat.loss_grad_many(*streams, w.data_ptr(), holds, torch.empty_like(w).data_ptr(), st)[1]
        dt = time.perf_counter() - t0
        out = []
        for m, r in enumerate(rows):
            sd, features = self._many_std_features(data, std[m])
            out.append(FitResult(spec=s, w=w[m].clone(), objective=float(r[0]), log_loss=float(r[1]), history=list(r[2]),
                                 iters=int(r[3]), evals=int(r[4]), reason=str(r[5]), std=sd, seconds=dt,
                                 pass_seconds=statistics.median(ev) if ev else 0.0,
                                 options=replace(o, reg_param=float(jobs[m].reg_param)), ls_fail=int(r[6]),
                                 features=features, holdout_log_loss=float(ho[m]) if holds[m] >= 0 else None))
        return out

    # ---- the fit ---------------------------------------------------------------
    def fit(self, train, w0: torch.Tensor | None = None, valid=None, valid_every: int = 1,
            patience: int | None = None, weights: FitWeights | None = None) -> FitResult:
        """Fit ``train`` from zeros or from ``w0`` (device layout, a warm start).

        With ``valid`` the current iterate is scored with :class:`Scorer` every
        ``valid_every`` accepted iterations; the result carries the iterate with the
        lowest validation log-loss, and ``patience`` checks in a row without
        improvement end the fit with reason ``early_stop``.  With ``weights`` the
        weighted objective, and ``holdout_log_loss`` from one raw evaluation at the
        returned weights."""
        if weights is not None:
            wts = self._weighted(train, weights, 2)
            self._wts = wts
            try:
                res = self.fit(train, w0, valid, valid_every, patience)
            finally:
                self._wts = None
            if wts.holdout >= 0:
                res.holdout_log_loss = self._eval_weighted(train, res.w, wts)[2]
            return res
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
        wts, st = self._wts, stream_handle(self.device)
        if wts is not None and self._data is not None and self._data.src is ds:
            data = self._data  # weighted calls on one dataset object share its resident copy (cross_validate)
        else:
            data = _Resident(ds, self.device)
            self._native.set_data(data.X.data_ptr(), data.y.data_ptr(), data.N, data.Npad, st)  # (clears the weights)
            self._data = data  # the native fitter reads these buffers until the next set_data
        if wts is not None and data.applied is not wts:
            self._apply_weights(data, wts)
        return data

    def _rows64(self, ds):
        return ds.X[:, : self.spec.F].to(torch.bfloat16).double().cpu(), ds.y.long().cpu()

    def _eval_weighted_cpu(self, ds, w, wts):
        s = self.spec
        X, y = self._rows64(ds)
        wc = w.detach().double().cpu()
        loss, gc, gb = weighted_loss_grad(X, y, s.coef(wc), s.intercept(wc), wts.u)
        ho = weighted_loss_grad(X, y, s.coef(wc), s.intercept(wc), wts.h)[0]
        return float(loss), s.pack(gc, gb, device=self.device), float(ho)

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
        X, y = self._rows64(train)
        extra = {}
        if self._wts is not None:  # float64 weighted closures through the oracle's own hooks
            u = self._wts.u
            extra = dict(loss_grad=lambda ce, bb: weighted_loss_grad(X, y, ce, bb, u), std=weighted_feature_std(X, u))
        c0 = b0 = None
        if w0 is not None:
            wc = w0.detach().float().cpu().reshape(-1)
            c0, b0 = s.coef(wc).double(), s.intercept(wc).double()

        def run(max_iter):
            return fit_reference(X, y, c0, b0, num_classes=s.K, reg_param=o.reg_param, max_iter=max_iter, tol=o.tol,
                                 hist=o.hist, ls_max=o.ls_max, zero_const=o.zero_const, **extra)

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


# Padded class counts at which ``cross_validate(batch="auto")`` batches the wide model: those where the batched
# grid was MEASURED faster than the sequential one.  2^20 rows x 45 entries in 2^20 features, 5 folds x 4 penalties
# (profiles/r21/README.md): batched / sequential 0.353 / 0.853 s with one logit (KP 1), 0.597 / 1.165 s with 6
# classes (KP 8).  KP 2, 4 and 16 have not been measured: "auto" takes the sequential path there.
WIDE_AUTO_BATCH_KP = (1, 8)


@dataclass
class CVResult:
    reg_params: list
    losses: list  # [R][folds] held-out weighted mean loss
    means: list  # [R]
    best_reg_param: float
    fold: torch.Tensor  # [N] uint8, the fold of every row
    seconds: float


def cross_validate(spec, ds, reg_params, folds: int = 5, seed: int = 0, device="cpu",
                   opts: FitOptions | None = None, sample_weight=None, class_weight=None,
                   col_chunk: int | None = None, batch: int | str | None = None) -> CVResult:
    """K-fold choice of ``reg_param``: fold ids are drawn once, the rows are made resident
    once, and the ``folds * len(reg_params)`` fits differ only in the held-out fold (one
    statistics pass, no copy) and the penalty.  A ``WideSpec`` with a ``SparseDataset``
    runs the wide fitter (``col_chunk`` as :class:`psx.ops.wide_fit.WideFitter`): its
    touched features, inverted index and work items are built once for all the fits.  The best penalty has the lowest mean
    held-out loss (the first of equals).  ``ds`` and ``sample_weight`` must not change
    while it runs: every fit reuses the first one's resident copies (see :class:`FitWeights`).

    ``batch``: None runs the fits one after another.  A number runs them that many at a time through
    ``fit_many`` of the dense or the wide fitter (one read of the rows per evaluation round and
    ``many_capacity`` jobs), ``"auto"`` all of them at once -- or one after another where that is not
    faster: a dense model whose read of the rows serves a single model (``many_capacity`` 1), and the wide
    model at the padded class counts of ``WIDE_AUTO_BATCH_KP`` only.  A class-weight table or none; the
    held-out losses agree with the sequential path to the fits' accuracy, not bit for bit."""
    from .panel_fit import PanelSpec  # (imports this module)

    if isinstance(spec, PanelSpec):
        raise NotImplementedError("cross_validate is not implemented for the panel model")
    regs = [float(r) for r in reg_params]
    if not regs or not 2 <= folds <= 255 or folds > ds.rows:
        raise ValueError("cross_validate needs penalties and 2 <= folds <= min(255, rows)")
    t0 = time.perf_counter()
    g = torch.Generator().manual_seed(seed)
    fold = (torch.randperm(ds.rows, generator=g) % folds).to(torch.uint8)
    o = opts or FitOptions()
    if is_gpu(torch.device(device)):
        ds = ds.to(device)
    if isinstance(spec, WideSpec):
        from .wide_fit import WideFitter

        f = WideFitter(spec, device, o, col_chunk=col_chunk)
    else:
        f = BatchFitter(spec, device, o)
    if batch is not None and not (batch == "auto" or (isinstance(batch, int) and batch >= 1)):
        raise ValueError("cross_validate(batch=...) is 'auto' or a number >= 1")
    # "auto": batched wherever one read of the rows serves at least two models.  Measured on 2^20 rows, 5 folds x
    # 4 penalties (profiles/r20/README.md): batched / sequential 0.174 / 0.352 s at width 1,024 with 6 classes,
    # 0.045 / 0.152 s with 2, and faster in every other measured cell (widths 128, 512, 2,048; 2 and 6 classes).
    # With capacity 1 (width 2,048, more than 8 classes) there is nothing to share: the sequential path.
    if batch == "auto" and f._native is not None and f.many_capacity < 2:
        batch = None
    if batch == "auto" and f._native is not None and isinstance(spec, WideSpec) and spec.KP not in WIDE_AUTO_BATCH_KP:
        batch = None
    if batch is not None:
        jobs = [FitJob(r, k) for r in regs for k in range(folds)]
        step = len(jobs) if batch == "auto" else batch
        shared, res = FitWeights(sample_weight, class_weight, fold), []
        for i in range(0, len(jobs), step):
            res += f.fit_many(ds, jobs[i: i + step], shared)
        losses = [[res[i * folds + k].holdout_log_loss for k in range(folds)] for i in range(len(regs))]
        means = [sum(row) / folds for row in losses]
        return CVResult(regs, losses, means, regs[means.index(min(means))], fold, time.perf_counter() - t0)
    losses = []
    for r in regs:
        f.opts = FitOptions(**{**asdict(o), "reg_param": r})
        _check_options(f.opts)
        # (every fit is handed the same dataset object: its first load is the only copy)
        losses.append([f.fit(ds, weights=FitWeights(sample_weight, class_weight, fold, k)).holdout_log_loss
                       for k in range(folds)])
    means = [sum(row) / folds for row in losses]
    return CVResult(regs, losses, means, regs[means.index(min(means))], fold, time.perf_counter() - t0)


__all__ = ["BatchFitter", "CVResult", "FitJob", "FitOptions", "FitResult", "FitWeights", "cross_validate", "loss_grad"]

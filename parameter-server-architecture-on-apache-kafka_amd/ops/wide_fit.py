"""Fit the wide (sparse-input) model to a dataset until the optimiser converges --
the objective, optimiser and result of :mod:`psx.ops.fit`, for CSR rows over
10^6 .. 10^8 hashed features, multinomial or one-logit (``K == 1``, sigmoid).

The fit runs in the subspace of the U distinct features the training set touches:
every other feature has sigma 0 by definition and is excluded (coefficient 0, or
``w0``'s value with ``zero_const=False``), as a constant feature is in the dense fit.
sigma_f is the sample std of feature f over ALL rows, absent entries counting as
zeros and an id repeated within a row as the sum of its entries.

GPU: ``csrc/kernels/wide_fit_kernels.hip`` driven by ``csrc/solver/wide_fit.hip`` (a
missing extension is a hard error).  The gradient's scatter runs without atomics: the
row pass stores every residual row once, the column pass gathers them through an
inverted index whose lists keep one fixed order, so a fit is bit-reproducible.  The
one-time structures (sorted feature ids, compact columns, inverted index, work items)
are built with torch on the device.  Columns longer than ``col_chunk`` entries are cut
into chunks of that size, one work item each, summed in chunk order.

CPU: :func:`psx.models.reference.fit_reference` on float64 sparse closures (the CSR
matrix over the touched columns and its transpose); no ``N x F`` matrix is built.
"""
from __future__ import annotations

import time
import warnings

import torch

from .. import _native
from ..models.reference import fit_reference
from ..models.wide import WideSpec
from .fit import FitOptions, FitResult, _FitterBase, _validate_oracle
from .lr import stream_handle
from .sparse import SparseDataset

# Entries of a work item of the column pass.  The rule of thumb for an atomics-free
# scatter-add is to split lists longer than a quarter of one wave's share of the entries
# (about 1,400 here: 47M entries, 8,192 waves in flight), 512 being a measured starting
# point; the sweep 128 .. 4096 of profiles/r13/README.md picked this value (the column
# pass is flat, the chunk-order sum of the reduction falls with the number of items).
DEFAULT_COL_CHUNK = 2048


def _check_spec(spec):
    if not isinstance(spec, WideSpec):
        raise ValueError(f"the wide fit trains the wide model (WideSpec), not {type(spec).__name__}")
    if not 1 <= spec.K <= 16:
        raise ValueError(f"{spec.K} classes: the wide model has 1 (sigmoid) .. 16")


def _check_data(spec: WideSpec, ds, min_rows: int):
    if not isinstance(ds, SparseDataset):
        raise ValueError(f"the wide model ({spec.F} features, {spec.K} classes) fits sparse rows (SparseDataset), "
                         f"got {type(ds).__name__}")
    if ds.num_features > spec.F:
        raise ValueError(f"the data has {ds.num_features} features, the model only {spec.F}")
    if ds.nnz and (int(ds.idx.min()) < 0 or int(ds.idx.max()) >= spec.F):
        raise ValueError(f"feature ids reach {int(ds.idx.max())} (lowest {int(ds.idx.min())}), the model has "
                         f"{spec.F} features")
    if ds.rows < min_rows:
        raise ValueError(f"{ds.rows} rows: at least {min_rows} needed")
    if ds.rows >= (1 << 31) - 64:
        raise ValueError(f"{ds.rows} rows: at most 2^31 - 65")
    lo, hi = int(ds.y.min()), int(ds.y.max())
    if spec.K == 1:
        if lo < 0 or hi > 1:
            raise ValueError(f"labels span [{lo}, {hi}], the one-logit model has labels 0 and 1")
    elif lo < 0 or hi >= spec.K:
        raise ValueError(f"labels span [{lo}, {hi}], the model has classes [0, {spec.K})")


class _Index:
    """What a fit needs of one dataset, on ``device``: the sorted touched features
    ``uniq`` [U], every entry's compact column ``col``, and the inverted index
    (``colptr``, ``crow``, ``cval``) ordered by (column, row) with a stable sort, so
    every column's list has one fixed order."""

    def __init__(self, spec: WideSpec, ds: SparseDataset, device):
        self.src = ds
        self.N = ds.rows
        self.indptr = ds.indptr.to(device, torch.int64).contiguous()
        self.val = ds.val.to(device, torch.bfloat16).contiguous()
        self.y = ds.y.to(device, torch.int32).contiguous()
        uniq, col = torch.unique(ds.idx.to(device, torch.int64), sorted=True, return_inverse=True)
        self.U = int(uniq.numel())
        if (self.U + 1) * spec.KP >= 1 << 31:
            raise ValueError(f"{self.U} touched features x {spec.KP} padded classes: the fit's vectors must stay "
                             f"below 2^31 elements")
        self.uniq = uniq.to(torch.int32)
        self.col = col.to(torch.int32).contiguous()
        counts = self.indptr[1:] - self.indptr[:-1]
        row_of = torch.repeat_interleave(torch.arange(self.N, device=device, dtype=torch.int32), counts)
        order = torch.sort(col, stable=True).indices  # entries are in row order: (column, row) order
        self.crow = row_of[order].contiguous()
        self.cval = self.val[order].contiguous()
        self.ccount = torch.bincount(col, minlength=self.U)
        self.colptr = torch.zeros(self.U + 1, dtype=torch.int64, device=device)
        torch.cumsum(self.ccount, 0, out=self.colptr[1:])


class _Resident(_Index):
    """:class:`_Index` plus the work items of the column pass: a column of at most
    ``col_chunk`` entries is one item, a longer one is cut into consecutive chunks."""

    def __init__(self, spec, ds, device, col_chunk: int, short_max: int):
        super().__init__(spec, ds, device)
        nchunks = (self.ccount + (col_chunk - 1)) // col_chunk
        first = torch.zeros(self.U + 1, dtype=torch.int64, device=device)
        torch.cumsum(nchunks, 0, out=first[1:])
        self.n_items = int(first[-1]) if self.U else 0
        if self.n_items >= (1 << 31) - 1:
            raise ValueError(f"{self.n_items} work items: raise col_chunk")
        item_col = torch.repeat_interleave(torch.arange(self.U, device=device), nchunks)
        chunk = torch.arange(self.n_items, device=device) - first[item_col]
        self.item_begin = (self.colptr[item_col] + chunk * col_chunk).contiguous()
        self.item_end = torch.minimum(self.item_begin + col_chunk, self.colptr[item_col + 1]).contiguous()
        self.col_item0 = first.to(torch.int32)
        short = (self.item_end - self.item_begin) <= short_max
        self.short_items = torch.nonzero(short).view(-1).to(torch.int32)
        self.long_items = torch.nonzero(~short).view(-1).to(torch.int32)


def _closures(ix: _Index, K: int):
    """float64 ``loss_grad(coef_eff [K, U], b [K])`` and sigma [U] of the rows behind ``ix`` (CPU)."""
    N, U = ix.N, ix.U
    val = ix.val.double()
    with warnings.catch_warnings():  # "sparse CSR support is in beta"
        warnings.simplefilter("ignore", UserWarning)
        A = torch.sparse_csr_tensor(ix.indptr, ix.col.long(), val, size=(N, U))
        At = torch.sparse_csr_tensor(ix.colptr, ix.crow.long(), ix.cval.double(), size=(U, N))
    y = ix.y.long()

    def loss_grad(ce, b):
        z = (A @ ce.t().contiguous()) + b
        if K == 1:
            zz = z[:, 0]
            yy = (y > 0).to(z.dtype)
            loss = (torch.nn.functional.softplus(zz) - yy * zz).mean()
            r = (torch.sigmoid(zz) - yy).view(-1, 1)
        else:
            loss = (torch.logsumexp(z, dim=1) - z.gather(1, y.view(-1, 1)).squeeze(1)).mean()
            r = torch.softmax(z, dim=1)
            r[torch.arange(N), y] -= 1.0
        return loss, (At @ r).t() / N, r.sum(0) / N

    # cells: entries of one column with the same row are adjacent in the inverted index and are summed first
    col_of = torch.repeat_interleave(torch.arange(U), ix.ccount)
    head = torch.ones(col_of.numel(), dtype=torch.bool)
    if head.numel() > 1:
        head[1:] = (col_of[1:] != col_of[:-1]) | (ix.crow[1:] != ix.crow[:-1])
    cell = torch.cumsum(head, 0) - 1
    x = torch.zeros(int(head.sum()), dtype=torch.float64).index_add_(0, cell, ix.cval.double())
    ccol = col_of[head]
    present = torch.bincount(ccol, minlength=U).double()
    mean = torch.zeros(U, dtype=torch.float64).index_add_(0, ccol, x) / N
    sq = torch.zeros(U, dtype=torch.float64).index_add_(0, ccol, (x - mean[ccol]) ** 2)
    if N < 2:
        return loss_grad, torch.zeros(U, dtype=torch.float64)
    return loss_grad, ((sq + (N - present) * mean * mean) / (N - 1)).clamp_min(0).sqrt()


class WideFitter(_FitterBase):
    """Full-batch L-BFGS trainer of one wide model on one device
    (``fit`` / ``loss_grad`` / ``valid`` as :class:`psx.ops.fit.BatchFitter`).

    ``fit`` may be called any number of times (each call loads its dataset); no
    state of one fit reaches the next.  ``col_chunk`` (default 2048) is the length at
    which a column's list is cut into work items; the reduction adds a column's items
    one after the other, N / col_chunk of them for a column every row holds, so a
    small ``col_chunk`` on many rows (below N / 1000 or so) slows every evaluation."""

    _check_spec = staticmethod(_check_spec)
    _check_data = staticmethod(_check_data)

    def __init__(self, spec: WideSpec, device, opts: FitOptions | None = None, col_chunk: int | None = None):
        super().__init__(spec, device, opts)
        self.col_chunk = DEFAULT_COL_CHUNK if col_chunk is None else int(col_chunk)
        if self.col_chunk < 1:
            raise ValueError(f"col_chunk must be >= 1, got {col_chunk}")

    def _new_native(self, hip):
        return hip.WideBatchFitter(self.spec.K, self.spec.KP, self.opts.hist, self.opts.max_wg or 0)

    def _load(self, ds: SparseDataset):
        if self._native is None:
            self._data = _Index(self.spec, ds, self.device)
            return self._data
        dev = self.device
        d = _Resident(self.spec, ds, dev, self.col_chunk, int(_native.hip().wide_fit_short))
        self._native.set_data(d.indptr.data_ptr(), d.col.data_ptr(), d.val.data_ptr(), d.y.data_ptr(),
                              d.uniq.data_ptr(), d.colptr.data_ptr(), d.crow.data_ptr(), d.cval.data_ptr(),
                              d.item_begin.data_ptr(), d.item_end.data_ptr(), d.col_item0.data_ptr(),
                              d.short_items.data_ptr(), d.long_items.data_ptr(), d.N, d.U, self.spec.F, d.n_items,
                              int(d.short_items.numel()), int(d.long_items.numel()), stream_handle(dev))
        self._data = d  # the native fitter reads these buffers until the next set_data
        return d

    def _untouched(self, w0):
        """The full vector before the touched features are written: zeros, or with
        ``zero_const=False`` the start's coefficients (centred like every excluded
        feature's when the fit centres coefficients)."""
        s, o = self.spec, self.opts
        w = torch.zeros(s.P, dtype=torch.float32, device=self.device)
        if w0 is not None and not o.zero_const:
            c = w0.detach().to(self.device, torch.float32).reshape(-1)[: s.F * s.KP].view(s.F, s.KP)[:, : s.K]
            if o.reg_param == 0.0 and s.K > 1:
                c = c - c.mean(1, keepdim=True)
            w[: s.F * s.KP].view(s.F, s.KP)[:, : s.K] = c
        return w

    _result_vector = _untouched  # finalize writes the touched features and the intercepts

    def _std_features(self, d, st):
        std = torch.empty(d.U, dtype=torch.float32, device=self.device)
        self._native.read_std(std.data_ptr(), st)
        return std, d.uniq.clone()

    def _loss_grad_cpu(self, ds, w, resident):
        s = self.spec
        d = self._data if resident else self._load(ds)
        wc = w.detach().double().cpu().reshape(-1)
        fg, _ = _closures(d, s.K)
        rows = d.uniq.long()
        ce = wc[: s.F * s.KP].view(s.F, s.KP)[rows][:, : s.K].t()
        loss, gc, gb = fg(ce, s.intercept(wc))
        g = torch.zeros(s.P, dtype=torch.float32, device=self.device)
        g[: s.F * s.KP].view(s.F, s.KP)[rows, : s.K] = gc.t().float()
        g[s.F * s.KP: s.F * s.KP + s.K] = gb.float()
        return float(loss), g

    def _fit_cpu(self, train, w0, valid, valid_every, patience) -> FitResult:
        s, o = self.spec, self.opts
        d = self._load(train)
        fg, sd = _closures(d, s.K)
        rows = d.uniq.long()
        c0, b0 = torch.zeros(s.K, d.U, dtype=torch.float64), None
        if w0 is not None:
            wc = w0.detach().float().cpu().reshape(-1)
            c0 = wc[: s.F * s.KP].view(s.F, s.KP)[rows][:, : s.K].t().double()
            b0 = s.intercept(wc).double()

        def run(max_iter):
            return fit_reference(None, d.y, c0, b0, reg_param=o.reg_param, max_iter=max_iter, tol=o.tol, hist=o.hist,
                                 ls_max=o.ls_max, zero_const=o.zero_const, loss_grad=fg, std=sd)

        def pack(r):
            w = self._untouched(w0)
            w[: s.F * s.KP].view(s.F, s.KP)[rows, : s.K] = r.coef.t().float()
            w[s.F * s.KP: s.F * s.KP + s.K] = r.intercept.float()
            return w

        t0 = time.perf_counter()
        ref = run(o.max_iter)
        dt = time.perf_counter() - t0
        res = FitResult(spec=s, w=pack(ref), objective=ref.objective, log_loss=ref.log_loss,
                        history=list(ref.history), iters=ref.iters, evals=ref.evals, reason=ref.reason,
                        std=ref.std.float(), seconds=0.0, pass_seconds=dt / max(1, ref.evals), options=o,
                        ls_fail=ref.ls_fail, features=d.uniq.clone())
        if valid is not None:
            _validate_oracle(res, ref, run, pack, self._validator(valid), valid_every, patience)
        return res


def wide_loss_grad(spec: WideSpec, ds: SparseDataset, w: torch.Tensor, device, max_wg: int | None = None,
                   col_chunk: int | None = None):
    """One evaluation: ``(mean loss, gradient [P] in device layout)`` of ``w`` over
    ``ds`` in the original feature space -- no standardisation, no penalty."""
    return WideFitter(spec, device, FitOptions(max_wg=max_wg), col_chunk=col_chunk).loss_grad(ds, w)


__all__ = ["WideFitter", "wide_loss_grad", "DEFAULT_COL_CHUNK"]

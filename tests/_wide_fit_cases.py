"""Inputs, float64 oracles and the derived bound shared by the wide full-batch fit
tests (test_wide_fit_cpu.py, test_gpu_wide_fit.py).

The sparse case generator: row lengths Poisson(12) clamped to [2, 40], rows 3, 8, 13,
18, 23 and 28 forced to 0, 1, 63, 64, 65 and 700 drawn entries; ids are log-uniform
ranks over a 1,500-id vocabulary spread over [2, F) (many columns of 1-3 entries, a
few long ones); every 7th row repeats its first id with half its value; values are
sign(v)(|v| + 0.1)/sqrt(len) in bf16.  With ``full_cols`` every row also holds feature
0 = 1.5 (sigma exactly 0) and feature 1 ~ N(0,1) (a column of N entries); without,
row 3 has no entry at all.  Labels are drawn from a planted softmax / sigmoid model.
The generator is written from the issue's description, not from its author's script
(which was not committed): seeds, U (about 1,170 - 1,310 touched features) and the
oracle's iteration counts differ from the figures quoted there; |coef| reaches 40-50.

Bound of one evaluation (``loss_grad``) against float64 on the bf16 values as stored.
All arithmetic is fp32, u = 2^-24.  Per row r with nnz_r entries

    dz_r = (nnz_r + 8) u max_c (sum_e |v_e w_c| + |b_c|)

bounds the margins' error (a dot product of nnz_r + 1 terms summed in some order).  A
margin error moves a residual by at most dz_r (the softmax Jacobian's absolute row
sums are 2 p (1 - p) <= 1/2, times the 2 dz_r spread of the errors; the sigmoid's
slope is <= 1/4), the fp32 exponential and divide add 1e-6 (tests/_fit_cases.py).  A
column of c_u entries is summed in fp32 in some order:

    |dg_uk| <= 1/N sum_e (dz_r(e) + 1e-6) |v_e|  +  (c_u + 8) u / N sum_e |R_r(e)k v_e|
    |dloss| <= mean_r (2 dz_r + 1e-6 zmax) + (N + 8) u mean_r |nll_r|

(v = 1 over all rows and c = N for the intercepts).
"""
import math

import torch

from psx.models.reference import feature_std, fit_reference
from psx.models.wide import WideSpec
from psx.ops.fit import FitOptions
from psx.ops.score import Scorer
from psx.ops.sparse import SparseDataset
from psx.ops.wide_fit import WideFitter

U24 = 2.0 ** -24
VOCAB = 1500
FORCED = {3: 0, 8: 1, 13: 63, 18: 64, 23: 65, 28: 700}


def sparse_case(N, F, K, seed=0, labels_from=0, full_cols=True, signal=3.0):
    """-> (WideSpec(F, K), SparseDataset on the CPU)."""
    spec = WideSpec(F, K)
    g = torch.Generator().manual_seed(15485863 * seed + 31 * N + F + K)
    lens = torch.poisson(torch.full((N,), 12.0), generator=g).long().clamp_(2, 40)
    for r, n in FORCED.items():
        if r < N:
            lens[r] = n
    slot = torch.randperm(F - 2, generator=g)[:VOCAB] + 2  # rank -> feature id
    idx, val, indptr = [], [], [0]
    for r in range(N):
        n = int(lens[r])
        rank = torch.exp(torch.rand(n, generator=g, dtype=torch.float64) * math.log(VOCAB)).long().clamp_(1, VOCAB)
        ids = slot[(rank - 1) % slot.numel()]
        v = torch.randn(n, generator=g)
        v = torch.sign(v) * (v.abs() + 0.1) / math.sqrt(max(n, 1))
        if r % 7 == 0 and n > 0:
            ids = torch.cat([ids, ids[:1]])
            v = torch.cat([v, v[:1] * 0.5])
        if full_cols:
            ids = torch.cat([ids, torch.tensor([0, 1])])
            v = torch.cat([v, torch.tensor([1.5]), torch.randn(1, generator=g)])
        idx.append(ids)
        val.append(v)
        indptr.append(indptr[-1] + ids.numel())
    idx = torch.cat(idx).to(torch.int32)
    val = torch.cat(val).to(torch.bfloat16)
    ds = SparseDataset(torch.tensor(indptr, dtype=torch.int64), idx, val, torch.zeros(N, dtype=torch.int32), F)
    W = torch.randn(max(K, 1), F, generator=g, dtype=torch.float64) * signal
    z = csr64(ds) @ W.t()
    if K == 1:
        y = (torch.rand(N, generator=g, dtype=torch.float64) < torch.sigmoid(z[:, 0])).to(torch.int32)
    else:
        z[:, :labels_from] = -1e9
        y = torch.multinomial(torch.softmax(z, 1), 1, generator=g).view(-1).to(torch.int32)
    ds.y = y
    return spec, ds


def csr64(ds, absolute=False):
    """The rows as a dense float64 [N, F] matrix (repeated ids summed; ``absolute``: of the |values|)."""
    out = torch.zeros(ds.rows, ds.num_features, dtype=torch.float64)
    counts = ds.indptr[1:] - ds.indptr[:-1]
    rows = torch.repeat_interleave(torch.arange(ds.rows), counts)
    v = ds.val.double()
    out.index_put_((rows, ds.idx.long()), v.abs() if absolute else v, accumulate=True)
    return out


def eval_weights(spec, wscale=0.05, seed=0):
    g = torch.Generator().manual_seed(6151 + seed + spec.K)
    return spec.pack(torch.randn(spec.K, spec.F, generator=g) * wscale, torch.randn(spec.K, generator=g) * 0.5)


def eval_oracle(spec, ds, w):
    """float64 (loss, gradient [P] in device layout, |dloss| bound, |dg| bound [P], max |z|)."""
    K, N = spec.K, ds.rows
    X, Xa = csr64(ds), csr64(ds, absolute=True)
    y = ds.y.long()
    W, b = spec.coef(w).double(), spec.intercept(w).double()
    z = X @ W.t() + b
    if K == 1:
        yy = (y > 0).double()
        R = (torch.sigmoid(z[:, 0]) - yy).view(-1, 1)
        nll = torch.nn.functional.softplus(z[:, 0]) - yy * z[:, 0]
    else:
        R = torch.softmax(z, 1)
        R[torch.arange(N), y] -= 1.0
        nll = torch.logsumexp(z, 1) - z.gather(1, y.view(-1, 1)).view(-1)
    nnz = (ds.indptr[1:] - ds.indptr[:-1]).double()
    dz = (nnz + 8) * U24 * (Xa @ W.abs().t() + b.abs()).max(1).values  # [N]
    per_row = dz + 1e-6
    cu = torch.bincount(ds.idx.long(), minlength=spec.F).double()  # entries per column
    bg_c = (per_row @ Xa) / N + (cu + 8) * U24 / N * (R.abs().t() @ Xa)  # [K, F]
    bg_b = per_row.mean() + (N + 8) * U24 / N * R.abs().sum(0)  # [K]
    zmax = max(1.0, float(z.abs().max()))
    bl = float((2 * dz + 1e-6 * zmax).mean() + (N + 8) * U24 * nll.abs().mean())
    gc, gb = (R.t() @ X) / N, R.sum(0) / N
    return float(nll.mean()), pack64(spec, gc, gb), bl, pack64(spec, bg_c, bg_b), zmax


def pack64(spec, coef, intercept):
    """WideSpec.pack in float64: [K, F] coefficients and [K] intercepts -> the device layout [P]."""
    w = torch.zeros(spec.P, dtype=torch.float64)
    w[: spec.F * spec.KP].view(spec.F, spec.KP)[:, : spec.K] = coef.t()
    w[spec.F * spec.KP: spec.F * spec.KP + spec.K] = intercept
    return w


def touched(ds):
    return torch.unique(ds.idx).long()


def dense_touched(ds):
    """(features [U], float64 rows over them): what the oracle fits."""
    f = touched(ds)
    return f, csr64(ds)[:, f]


def warm_start(spec, seed=0, scale=0.05):
    g = torch.Generator().manual_seed(4242 + seed)
    return spec.pack(torch.randn(spec.K, spec.F, generator=g) * scale, torch.randn(spec.K, generator=g) * 0.1)


def oracle_fit(spec, ds, w0=None, **kw):
    """fit_reference on the dense matrix of the touched columns -> (features, FitReference)."""
    f, X = dense_touched(ds)
    c0 = b0 = None
    if w0 is not None:
        c0, b0 = spec.coef(w0)[:, f].double(), spec.intercept(w0).double()
    return f, fit_reference(X, ds.y.long(), c0, b0, num_classes=spec.K, **kw)


# the converged cases of the issue: (N, F, K, max_iter), reg_param 0.1, tol 0
CONVERGED = [(600, 5000, 4, 300), (1000, 20000, 6, 400), (600, 5000, 1, 300)]
_CACHE = {}


def converged_oracle(i):
    """(spec, ds, features, fit_reference result), computed once per session."""
    if i not in _CACHE:
        N, F, K, it = CONVERGED[i]
        spec, ds = sparse_case(N, F, K, seed=i)
        f, ref = oracle_fit(spec, ds, reg_param=0.1, tol=0.0, max_iter=it)
        _CACHE[i] = (spec, ds, f, ref)
    return _CACHE[i]


def from_dense(dense_ds):
    """The CSR form of a dense Dataset (its non-zero bf16 values) -> SparseDataset."""
    F = dense_ds.num_features
    X = dense_ds.X[:, :F]
    nz = X != 0
    rows, cols = torch.nonzero(nz, as_tuple=True)
    indptr = torch.zeros(X.shape[0] + 1, dtype=torch.int64)
    torch.cumsum(nz.sum(1), 0, out=indptr[1:])
    return SparseDataset(indptr, cols.to(torch.int32), X[rows, cols].to(torch.bfloat16), dense_ds.y.clone(), F)


# ---- validation (CPU and device) ------------------------------------------------------------
def validation_sets():
    """Train rows, and validation rows with SHUFFLED labels: fitting the train set makes them worse."""
    spec, ds = sparse_case(300, 5000, 4, seed=8)
    g = torch.Generator().manual_seed(5)
    bad = ds.slice(0, 120)
    bad = SparseDataset(bad.indptr, bad.idx, bad.val,
                        ((ds.y[:120] + 1 + torch.randint(0, 3, (120,), generator=g)) % 4).to(torch.int32), 5000)
    return spec, ds.slice(0, 200), ds.slice(200, 300), bad


def check_validation(device):
    spec, train, good, bad = validation_sets()
    f = WideFitter(spec, device, FitOptions(max_iter=12, reg_param=0.0))
    res = f.fit(train, valid=good, valid_every=2)
    marks = [i for i, _ in res.valid_history]
    assert len(marks) >= 2 and marks == sorted(set(marks))
    best_i, best_v = min(res.valid_history, key=lambda t: (t[1], t[0]))
    assert res.best_iter == best_i
    assert Scorer(spec, res.w, device).score(good.to(device)).log_loss == best_v
    stop = f.fit(train, valid=bad, valid_every=1, patience=1)
    assert stop.reason == "early_stop" and stop.best_iter == 1 and len(stop.valid_history) == 2
    assert stop.valid_history[1][1] > stop.valid_history[0][1]
    assert stop.iters < res.iters


__all__ = ["CONVERGED", "check_validation", "converged_oracle", "csr64", "dense_touched", "eval_oracle",
           "eval_weights", "feature_std", "from_dense", "oracle_fit", "sparse_case", "touched", "warm_start"]

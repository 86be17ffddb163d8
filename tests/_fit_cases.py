"""Inputs, float64 oracles and derived bounds shared by the full-batch fit tests
(test_fit_cpu.py, test_gpu_fit.py).

Bound of one evaluation (``loss_grad``) against float64 ``multinomial_loss_grad`` on
the bf16 rows as stored.  With u = 2^-24 (fp32 unit roundoff):

  1. margins: the weights enter the MFMA as bf16 hi + lo.  hi rounds w to 8 bits
     (|w - hi| <= 2^-9 |w|), lo rounds the rest to 8 bits again, so
     |w - hi - lo| <= 2^-18 |w|; the products with the exact bf16 features are
     accumulated in fp32 over F terms.  Per row r:
         dz_r = (2^-18 + (F + 8) u) max_c (sum_f |x_rf w_cf| + |b_c|)
     A margin error moves a probability by at most dz_r (the softmax Jacobian's
     absolute row sums are 2 p (1 - p) <= 1/2, times the 2 dz_r spread of the
     errors); the fp32 exponential and divide add 1e-6 (tests/_score_cases.py).
  2. residuals: they enter the backward MFMA as bf16 hi + lo too: 2^-18 |R| <= 2^-18.
  3. rows: R^T X is accumulated in fp32 over N terms (tiles in a workgroup's
     registers, then the workgroups): (N + 8) u sum_r |R_rc x_rf|.

      |dg_cf| <= 1/N sum_r (dz_r + 1e-6 + 2^-18) |x_rf| + (N + 8) u / N sum_r |R_rc x_rf|

  (x = 1 for the intercepts), and for the loss, per row 2 dz_r + 1e-6 max(1, max|z|)
  as the scorer's per-row loss, plus the fp32 sum over the rows:

      |dloss| <= mean_r (2 dz_r + 1e-6 zmax) + (N + 8) u mean_r |nll_r|
"""
import math

import torch

from psx.models.logreg import ModelSpec
from psx.models.reference import fit_reference, multinomial_loss_grad
from psx.ops.fit import BatchFitter, FitOptions
from psx.ops.score import Scorer
from psx.utils.data import Dataset

U24 = 2.0 ** -24
U18 = 2.0 ** -18


def eval_case(N, F, K, wscale=0.05, seed=0, labels_from=0):
    """X ~ N(0,1) in bf16, w ~ wscale N(0,1), intercepts 0.5 N(0,1), labels uniform in [labels_from, K)."""
    spec = ModelSpec(F, K)
    g = torch.Generator().manual_seed(7919 * N + 31 * F + K + seed)
    X = torch.zeros(N, spec.Fp)
    X[:, :F] = torch.randn(N, F, generator=g)
    ds = Dataset(X.to(torch.bfloat16), torch.randint(labels_from, K, (N,), generator=g).to(torch.int32), F)
    w = spec.pack(torch.randn(K, F, generator=g) * wscale, torch.randn(K, generator=g) * 0.5)
    return spec, ds, w


def eval_oracle(spec, ds, w):
    """float64 (loss, gradient [P] in device layout, |dloss| bound, |dg| bound [P])."""
    F, K, N = spec.F, spec.K, ds.rows
    X = ds.X[:, :F].double()
    y = ds.y.long()
    W, b = spec.coef(w).double(), spec.intercept(w).double()
    loss, gc, gb = multinomial_loss_grad(X, y, W, b)
    z = X @ W.t() + b
    R = torch.softmax(z, 1)
    R[torch.arange(N), y] -= 1.0
    nll = torch.logsumexp(z, 1) - z.gather(1, y.view(-1, 1)).view(-1)
    dz = (U18 + (F + 8) * U24) * (X.abs() @ W.abs().t() + b.abs()).max(1).values  # [N]
    per_row = dz + 1e-6 + U18
    bg_c = (per_row @ X.abs()) / N + (N + 8) * U24 / N * (R.abs().t() @ X.abs())  # [K, F]
    bg_b = per_row.mean() + (N + 8) * U24 / N * R.abs().sum(0)  # [K]
    zmax = max(1.0, float(z.abs().max()))
    bl = float((2 * dz + 1e-6 * zmax).mean() + (N + 8) * U24 * nll.abs().mean())
    pk = lambda c, i: torch.cat([torch.nn.functional.pad(c, (0, spec.Fp - F)).reshape(-1), i])  # noqa: E731
    return float(loss), pk(gc, gb), bl, pk(bg_c, bg_b), zmax


def fit_case(N, F, K, seed=0, labels_from=0):
    """bf16-rounded rows of uncentred features with scales 0.2..5 and one constant
    column; labels drawn from a softmax model (of the classes >= labels_from)."""
    spec = ModelSpec(F, K)
    g = torch.Generator().manual_seed(104729 * seed + 13 * N + F + K)
    scale = torch.logspace(math.log10(0.2), math.log10(5.0), F)[torch.randperm(F, generator=g)]
    mean = torch.randn(F, generator=g) * scale
    Z = torch.randn(N, F, generator=g)
    X = Z * scale + mean
    const = F // 2
    X[:, const] = 1.5
    Z[:, const] = 0.0
    W = torch.randn(K, F, generator=g) * (2.0 / math.sqrt(F))
    logits = Z @ W.t()
    logits[:, :labels_from] = -1e9
    y = torch.multinomial(torch.softmax(logits, 1), 1, generator=g).view(-1).to(torch.int32)
    Xp = torch.zeros(N, spec.Fp)
    Xp[:, :F] = X
    return spec, Dataset(Xp.to(torch.bfloat16), y, F), const


def rows64(spec, ds):
    return ds.X[:, : spec.F].double(), ds.y.long()


def warm_start(spec, seed=0, scale=0.05):
    g = torch.Generator().manual_seed(4242 + seed)
    return spec.pack(torch.randn(spec.K, spec.F, generator=g) * scale, torch.randn(spec.K, generator=g) * 0.1)


# the converged cases of the issue: (N, F, K, max_iter), reg_param 0.1, tol 0
CONVERGED = [(600, 20, 4, 300), (1000, 100, 6, 400)]
_CACHE = {}


def converged_oracle(i):
    """(spec, ds, constant column, fit_reference result), computed once per session."""
    if i not in _CACHE:
        N, F, K, it = CONVERGED[i]
        spec, ds, const = fit_case(N, F, K, seed=i)
        X, y = rows64(spec, ds)
        _CACHE[i] = (spec, ds, const, fit_reference(X, y, num_classes=K, reg_param=0.1, tol=0.0, max_iter=it))
    return _CACHE[i]


# ---- validation (CPU and device) ------------------------------------------------------------
def validation_sets():
    """Train rows, and validation rows with SHUFFLED labels: fitting the train set makes them worse."""
    spec, ds, _ = fit_case(300, 12, 4, seed=8)
    g = torch.Generator().manual_seed(5)
    bad = Dataset(ds.X[:120].clone(), ((ds.y[:120] + 1 + torch.randint(0, 3, (120,), generator=g)) % 4).to(torch.int32),
                  ds.num_features)
    good = Dataset(ds.X[200:].clone(), ds.y[200:].clone(), ds.num_features)
    train = Dataset(ds.X[:200].clone(), ds.y[:200].clone(), ds.num_features)
    return spec, train, good, bad


def check_validation(device):
    spec, train, good, bad = validation_sets()
    f = BatchFitter(spec, device, FitOptions(max_iter=12, reg_param=0.0))
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

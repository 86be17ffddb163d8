"""The weighted dense fit on MI355X (csrc/kernels/fit_weighted.hip): row weights, class
weights and a held-out fold against the float64 weighted oracles of
psx/models/reference.py on the bf16 rows as stored.

One evaluation keeps the derived bound of _fit_cases.py for the same (rows, weights of
the model): the weights have mean about 1, so the weighted sums have the unweighted
scale.  The short fits keep the bounds of test_gpu_fit.py / test_gpu_fit_geometry.py
(history 1e-3 of max(1, |f|), coefficients 1e-2 of the largest).

The driver clamps the grid to the tile count (as for the plain kernels), so "default
grid" means one workgroup per tile here: a workgroup without a tile is never launched
through the public interface.  The bounds taken over are far above the observed
errors (profiles/r18/README.md); the sharp checks are the unit-weight identity, sigma
and the short fits."""
import functools

import pytest
import torch

from _fit_cases import CONVERGED, eval_case, eval_oracle, fit_case, rows64
from psx import _native
from psx.models.reference import fit_reference, weighted_feature_std, weighted_loss_grad
from psx.ops.fit import BatchFitter, FitOptions, FitWeights
from psx.utils.data import Dataset

pytestmark = pytest.mark.gpu

N_ROWS = 100  # four tiles, the last with 4 real rows
CONST = 5  # constant over the training rows, varies in the held-out ones


def draw_weights(N, K, seed=0):
    """Sample weights in [0, 2] with exact zeros, a class table, 3 folds; tile 1 is held
    out as a whole, tile 2 has weight 0."""
    g = torch.Generator().manual_seed(977 + seed)
    sw = torch.rand(N, generator=g) * 2
    sw[torch.rand(N, generator=g) < 0.1] = 0.0
    fold = torch.randint(0, 3, (N,), generator=g).to(torch.uint8)
    if N > 96:
        fold[32:64] = 1
        sw[64:96] = 0.0
    return FitWeights(sw, 0.5 + torch.rand(K, generator=g), fold, 1)


def effective(wts, y):
    v = (wts.sample_weight * wts.class_weight.float()[y]).double()
    held = wts.fold == wts.holdout
    return torch.where(held, v * 0, v), torch.where(held, v, v * 0)


@functools.lru_cache(maxsize=None)
def eval_reference(FP, K):
    spec, ds, w = eval_case(N_ROWS, FP - 3, K, seed=5)
    assert spec.Fp == FP
    wts = draw_weights(N_ROWS, K)
    ds.X[wts.fold != 1, CONST] = 1.5
    X, y = rows64(spec, ds)
    u, h = effective(wts, y)
    W, b = spec.coef(w).double(), spec.intercept(w).double()
    loss, gc, gb = weighted_loss_grad(X, y, W, b, u)
    _, _, bl, bg, _ = eval_oracle(spec, ds, w)
    g64 = torch.cat([torch.nn.functional.pad(gc, (0, FP - spec.F)).reshape(-1), gb])
    return spec, ds, w, wts, float(loss), g64, float(weighted_loss_grad(X, y, W, b, h)[0]), bl, bg, \
        weighted_feature_std(X, u)


CELLS = [(FP, K) for FP in (128, 1024, 2048) for K in (2, 6, 16)]


@pytest.mark.parametrize("max_wg", [3, None])
@pytest.mark.parametrize("FP,K", CELLS)
def test_weighted_loss_grad_and_holdout_loss(cuda, FP, K, max_wg):
    spec, ds, w, wts, loss64, g64, ho64, bl, bg, _ = eval_reference(FP, K)
    f = BatchFitter(spec, cuda, FitOptions(max_wg=max_wg))
    loss, g = f.loss_grad(ds, w.to(cuda), weights=wts)
    ho = f.holdout_loss(ds, w.to(cuda), wts)
    assert _native.hip_loaded_path() is not None and f._native.weighted
    assert f._native.grid == min(max_wg or 4, 4)
    err = (g.cpu().double() - g64).abs()
    print(f"[FP{FP} K{K} wg{max_wg}] loss err {abs(loss - loss64):.3e} held-out err {abs(ho - ho64):.3e} "
          f"(bound {bl:.3e}) largest grad err/bound {(err / bg.clamp_min(1e-300)).max().item():.3f}")
    assert abs(loss - loss64) <= bl and abs(ho - ho64) <= bl
    assert bool((err <= bg).all())


@pytest.mark.parametrize("max_wg", [3, None])
@pytest.mark.parametrize("FP,K", CELLS)
def test_weighted_sigma(cuda, FP, K, max_wg):
    spec, ds, _, wts, *_, ref = eval_reference(FP, K)
    res = BatchFitter(spec, cuda, FitOptions(max_iter=1, max_wg=max_wg)).fit(ds, weights=wts)
    std = res.std.cpu().double()
    assert float(ref[CONST]) == 0.0 and float(std[CONST]) == 0.0
    assert float(ds.X[:, CONST].float().std()) > 0 and bool((spec.coef(res.w.cpu())[:, CONST] == 0).all())
    print(f"[FP{FP} K{K} wg{max_wg}] largest sigma error {float(((std - ref).abs() / ref.clamp_min(1e-300)).max()):.3e}")
    assert bool(((std - ref).abs() <= 1e-6 * ref).all())


@pytest.mark.parametrize("FP", [1024, 2048])
@pytest.mark.parametrize("N", [100, 4128])
def test_unit_weights_are_the_plain_path(cuda, N, FP):
    spec, ds, w = eval_case(N, FP - 3, 6, seed=1)
    ones = FitWeights(sample_weight=torch.ones(N))
    f = BatchFitter(spec, cuda, FitOptions(max_iter=3, max_wg=3, reg_param=0.01))
    loss, g = f.loss_grad(ds, w.to(cuda))
    assert not f._native.weighted
    loss_w, g_w = f.loss_grad(ds, w.to(cuda), weights=ones)
    assert f._native.weighted and f._native.grid == 3
    assert loss_w == loss and torch.equal(g_w, g)
    a, b = f.fit(ds), f.fit(ds, weights=ones)
    assert torch.equal(a.std, b.std) and torch.equal(a.w, b.w) and a.history == b.history
    assert b.holdout_log_loss is None


@functools.lru_cache(maxsize=None)
def short_fit():
    """The smallest converged case's rows, 8 iterations, weights and fold 0 held out."""
    N, F, K, _ = CONVERGED[0]
    spec, ds, const = fit_case(N, F, K, seed=0)
    wts = draw_weights(N, K, seed=1)
    wts.holdout = 0
    X, y = rows64(spec, ds)
    u, h = effective(wts, y)
    ref = fit_reference(X, y, num_classes=K, reg_param=0.1, tol=0.0, max_iter=8, std=weighted_feature_std(X, u),
                        loss_grad=lambda ce, bb: weighted_loss_grad(X, y, ce, bb, u))
    return spec, ds, wts, ref, float(weighted_loss_grad(X, y, ref.coef, ref.intercept, h)[0])


def check_short_fit(spec, res, ref):
    assert (res.iters, res.reason) == (ref.iters, ref.reason) and len(res.history) == len(ref.history)
    for a, b in zip(res.history, ref.history):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b))
    err = float((spec.coef(res.w.cpu()).double() - ref.coef).abs().max() / ref.coef.abs().max())
    print(f"iters {res.iters} {res.reason} objective {res.objective:.9g} / {ref.objective:.9g} coefficient err {err:.3e}")
    assert err <= 1e-2


def test_short_weighted_fit_matches_the_oracle(cuda):
    spec, ds, wts, ref, ho64 = short_fit()
    res = BatchFitter(spec, cuda, FitOptions(max_iter=8, tol=0.0, reg_param=0.1)).fit(ds, weights=wts)
    check_short_fit(spec, res, ref)
    assert abs(res.holdout_log_loss - ho64) <= 1e-3 * max(1.0, ho64)


def test_zero_weight_equals_removal(cuda):
    spec, ds, wts, ref, _ = short_fit()
    keep = wts.fold != 0
    held = BatchFitter(spec, cuda, FitOptions(max_iter=8, tol=0.0, reg_param=0.1)).fit(
        ds, weights=FitWeights(fold=wts.fold, holdout=0))
    cut = BatchFitter(spec, cuda, FitOptions(max_iter=8, tol=0.0, reg_param=0.1)).fit(
        Dataset(ds.X[keep].clone(), ds.y[keep].clone(), ds.num_features))
    assert (held.iters, held.reason) == (cut.iters, cut.reason)
    for a, b in zip(held.history, cut.history):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b))
    top = float(cut.w.abs().max())
    assert float((held.w - cut.w).abs().max()) <= 1e-2 * top
    assert torch.allclose(held.std, cut.std, rtol=1e-6, atol=0)


def test_lifecycle(cuda):
    spec, ds, wts, _, _ = short_fit()
    f = BatchFitter(spec, cuda, FitOptions(max_iter=5, max_wg=3, reg_param=0.01))
    with pytest.raises(RuntimeError):
        f._native.set_weights()
    a = f.fit(ds, weights=wts)
    assert f._native.weighted
    other = fit_case(100, spec.F, spec.K, seed=4)[1]
    f.fit(other)  # a new dataset clears the weights
    assert not f._native.weighted
    b = f.fit(ds, weights=wts)
    assert a.iters >= 3 and torch.equal(a.w, b.w) and a.history == b.history
    assert a.holdout_log_loss == b.holdout_log_loss

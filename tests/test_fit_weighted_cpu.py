"""Row weights, class weights, a held-out fold and cross-validation of the dense fit on
the CPU path (psx/ops/fit.py over the float64 closures of psx/models/reference.py)."""
import pytest
import torch

from _fit_cases import fit_case, rows64
from psx.models.reference import fit_reference, weighted_feature_std, weighted_loss_grad
from psx.ops.fit import BatchFitter, FitOptions, FitWeights, _Weights, cross_validate

SPEC, DS, _ = fit_case(120, 6, 3, seed=3)
N = DS.rows
FOLD = (torch.arange(N) % 3).to(torch.uint8)


@pytest.mark.parametrize("wts", [
    FitWeights(sample_weight=torch.ones(N - 1)),
    FitWeights(fold=FOLD[:-1], holdout=0),
    FitWeights(class_weight=torch.ones(SPEC.K + 1)),
    FitWeights(class_weight="auto"),
    FitWeights(sample_weight=torch.full((N,), float("nan"))),
    FitWeights(sample_weight=-torch.ones(N)),
    FitWeights(sample_weight=torch.full((N,), 1e-3)),  # W <= 1
    FitWeights(sample_weight=torch.nn.functional.one_hot(torch.tensor(3), N) * 5.0),  # one row of positive weight
    FitWeights(holdout=0),  # no fold ids
    FitWeights(fold=FOLD, holdout=7),  # an empty held-out fold
], ids=range(10))
def test_bad_weights_raise(wts):
    f = BatchFitter(SPEC, "cpu", FitOptions(max_iter=2))
    w = torch.zeros(SPEC.P)
    with pytest.raises(ValueError):
        f.fit(DS, weights=wts)
    with pytest.raises(ValueError):
        f.loss_grad(DS, w, weights=wts)


def test_balanced_is_the_hand_formula():
    w = _Weights(SPEC, DS, FitWeights(class_weight="balanced", fold=FOLD, holdout=2))
    y = DS.y.long()[FOLD != 2]
    cnt = torch.bincount(y, minlength=SPEC.K).double()
    assert bool((cnt > 0).all())
    assert torch.allclose(w.cw.double(), y.numel() / (SPEC.K * cnt), rtol=1e-6)
    assert bool((w.u[FOLD == 2] == 0).all()) and bool((w.h[FOLD != 2] == 0).all())


def test_integer_weights_equal_repeated_rows():
    X, y = rows64(SPEC, DS)
    k = (torch.arange(N) % 3).long()  # 0: dropped, 1, 2: repeated
    u = k.double()
    a = fit_reference(X, y, num_classes=SPEC.K, reg_param=0.05, max_iter=30, std=weighted_feature_std(X, u),
                      loss_grad=lambda ce, bb: weighted_loss_grad(X, y, ce, bb, u))
    rep = torch.repeat_interleave(torch.arange(N), k)
    b = fit_reference(X[rep], y[rep], num_classes=SPEC.K, reg_param=0.05, max_iter=30)
    assert a.iters == b.iters and torch.allclose(a.std, b.std, rtol=1e-12)
    assert torch.allclose(a.coef, b.coef, rtol=1e-7, atol=1e-9) and abs(a.objective - b.objective) <= 1e-12
    res = BatchFitter(SPEC, "cpu", FitOptions(max_iter=30, reg_param=0.05)).fit(
        DS, weights=FitWeights(sample_weight=k.float()))
    assert res.history == a.history and res.holdout_log_loss is None


def test_cross_validate_on_the_cpu():
    regs = [0.0, 0.01, 1.0]
    cv = cross_validate(SPEC, DS, regs, folds=4, seed=1, opts=FitOptions(max_iter=15))
    assert len(cv.losses) == 3 and all(len(r) == 4 for r in cv.losses)
    assert cv.means == [sum(r) / 4 for r in cv.losses]
    assert cv.best_reg_param == regs[cv.means.index(min(cv.means))]
    assert torch.bincount(cv.fold.long()).tolist() == [30, 30, 30, 30]
    f = BatchFitter(SPEC, "cpu", FitOptions(max_iter=15, reg_param=0.01))
    res = f.fit(DS, weights=FitWeights(fold=cv.fold, holdout=2))
    assert res.holdout_log_loss == cv.losses[1][2]
    assert res.holdout_log_loss == f.holdout_loss(DS, res.w, FitWeights(fold=cv.fold, holdout=2))

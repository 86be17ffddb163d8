"""The centred mode of the fp32-row family on the CPU (psx/ops/fit_f32.py): the float64 reference on X - c
with the intercepts mapped back, so that CPU and GPU agree.  The data is the fit of
tests/test_gpu_fit_f32.py with its two signal columns at ``offset`` + N(0,1): uncentred, the float64
reference itself stops at 0.9876 (offset 100) against an optimum of 0.6019."""
import pytest
import torch

from psx.models.logreg import ModelSpec
from psx.models.reference import fit_reference, multinomial_loss_grad
from psx.ops.fit import FitOptions, FitWeights
from psx.ops.fit_f32 import F32Fitter, F32Scorer
from psx.utils.data import Dataset

REG = 0.01


def fit_data(offset):
    """600 x 20 (padded 128), K 4; column 3 constant, the signal in columns 5 and 9 = offset + N(0,1)."""
    N, F, K = 600, 20, 4
    g = torch.Generator().manual_seed(11)
    X = torch.zeros(N, 128)
    X[:, :F] = torch.randn(N, F, generator=g)
    X[:, 3] = 1.5
    a, b = X[:, 5].clone(), X[:, 9].clone()
    X[:, 5] += offset
    X[:, 9] += offset
    y = torch.multinomial(torch.softmax(3.0 * torch.stack([a, -a, b, -b], 1), 1), 1, generator=g).view(-1).to(torch.int32)
    return ModelSpec(F, K), Dataset(X, y, F)


def raw_objective(spec, ds, res):
    """float64 objective of the returned raw (w, b) on the UNCENTRED rows: checks the intercept map."""
    X, w = ds.X[:, : spec.F].double(), res.w.double().cpu()
    W, b = spec.coef(w), spec.intercept(w)
    return float(multinomial_loss_grad(X, ds.y.long(), W, b)[0] + 0.5 * REG * ((W * res.std.double().cpu()) ** 2).sum())


def test_centred_cpu_fit_reaches_the_centred_reference():
    spec, ds = fit_data(100.0)
    X = ds.X[:, : spec.F].double()
    ref = fit_reference(X - X.mean(0), ds.y.long(), num_classes=spec.K, reg_param=REG)
    margin = 1e-3 * max(1.0, abs(ref.objective))
    res = F32Fitter(spec, "cpu", FitOptions(reg_param=REG), center=True).fit(ds)
    assert res.reason == "tol" and abs(res.objective - ref.objective) <= margin
    assert abs(raw_objective(spec, ds, res) - ref.objective) <= margin
    assert res.center.dtype == torch.float32 and float(res.center[3]) == 1.5
    assert torch.allclose(res.center.double(), X.mean(0), rtol=2.0 ** -23, atol=0)
    plain = F32Fitter(spec, "cpu", FitOptions(reg_param=REG)).fit(ds)
    assert plain.objective > 0.9 and plain.center is None  # today's path: stalled far from 0.6019


def test_cpu_scorer_is_the_same_with_a_centre():
    spec, ds = fit_data(1000.0)
    w = spec.init("random", seed=3, scale=0.05)
    a = F32Scorer(spec, ds, "cpu").score(w, proba=True)
    b = F32Scorer(spec, ds, "cpu", center=ds.X[:, : spec.F].mean(0)).score(w, proba=True)
    assert torch.equal(a.pred, b.pred) and torch.equal(a.proba, b.proba) and torch.equal(a.nll, b.nll)


@pytest.mark.parametrize("center", [torch.zeros(19), torch.zeros(20, dtype=torch.float64)])
def test_a_centre_of_the_wrong_length_or_dtype_is_refused(center):
    spec, ds = fit_data(100.0)
    with pytest.raises(ValueError):
        F32Scorer(spec, ds, "cpu", center=center)


def test_centred_fit_has_no_row_weights():
    spec, ds = fit_data(100.0)
    with pytest.raises(NotImplementedError):
        F32Fitter(spec, "cpu", center=True).fit(ds, weights=FitWeights(sample_weight=torch.ones(ds.rows)))

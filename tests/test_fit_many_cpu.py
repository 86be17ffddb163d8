"""fit_many / loss_grad_many without a GPU: a loop over the existing CPU paths, and the
argument checks that come before any launch."""
import pytest
import torch

from _fit_cases import fit_case
from psx.models.wide import WideSpec
from psx.ops.fit import BatchFitter, FitJob, FitOptions, FitWeights, cross_validate
from psx.ops.wide_fit import WideFitter


def case():
    spec, ds, _ = fit_case(120, 8, 3, seed=2)
    g = torch.Generator().manual_seed(1)
    return spec, ds, FitWeights(torch.rand(120, generator=g) + 0.5, None, torch.randint(0, 3, (120,), generator=g))


def test_cpu_fit_many_is_the_loop_of_fit():
    spec, ds, wts = case()
    jobs = [FitJob(0.1, 0), FitJob(0.01, 1), FitJob(0.1, None)]
    f = BatchFitter(spec, "cpu", FitOptions(max_iter=6))
    res = f.fit_many(ds, jobs, wts)
    assert f.opts.reg_param == 0.0
    for j, r in zip(jobs, res):
        one = BatchFitter(spec, "cpu", FitOptions(max_iter=6, reg_param=j.reg_param)).fit(
            ds, weights=FitWeights(wts.sample_weight, None, wts.fold, j.holdout))
        assert torch.equal(r.w, one.w) and torch.equal(r.std, one.std) and r.history == one.history
        assert (r.iters, r.reason, r.holdout_log_loss) == (one.iters, one.reason, one.holdout_log_loss)
    w = torch.stack([r.w for r in res])
    loss, g, ho = f.loss_grad_many(ds, w, wts, [j.holdout for j in jobs])
    assert g.shape == w.shape and float(ho[0]) == res[0].holdout_log_loss and float(ho[2]) == 0.0
    assert float(loss[1]) == f.loss_grad(ds, w[1], weights=FitWeights(wts.sample_weight, None, wts.fold, 1))[0]
    cv = cross_validate(spec, ds, [0.1, 0.01], folds=3, opts=FitOptions(max_iter=6), batch="auto")
    assert cv.losses == cross_validate(spec, ds, [0.1, 0.01], folds=3, opts=FitOptions(max_iter=6)).losses


def test_fit_many_argument_checks():
    spec, ds, wts = case()
    f = BatchFitter(spec, "cpu")
    with pytest.raises(ValueError):
        f.fit_many(ds, [FitJob(0.1, 0)], FitWeights(fold=wts.fold, holdout=1))
    with pytest.raises(ValueError):
        f.fit_many(ds, [], wts)
    with pytest.raises(ValueError):
        f.fit_many(ds, [FitJob(-1.0, 0)], wts)
    with pytest.raises(ValueError):
        f.fit_many(ds, [FitJob(0.1, 0)], None)  # a held-out fold needs fold ids
    with pytest.raises(ValueError):
        WideFitter(WideSpec(64, 3), "cpu").fit_many(ds, [FitJob(0.1, None)], None)
    with pytest.raises(ValueError):
        cross_validate(spec, ds, [0.1], folds=3, batch=0)

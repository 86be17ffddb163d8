"""fit_many / loss_grad_many / cross_validate(batch=) of the wide model without a GPU: the
loop over the existing CPU paths, the argument checks, and the command line."""
import json

import pytest
import torch

from _wide_fit_cases import sparse_case
from psx.apps import fit as fit_app
from psx.ops.fit import FitJob, FitOptions, FitWeights, cross_validate
from psx.ops.wide_fit import WideFitter


def case(K):
    spec, ds = sparse_case(150, 5000, K, seed=3)
    g = torch.Generator().manual_seed(1)
    return spec, ds, FitWeights(torch.rand(150, generator=g) + 0.5, None, torch.randint(0, 3, (150,), generator=g))


@pytest.mark.parametrize("K", [1, 4])
def test_cpu_fit_many_is_the_loop_of_fit(K):
    spec, ds, wts = case(K)
    jobs = [FitJob(0.1, 0), FitJob(0.01, 1), FitJob(0.1, None)]
    f = WideFitter(spec, "cpu", FitOptions(max_iter=5))
    res = f.fit_many(ds, jobs, wts)
    assert f.opts.reg_param == 0.0
    for j, r in zip(jobs, res):
        one = WideFitter(spec, "cpu", FitOptions(max_iter=5, reg_param=j.reg_param)).fit(
            ds, weights=FitWeights(wts.sample_weight, None, wts.fold, j.holdout))
        assert torch.equal(r.w, one.w) and torch.equal(r.std, one.std) and r.history == one.history
        assert torch.equal(r.features, one.features) and r.holdout_log_loss == one.holdout_log_loss
    w = torch.stack([r.w for r in res])
    loss, g, ho = f.loss_grad_many(ds, w, wts, [j.holdout for j in jobs])
    assert float(ho[0]) == res[0].holdout_log_loss and float(ho[2]) == 0.0
    for m, j in enumerate(jobs):
        l1, g1 = f.loss_grad(ds, w[m], weights=FitWeights(wts.sample_weight, None, wts.fold, j.holdout))
        assert float(loss[m]) == l1 and torch.equal(g[m], g1)


def test_cross_validate_batched_equals_sequential_on_the_cpu():
    spec, ds, _ = case(1)
    kw = dict(folds=3, seed=1, opts=FitOptions(max_iter=5))
    assert cross_validate(spec, ds, [0.1, 0.01], batch="auto", **kw).losses == cross_validate(spec, ds, [0.1, 0.01], **kw).losses


def test_fit_many_argument_checks():
    spec, ds, wts = case(4)
    f = WideFitter(spec, "cpu")
    with pytest.raises(ValueError):
        f.fit_many(ds, [FitJob(0.1, 0)], FitWeights(fold=wts.fold, holdout=1))  # a shared holdout
    with pytest.raises(ValueError):
        f.fit_many(ds, [], wts)
    with pytest.raises(ValueError):
        f.fit_many(ds, [FitJob(-1.0, 0)], wts)
    with pytest.raises(ValueError):
        f.fit_many(ds, [FitJob(0.1, 0), FitJob(0.1, 1)], FitWeights(class_weight="balanced", fold=wts.fold))


def test_fit_app_batches_a_libsvm_cross_validation(tmp_path, capsys):
    _, ds = sparse_case(60, 200, 1, seed=5)
    path = tmp_path / "train.svm"
    with open(path, "w") as fh:
        for r in range(ds.rows):
            a, b = int(ds.indptr[r]), int(ds.indptr[r + 1])
            cells = {}  # (a LIBSVM row lists an id once: repeated ids summed)
            for i, v in zip(ds.idx[a:b].tolist(), ds.val[a:b].float().tolist()):
                cells[i] = cells.get(i, 0.0) + v
            fh.write(f"{int(ds.y[r])} " + " ".join(f"{i + 1}:{v!r}" for i, v in sorted(cells.items())) + "\n")
    assert fit_app.main(["--train", str(path), "--device", "cpu", "--max_iter", "5", "--num_features", "200", "--sigmoid",
                         "--cv", "3", "--reg_params", "0.01,1", "--cv_batch", "auto"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["cv_folds"] == 3 and line["reg_param"] in (0.01, 1.0)

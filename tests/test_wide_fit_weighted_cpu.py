"""Row weights, a held-out fold and cross-validation of the wide fit on the CPU path:
the weighted closures and sigma of psx/ops/wide_fit.py against the dense float64
oracles of psx/models/reference.py, the front end, and the command line."""
import json

import pytest
import torch

from _wide_fit_cases import csr64, sparse_case
from psx.apps import fit as fit_app
from psx.models.reference import weighted_feature_std, weighted_loss_grad
from psx.ops.fit import FitOptions, FitWeights, _Weights, cross_validate
from psx.ops.wide_fit import WideFitter, _closures, _Index


def weights_for(N, K, seed=0):
    g = torch.Generator().manual_seed(977 + seed)
    sw = torch.rand(N, generator=g) * 2
    sw[torch.rand(N, generator=g) < 0.1] = 0.0
    sw[64:96] = 0.0
    fold = torch.randint(0, 3, (N,), generator=g).to(torch.uint8)
    return FitWeights(sw, 0.5 + torch.rand(max(K, 2), generator=g), fold, 1)


@pytest.mark.parametrize("K", [1, 4])
def test_weighted_closures_and_sigma_match_the_dense_oracles(K):
    spec, ds = sparse_case(150, 5000, K, seed=3)
    u = _Weights(spec, ds, weights_for(150, K)).u
    ix = _Index(spec, ds, "cpu")
    fg, sd = _closures(ix, K, u)
    f = ix.uniq.long()
    X, y = csr64(ds)[:, f], ds.y.long()
    g = torch.Generator().manual_seed(1)
    ce, b = torch.randn(K, f.numel(), generator=g, dtype=torch.float64) * 0.1, torch.randn(K, generator=g).double()
    for got, ref in zip(fg(ce, b), weighted_loss_grad(X, y, ce, b, u)):
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    ref = weighted_feature_std(X, u)
    assert float(sd[0]) == 0.0 and bool(((sd == 0) == (ref == 0)).all()) and int((ref == 0).sum()) > 1
    assert bool(((sd - ref).abs() <= 1e-12 * ref).all())


def test_weighted_fit_and_cross_validate_on_the_cpu():
    spec, ds = sparse_case(150, 5000, 1, seed=3)
    wts = weights_for(150, 1)
    f = WideFitter(spec, "cpu", FitOptions(max_iter=5, reg_param=0.1))
    res = f.fit(ds, weights=wts)
    assert res.iters >= 1 and res.holdout_log_loss > 0
    assert res.holdout_log_loss == f.holdout_loss(ds, res.w, wts)
    assert f.loss_grad(ds, res.w, weights=wts)[0] == pytest.approx(res.log_loss, rel=1e-6)
    regs = [0.01, 1.0]
    cv = cross_validate(spec, ds, regs, folds=3, seed=1, opts=FitOptions(max_iter=5), class_weight="balanced")
    assert [len(r) for r in cv.losses] == [3, 3] and cv.best_reg_param == regs[cv.means.index(min(cv.means))]
    one = WideFitter(spec, "cpu", FitOptions(max_iter=5, reg_param=1.0)).fit(
        ds, weights=FitWeights(class_weight="balanced", fold=cv.fold, holdout=2))
    assert one.holdout_log_loss == cv.losses[1][2]


@pytest.mark.parametrize("extra", [["--class_weight", "balanced"], ["--sigmoid", "--class_weight", "1,3"],
                                   ["--cv", "3", "--reg_params", "0.01,1"]], ids=["balanced", "table", "cv"])
def test_fit_app_takes_weights_and_cv_with_libsvm_rows(tmp_path, capsys, extra):
    _, ds = sparse_case(60, 200, 1, seed=5)
    path = tmp_path / "train.svm"
    with open(path, "w") as fh:
        for r in range(ds.rows):
            a, b = int(ds.indptr[r]), int(ds.indptr[r + 1])
            cells = {}  # (a LIBSVM row lists an id once: repeated ids summed)
            for i, v in zip(ds.idx[a:b].tolist(), ds.val[a:b].float().tolist()):
                cells[i] = cells.get(i, 0.0) + v
            fh.write(f"{int(ds.y[r])} " + " ".join(f"{i + 1}:{v!r}" for i, v in sorted(cells.items())) + "\n")
    assert fit_app.main(["--train", str(path), "--device", "cpu", "--max_iter", "5", "--num_features", "200"]
                        + extra) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["rows"] == 60 and line["iterations"] >= 1
    if "--cv" in extra:
        assert line["cv_folds"] == 3 and line["reg_param"] in (0.01, 1.0)

"""The wide full-batch fit without a GPU: the float64 sparse closures against the
dense oracle, fit_reference's two keywords and its one-logit guard, the CPU path of
psx.ops.wide_fit.WideFitter (result layout, checkpoint round trip, validation, the
errors) and the LIBSVM branch of python -m psx.apps.fit."""
import json
import os
import subprocess
import sys

import pytest
import torch

from _wide_fit_cases import (check_validation, csr64, dense_touched, oracle_fit, sparse_case, touched, warm_start)
from psx.models.logreg import ModelSpec
from psx.models.reference import feature_std, fit_reference, multinomial_loss_grad
from psx.models.wide import WideSpec
from psx.ops.fit import FitOptions
from psx.ops.score import Scorer
from psx.ops.sparse import SparseDataset
from psx.ops.wide_fit import WideFitter, _closures, _Index, wide_loss_grad
from psx.utils.data import Dataset, save_libsvm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K", [1, 6])
def test_sparse_closures_equal_the_dense_oracle(K):
    spec, ds = sparse_case(229, 5000, K, seed=1)
    assert int(ds.indptr[1] - ds.indptr[0]) > int(torch.unique(ds.idx[: int(ds.indptr[1])]).numel())  # a repeated id
    ix = _Index(spec, ds, torch.device("cpu"))
    fg, sd = _closures(ix, K)
    f, X = dense_touched(ds)
    assert torch.equal(ix.uniq.long(), f)
    assert torch.allclose(sd, feature_std(X), rtol=0, atol=1e-12)
    assert float(sd[0]) == 0.0  # feature 0 is 1.5 in every row: exactly excluded
    g = torch.Generator().manual_seed(3)
    ce = torch.randn(K, f.numel(), generator=g, dtype=torch.float64) * 0.3
    b = torch.randn(K, generator=g, dtype=torch.float64)
    loss, gc, gb = fg(ce, b)
    loss64, gc64, gb64 = multinomial_loss_grad(X, ds.y.long(), ce, b)
    assert abs(float(loss) - float(loss64)) <= 1e-12
    assert float((gc - gc64).abs().max()) <= 1e-12 and float((gb - gb64).abs().max()) <= 1e-12


@pytest.mark.parametrize("K,lam", [(1, 0.05), (6, 0.0), (6, 0.05)])
def test_fit_reference_with_closures_equals_the_dense_call(K, lam):
    spec, ds = sparse_case(229, 5000, K, seed=2)
    f, X = dense_touched(ds)
    fg, sd = _closures(_Index(spec, ds, torch.device("cpu")), K)
    kw = dict(reg_param=lam, max_iter=25, tol=1e-9)
    dense = fit_reference(X, ds.y.long(), num_classes=K, **kw)
    sparse = fit_reference(None, ds.y, torch.zeros(K, f.numel(), dtype=torch.float64), None, loss_grad=fg, std=sd,
                           **kw)
    assert (sparse.iters, sparse.reason) == (dense.iters, dense.reason) and dense.iters >= 5
    assert abs(sparse.objective - dense.objective) <= 1e-10


def test_the_one_logit_oracle_is_not_centred():
    spec, ds = sparse_case(600, 5000, 1, seed=2)
    _, ref = oracle_fit(spec, ds, reg_param=0.1, max_iter=30)
    assert ref.iters >= 3 and float(ref.coef.abs().max()) > 0 and float(ref.intercept.abs().max()) > 0


def test_cpu_fitter_result_checkpoint_and_scores(tmp_path):
    spec, ds = sparse_case(300, 5000, 4, seed=3)
    res = WideFitter(spec, "cpu", FitOptions(max_iter=20, reg_param=0.05)).fit(ds)
    f, ref = oracle_fit(spec, ds, reg_param=0.05, max_iter=20)
    assert (res.iters, res.reason) == (ref.iters, ref.reason) and abs(res.objective - ref.objective) <= 1e-10
    assert torch.equal(res.features.long(), f) and res.std.shape == (f.numel(),)
    assert res.w.shape == (spec.P,)
    coef = spec.coef(res.w)
    out = torch.ones(spec.F, dtype=torch.bool)
    out[f] = False
    assert bool((coef[:, out] == 0).all())  # zero outside the touched features
    assert float(res.std[0]) == 0.0 and int(res.features[0]) == 0 and bool((coef[:, 0] == 0).all())
    assert torch.allclose(coef[:, f].double(), ref.coef, rtol=1e-6, atol=1e-9)  # fp32 storage of the same fit
    sc = Scorer(spec, res.w, "cpu").score(ds)
    res.save(str(tmp_path))
    state = torch.load(str(tmp_path / "server.ckpt"), weights_only=True)
    assert state["model"] == "wide" and "w_reference_layout" not in state
    again = Scorer.from_checkpoint(str(tmp_path), "cpu")
    assert again.wide and again.spec == spec
    sc2 = again.score(ds)
    assert (sc2.accuracy, sc2.f1, sc2.log_loss) == (sc.accuracy, sc.f1, sc.log_loss)
    assert torch.equal(sc2.confusion, sc.confusion)


def test_cpu_loss_grad_is_zero_on_untouched_features():
    spec, ds = sparse_case(40, 5000, 3, seed=4, full_cols=False)
    w = warm_start(spec, seed=1)
    loss, g = wide_loss_grad(spec, ds, w, "cpu")
    X = csr64(ds)
    loss64, gc, gb = multinomial_loss_grad(X, ds.y.long(), spec.coef(w).double(), spec.intercept(w).double())
    assert abs(loss - float(loss64)) <= 1e-9
    assert float((g.double() - spec.pack(gc, gb).double()).abs().max()) <= 1e-6
    out = torch.ones(spec.F, dtype=torch.bool)
    out[touched(ds)] = False
    assert bool((spec.coef(g)[:, out] == 0).all())


def test_cpu_warm_start_keeps_excluded_coefficients_when_asked():
    spec, ds = sparse_case(120, 5000, 3, seed=5)
    w0 = warm_start(spec, seed=2)
    keep = WideFitter(spec, "cpu", FitOptions(max_iter=3, reg_param=0.05, zero_const=False)).fit(ds, w0=w0)
    drop = WideFitter(spec, "cpu", FitOptions(max_iter=3, reg_param=0.05)).fit(ds, w0=w0)
    out = torch.ones(spec.F, dtype=torch.bool)
    out[touched(ds)] = False
    assert torch.equal(spec.coef(keep.w)[:, out], spec.coef(w0)[:, out]) and bool((spec.coef(drop.w)[:, out] == 0).all())
    assert torch.equal(spec.coef(keep.w)[:, 0], spec.coef(w0)[:, 0])  # feature 0 is constant: excluded too


def test_cpu_validation():
    check_validation("cpu")


def test_errors_are_value_errors():
    spec, ds = sparse_case(40, 5000, 3, seed=6)
    f = WideFitter(spec, "cpu")
    with pytest.raises(ValueError, match="sparse rows"):
        f.fit(Dataset(torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.int32), 100))
    with pytest.raises(ValueError, match="feature"):
        WideFitter(WideSpec(100, 3), "cpu").fit(ds)
    wide_ids = SparseDataset(ds.indptr, ds.idx.clone(), ds.val, ds.y, 50)
    with pytest.raises(ValueError, match="feature ids"):
        WideFitter(WideSpec(50, 3), "cpu").fit(wide_ids)
    bad_y = SparseDataset(ds.indptr, ds.idx, ds.val, ds.y + 1, ds.num_features)
    with pytest.raises(ValueError, match="labels"):
        f.fit(bad_y)
    two = SparseDataset(ds.indptr, ds.idx, ds.val, torch.full_like(ds.y, 2), ds.num_features)
    with pytest.raises(ValueError, match="labels"):
        WideFitter(WideSpec(5000, 1), "cpu").fit(two)
    with pytest.raises(ValueError, match="at least 2"):
        f.fit(ds.slice(0, 1))
    with pytest.raises(ValueError, match="col_chunk"):
        WideFitter(spec, "cpu", col_chunk=0)
    with pytest.raises(ValueError, match="WideSpec"):
        WideFitter(ModelSpec(100, 3), "cpu")
    with pytest.raises(ValueError, match="weights"):
        f.fit(ds, w0=torch.zeros(7))


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "psx.apps.fit", *args], capture_output=True, text=True, env=env,
                          cwd=ROOT, timeout=300)


def test_cli_fits_a_libsvm_file(tmp_path):
    spec, ds = sparse_case(200, 5000, 4, seed=7)
    # LIBSVM labels are the classes themselves; ids are written one-based
    path = str(tmp_path / "train.svm")
    save_libsvm(ds, path)
    out = _cli("--train", path, "--num_features", "5000", "--reg_param", "0.05", "--max_iter", "10", "--device", "cpu",
               "--valid_frac", "0.2", "--test", path, "--checkpoint_dir", str(tmp_path / "ck"))
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    for key in ("rows", "features", "classes", "iterations", "evaluations", "reason", "objective", "train_log_loss",
                "touched_features", "valid_rows", "best_iteration", "test_accuracy", "fit_seconds"):
        assert key in line, key
    assert line["features"] == 5000 and line["classes"] == 4 and line["rows"] == 160
    assert 0 < line["touched_features"] <= touched(ds).numel()
    assert Scorer.from_checkpoint(str(tmp_path / "ck"), "cpu").wide
    # a warm start from that checkpoint, and the stray-argument / help exits
    again = _cli("--train", path, "--num_features", "5000", "--max_iter", "2", "--device", "cpu", "--init_checkpoint",
                 str(tmp_path / "ck"))
    assert again.returncode == 0, again.stderr
    assert _cli("--train", path, "stray").returncode == 2
    assert _cli("-h").returncode == 0
    assert _cli("--train", str(tmp_path / "rows.csv"), "--sigmoid").returncode == 2


def test_cli_sigmoid(tmp_path):
    spec, ds = sparse_case(200, 5000, 1, seed=8)
    path = str(tmp_path / "train.svm")
    save_libsvm(ds, path)
    out = _cli("--train", path, "--sigmoid", "--reg_param", "0.05", "--max_iter", "5", "--device", "cpu")
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["classes"] == 1 and line["iterations"] >= 1 and line["touched_features"] > 0

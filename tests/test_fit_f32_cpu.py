"""The fp32-row family without a GPU: spec and dtype errors, what is not implemented, the CPU
(float64 reference) paths of F32Fitter / f32_score on the fp32 rows as stored, and the checkpoint."""
import pytest
import torch

from psx.models.logreg import ModelSpec, from_reference_layout
from psx.models.reference import fit_reference, multinomial_loss_grad
from psx.ops.fit import FitJob, FitOptions, FitWeights
from psx.ops.fit_f32 import F32Fitter, F32Scorer, f32_score
from psx.ops.panel_fit import PanelSpec
from psx.utils.checkpoint import CKPT_NAME
from psx.utils.data import Dataset

N, F, K = 60, 20, 3


@pytest.fixture(scope="module")
def small():
    g = torch.Generator().manual_seed(3)
    X = torch.zeros(N, 128)
    X[:, :F] = torch.randn(N, F, generator=g)
    X[:, 4] = 1.5
    X[:, 7] += 100.0  # bf16 cannot hold this column
    y = torch.randint(0, K, (N,), generator=g).to(torch.int32)
    spec = ModelSpec(F, K)
    w = spec.pack(torch.randn(K, F, generator=g) * 0.05, torch.randn(K, generator=g) * 0.5)
    return spec, Dataset(X, y, F), w, X[:, :F].double(), y.long()


def test_spec_and_dtype_errors(small):
    spec, ds, w, _, _ = small
    with pytest.raises(ValueError, match="BatchFitter"):
        F32Fitter(spec, "cpu").loss_grad(ds.as_dtype("bf16"), w)
    with pytest.raises(ValueError, match="BatchFitter"):
        F32Scorer(spec, ds.as_dtype("bf16"), "cpu")
    with pytest.raises(ValueError, match="1024"):
        F32Fitter(ModelSpec(2000, K), "cpu")
    with pytest.raises(ValueError, match="ModelSpec"):
        F32Fitter(PanelSpec(2100, K), "cpu")


def test_not_implemented(small):
    spec, ds, w, _, _ = small
    f = F32Fitter(spec, "cpu")
    wts = FitWeights(sample_weight=torch.ones(N))
    for call in (lambda: f.fit(ds, weights=wts), lambda: f.loss_grad(ds, w, weights=wts),
                 lambda: f.fit_many(ds, [FitJob(0.1)]), lambda: f.loss_grad_many(ds, w.view(1, -1), None, [None]),
                 lambda: f.holdout_loss(ds, w, wts), lambda: f.cross_validate(ds, [0.1]),
                 lambda: f32_score(spec, w, ds, "cpu", curves=True)):
        with pytest.raises(NotImplementedError):
            call()


def test_cpu_paths_equal_the_reference(small, tmp_path):
    spec, ds, w, X, y = small
    loss, gc, gb = multinomial_loss_grad(X, y, spec.coef(w).double(), spec.intercept(w).double())
    f = F32Fitter(spec, "cpu", FitOptions(reg_param=0.01, max_iter=5))
    got_loss, g = f.loss_grad(ds, w)
    assert got_loss == float(loss) and torch.equal(g, spec.pack(gc, gb))
    ref = fit_reference(X, y, num_classes=K, reg_param=0.01, max_iter=5)
    res, resv = f.fit(ds), f.fit(ds, valid=ds)
    assert res.objective == ref.objective and res.iters == ref.iters and float(res.std[4]) == 0.0
    assert torch.equal(res.w, spec.pack(ref.coef, ref.intercept)) and len(resv.valid_history) == res.iters
    assert res.objective != fit_reference(X.to(torch.bfloat16).double(), y, num_classes=K, reg_param=0.01,
                                          max_iter=5).objective  # (not the rounded rows)
    sc = f32_score(spec, res.w, ds, "cpu", proba=True)
    z = X @ spec.coef(res.w).double().t() + spec.intercept(res.w).double()
    assert torch.equal(sc.pred.long(), z.argmax(1)) and sc.rows == N and int(sc.confusion.sum()) == N
    assert sc.log_loss == pytest.approx(float(torch.nn.functional.cross_entropy(z, y)), rel=1e-6)
    assert sc.log_loss == resv.valid_history[-1][1]
    # the ordinary dense checkpoint, which carries the reference layout
    state = torch.load(res.save(str(tmp_path)), weights_only=True)
    assert state["model"] == "dense" and state["num_features"] == F and state["w_reference_layout"].numel() == spec.P_ref
    assert torch.equal(from_reference_layout(spec, state["w_reference_layout"]), res.w)
    assert (tmp_path / CKPT_NAME).exists()

"""The panel family without a GPU: PanelSpec's widths and errors, what is not implemented,
the CPU (float64 reference) paths of PanelFitter / panel_score, and the checkpoint layout."""
import pytest
import torch

from psx.models.logreg import from_reference_layout
from psx.models.reference import fit_reference, multinomial_loss_grad
from psx.ops.fit import FitJob, FitOptions, FitWeights, cross_validate
from psx.ops.panel_fit import PanelFitter, PanelSpec, panel_dataset, panel_score
from psx.utils.checkpoint import CKPT_NAME

N, F, K = 60, 2100, 3


@pytest.fixture(scope="module")
def small():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, F, generator=g)
    x[:, 2070] = 1.5
    y = torch.randint(0, K, (N,), generator=g)
    spec = PanelSpec(F, K)
    w = spec.pack(torch.randn(K, F, generator=g) * 0.05, torch.randn(K, generator=g) * 0.5)
    return spec, panel_dataset(x, y), w, x.to(torch.bfloat16).double(), y


@pytest.mark.parametrize("F_,Fp", [(2049, 4096), (4096, 4096), (4097, 8192), (8193, 16384), (16384, 16384)])
def test_spec_widths(F_, Fp):
    s = PanelSpec(F_, 6)
    assert (s.F, s.K, s.Fp, s.P, s.P_ref) == (F_, 6, Fp, 6 * Fp + 6, 6 * F_ + 6)
    w = s.init("random", seed=1)
    assert w.numel() == s.P and s.coef(w).shape == (6, F_) and s.intercept(w).shape == (6,)


def test_spec_errors():
    with pytest.raises(ValueError, match="ModelSpec.*BatchFitter"):
        PanelSpec(2048, 6)
    with pytest.raises(ValueError, match="16384"):
        PanelSpec(16385, 6)


def test_not_implemented(small):
    spec, ds, w, _, _ = small
    f = PanelFitter(spec, "cpu")
    wts = FitWeights(sample_weight=torch.ones(N))
    for call in (lambda: f.fit(ds, weights=wts), lambda: f.loss_grad(ds, w, weights=wts),
                 lambda: f.fit_many(ds, [FitJob(0.1)]), lambda: f.loss_grad_many(ds, w.view(1, -1), None, [None]),
                 lambda: cross_validate(spec, ds, [0.1], folds=2), lambda: panel_score(spec, w, ds, "cpu", curves=True)):
        with pytest.raises(NotImplementedError):
            call()


def test_cpu_paths_equal_the_reference(small, tmp_path):
    spec, ds, w, X, y = small
    assert tuple(ds.X.shape) == (64, 4096) and ds.rows == N
    loss, gc, gb = multinomial_loss_grad(X, y, spec.coef(w).double(), spec.intercept(w).double())
    f = PanelFitter(spec, "cpu", FitOptions(reg_param=0.01, max_iter=5))
    got_loss, g = f.loss_grad(ds, w)
    assert got_loss == float(loss) and torch.equal(g, spec.pack(gc, gb))
    ref = fit_reference(X, y, num_classes=K, reg_param=0.01, max_iter=5)
    res, resv = f.fit(ds), f.fit(ds, valid=ds)
    assert res.objective == ref.objective and res.iters == ref.iters and float(res.std[2070]) == 0.0
    assert torch.equal(res.w, spec.pack(ref.coef, ref.intercept)) and len(resv.valid_history) == res.iters
    sc = panel_score(spec, res.w, ds, "cpu", proba=True)
    z = X @ spec.coef(res.w).double().t() + spec.intercept(res.w).double()
    assert torch.equal(sc.pred.long(), z.argmax(1)) and sc.rows == N and int(sc.confusion.sum()) == N
    assert sc.log_loss == pytest.approx(float(torch.nn.functional.cross_entropy(z, y)), rel=1e-6)
    assert sc.log_loss == resv.valid_history[-1][1]
    # the checkpoint carries the reference layout
    state = torch.load(res.save(str(tmp_path)), weights_only=True)
    assert state["num_features"] == F and state["w_reference_layout"].numel() == spec.P_ref
    assert torch.equal(from_reference_layout(spec, state["w_reference_layout"]), res.w)
    assert (tmp_path / CKPT_NAME).exists()

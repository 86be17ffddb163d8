"""Panel fit and scorer on MI355X (csrc/kernels/panel_fit.hip, csrc/solver/panel_fit.hip)
against float64 on the bf16-rounded rows.

One evaluation is held to the derived bound of tests/_fit_cases.py (``eval_oracle``), the
check tests/test_gpu_fit.py applies to the same quantity, and to a sharper form of it.  That
bound charges a margin (F + 8) fp32 roundings, a sequential sum over the features, which at
16,384 features allows a loss error of 1.0: it could not tell a missing panel.  The panel
kernels sum a margin in a tree of fixed depth instead -- 8 products inside one MFMA, the 16
MFMAs (8 k-steps x hi/lo) of a wave's slice, 4 waves, at most 16 panels -- so DEPTH = 44
replaces F + 8 in dz_r; everything else is the derivation of tests/_fit_cases.py unchanged.
The sharper bound is below the inherited one wherever F + 8 > 44 and both are asserted.
Measured on an MI355X (profiles/r22/README.md): the largest loss error is 0.012 of the sharper
bound, the largest gradient error 0.007 of it.  The scorer's per-row bounds use the same dz_r:
a probability moves by at most dz_r + 1e-6, a row's loss by 2 dz_r + 1e-6 max|z|.  The fit
uses the objective criterion of the dense fits (1e-3 relative)."""
import pytest
import torch

from _fit_cases import U18, U24, eval_oracle
from psx.models.reference import fit_reference
from psx.ops.fit import FitOptions
from psx.ops.panel_fit import PanelFitter, PanelSpec, panel_dataset, panel_score
from psx.utils.data import Dataset

pytestmark = pytest.mark.gpu

WIDTHS = [(2049, 4096), (4096, 4096), (5000, 8192), (16384, 16384)]  # first past the old limit (a panel that is
# all padding), full, a partial last panel, the top
ROWS = [(1, None), (33, None), (200, 3)]  # one row; a ragged second tile; several tiles per workgroup


def case(N, F, K, seed=0, wscale=0.05, const=None):
    """X ~ N(0,1) with a constant column (the last feature unless given), non-zero weights and intercepts."""
    g = torch.Generator().manual_seed(7919 * N + 31 * F + K + seed)
    x = torch.randn(N, F, generator=g)
    x[:, F - 1 if const is None else const] = 1.5
    y = torch.randint(0, K, (N,), generator=g)
    spec = PanelSpec(F, K)
    w = spec.pack(torch.randn(K, F, generator=g) * wscale, torch.randn(K, generator=g) * 0.5)
    return spec, panel_dataset(x, y), w


DEPTH = 8 + 16 + 4 + 16  # fp32 roundings on a margin's path through the panel kernels (module docstring)


def margin_err(X, W, b):
    return (U18 + DEPTH * U24) * (X.abs() @ W.abs().t() + b.abs()).max(1).values  # dz_r


def sharp_bounds(spec, ds, w):
    """eval_oracle's (|dloss|, |dg|) bounds with DEPTH for F + 8."""
    N, F = ds.rows, spec.F
    X, y = ds.X[:N, :F].double(), ds.y[:N].long()
    W, b = spec.coef(w).double(), spec.intercept(w).double()
    z = X @ W.t() + b
    R = torch.softmax(z, 1)
    R[torch.arange(N), y] -= 1.0
    nll = torch.logsumexp(z, 1) - z.gather(1, y.view(-1, 1)).view(-1)
    dz = margin_err(X, W, b)
    per_row, rows = dz + 1e-6 + U18, (N + 8) * U24 / N
    bg = torch.zeros(spec.K, spec.Fp, dtype=torch.float64)
    bg[:, :F] = (per_row @ X.abs()) / N + rows * (R.abs().t() @ X.abs())
    bl = float((2 * dz + 1e-6 * max(1.0, float(z.abs().max()))).mean() + (N + 8) * U24 * nll.abs().mean())
    return bl, torch.cat([bg.reshape(-1), per_row.mean() + rows * R.abs().sum(0)])


def plain(ds):
    return Dataset(ds.X[: ds.rows], ds.y[: ds.rows], ds.num_features)


@pytest.mark.parametrize("N,max_wg", ROWS)
@pytest.mark.parametrize("K", [2, 6, 16])
@pytest.mark.parametrize("F,FP", WIDTHS)
def test_loss_grad_within_the_derived_bound(cuda, F, FP, K, N, max_wg):
    spec, ds, w = case(N, F, K)
    assert spec.Fp == FP and tuple(ds.X.shape) == ((N + 31) // 32 * 32, FP)
    loss64, g64, bl0, bg0, _ = eval_oracle(spec, plain(ds), w)
    bl, bg = sharp_bounds(spec, ds, w)
    assert bl <= bl0 and bool((bg <= bg0).all())
    f = PanelFitter(spec, cuda, FitOptions(max_wg=max_wg))
    loss, g = f.loss_grad(ds, w)
    g = g.cpu().double()
    err = (g - g64).abs()
    print(f"[{N}x{F} K{K} wg{max_wg}] grid {f._native.grid} loss err {abs(loss - loss64):.3e} (bound {bl:.3e}, "
          f"inherited {bl0:.3e}) largest grad err/bound {(err / bg.clamp_min(1e-300)).max().item():.3f}")
    assert f._native.grid == min((N + 31) // 32, max_wg or 1 << 30)
    assert bool(torch.isfinite(g).all()) and abs(loss - loss64) <= bl
    assert bool((err <= bg).all())
    assert bool((g[: K * FP].view(K, FP)[:, F:] == 0).all())  # padding features


def test_evaluations_are_bit_reproducible(cuda):
    spec, ds, w = case(200, 5000, 6)
    f = PanelFitter(spec, cuda, FitOptions(max_wg=3))
    a = f.loss_grad(ds, w)
    b = f.loss_grad(ds, w)
    assert a[0] == b[0] and torch.equal(a[1], b[1])


def test_fit_reaches_the_reference_objective(cuda, tmp_path):
    N, F, K = 256, 2100, 3
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, F, generator=g) * (0.2 + 4.8 * torch.rand(F, generator=g)) + torch.randn(F, generator=g)
    x[:, 2070] = 1.5  # constant, in the last live panel
    y = torch.multinomial(torch.softmax(x[:, :K] * 2.0, 1), 1, generator=g).view(-1)
    spec, ds = PanelSpec(F, K), panel_dataset(x, y)
    ref = fit_reference(ds.X[:N, :F].double(), y, num_classes=K, reg_param=0.01)
    res = PanelFitter(spec, cuda, FitOptions(reg_param=0.01)).fit(ds)
    print(f"fit: iters {res.iters} evals {res.evals} reason {res.reason} objective {res.objective:.9g} "
          f"(reference {ref.iters}, {ref.reason}, {ref.objective:.9g})")
    assert res.reason in ("tol", "max_iter")
    assert abs(res.objective - ref.objective) <= 1e-3 * max(1.0, abs(ref.objective))
    assert float(res.std[2070]) == 0.0 and bool((spec.coef(res.w.cpu())[:, 2070] == 0).all())
    assert torch.allclose(res.std.cpu().double(), ref.std, rtol=1e-6, atol=0)
    again = PanelFitter(spec, cuda, FitOptions(reg_param=0.01)).fit(ds)
    assert torch.equal(again.w, res.w) and again.history == res.history


def test_score_outputs(cuda):
    N, F, K = 70, 5000, 6
    spec, ds, w = case(N, F, K)
    ds.y[5] = 9  # outside [0, K)
    X, yl = ds.X[:N, :F].double(), ds.y[:N].long()
    W, b = spec.coef(w).double(), spec.intercept(w).double()
    z = X @ W.t() + b
    top = z.topk(2, 1).values
    dz = margin_err(X, W, b)
    assert bool((top[:, 0] - top[:, 1] > 2 * dz).all())  # no prediction hangs on the rounding
    ok = (yl >= 0) & (yl < K)
    nll = torch.logsumexp(z, 1) - z.gather(1, yl.clamp(0, K - 1).view(-1, 1)).view(-1)
    conf = torch.zeros(16, 16, dtype=torch.int64)
    conf.view(-1).index_add_(0, yl.clamp(0, 15) * 16 + z.argmax(1), torch.ones(N, dtype=torch.int64))
    r = panel_score(spec, w, ds, cuda, proba=True)
    assert torch.equal(r.pred.cpu().long(), z.argmax(1))
    perr = (r.proba.cpu().double() - torch.softmax(z, 1)).abs().max(1).values
    got = r.nll.cpu().double()
    nerr = (got - nll).abs()[ok]
    print(f"score: largest proba err/bound {(perr / (dz + 1e-6)).max().item():.3f}, "
          f"nll {(nerr / (2 * dz + 1e-6 * z.abs().max())[ok]).max().item():.3f}")
    assert bool((perr <= dz + 1e-6).all())
    assert bool((nerr <= (2 * dz + 1e-6 * z.abs().max())[ok]).all()) and bool(torch.isnan(got[5]))
    assert torch.equal(r.confusion, conf[:K, :K]) and r.rows_out_of_range == 1 and r.rows == N
    assert abs(r.log_loss - float(nll[ok].mean())) <= float((2 * dz + 1e-6 * z.abs().max()).max())
    assert r.accuracy == pytest.approx(float((z.argmax(1) == yl).sum()) / (N - 1))  # over the rows of the K x K cells
    with pytest.raises(NotImplementedError):
        panel_score(spec, w, ds, cuda, curves=True)

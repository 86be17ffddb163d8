"""Centred mode of the fp32-row family on MI355X (fit_lossgrad_f32_kernel<FP, true>, score_f32_kernel<FP, true>
and the three vector kernels of csrc/kernels/fit_f32.hip) against float64.

The kernels multiply x - c_f, so one evaluation is held to the derivation of tests/test_gpu_fit_f32.py on the
CENTRED rows, ``oracle(spec, X64 - c, y, w')`` with ``b' = b + W c`` in float64, times 1.01: the subtraction is one
more fp32 rounding, 2^-24 against the 3 * 2^-18 already charged per element (1/192).  In the 100 + N(0,1) column
that bound is about 100 times tighter than the uncentred one.  The raw gradient is g'_w + c_f g_b formed in fp64 and
rounded once: the centred bound plus |c_f| bound(g_b) + 2^-23 |g64|.  Fits: the dense fits' criterion against the
float64 reference on X - mean, 0.601921 / 0.601922 in 11 iterations (uncentred: 0.9876 and 1.3856).

Measured on an MI355X (profiles/r24/README.md), largest error / bound: with 200 rows loss 0.002, centred gradient
0.038 and raw gradient 0.036; with 33 rows 0.014, 0.164 and 0.145; with ONE row (every column constant, the staged
tile exactly zero) 0.042, 0.005 and 0.010."""
import pytest
import torch

from psx.models.reference import fit_reference
from psx.ops.fit import FitOptions
from psx.ops.fit_f32 import F32Fitter, f32_score
from test_fit_f32_center_cpu import REG, fit_data, raw_objective
from test_gpu_fit_f32 import ROWS, case, margin_err, oracle, rows64

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,max_wg", ROWS)
@pytest.mark.parametrize("K", [2, 16])
@pytest.mark.parametrize("FP", [128, 512, 1024])
def test_centred_evaluation_within_the_derived_bound(cuda, FP, K, N, max_wg):
    spec, ds, w = case(N, FP, K)
    F, KF = spec.F, K * FP
    X, y = rows64(spec, ds)
    f = F32Fitter(spec, cuda, FitOptions(max_wg=max_wg), center=True)
    loss, g, c = f.loss_grad_centred(ds, w)
    g, c = g.cpu().double(), c.cpu()
    mean, live = X.mean(0), torch.arange(F) != 1
    assert c.dtype == torch.float32 and float(c[1]) == 1.5 and bool((c[F:] == 0).all())
    assert N == 1 or bool(((c[:F].double() - mean).abs()[live] <= 2.0 ** -23 * mean.abs()[live]).all())
    c64 = c.double()
    w64 = w.double()
    w64[KF:] += spec.coef(w64) @ c64[:F]  # b' = b + W c
    loss64, g64, bl, bg = oracle(spec, X - c64[:F], y, w64)
    err = (g - g64).abs()
    # raw coordinates
    loss_r, gr = f.loss_grad(ds, w)
    gr = gr.cpu().double()
    g64r = oracle(spec, X, y, w)[1]
    bgr = 1.01 * bg + 2.0 ** -23 * g64r.abs()
    bgr[:KF] += (c64.abs() * 1.01 * bg[KF:].view(K, 1)).reshape(-1)
    err_r = (gr - g64r).abs()
    print(f"[{N}x{FP} K{K} wg{max_wg}] centred: loss err/bound {abs(loss - loss64) / bl:.4f} grad "
          f"{(err / bg.clamp_min(1e-300)).max().item():.4f} (offset column {(err / bg.clamp_min(1e-300))[torch.arange(K) * FP + 2].max().item():.4f}); "
          f"raw grad {(err_r / bgr.clamp_min(1e-300)).max().item():.4f}")
    assert bool(torch.isfinite(g).all()) and abs(loss - loss64) <= 1.01 * bl and loss_r == loss
    assert bool((err <= 1.01 * bg).all()) and bool((err_r <= bgr).all())
    for v in (g, gr):  # padding features
        assert bool((v[:KF].view(K, FP)[:, F:] == 0).all())
    again = f.loss_grad_centred(ds, w)
    assert again[0] == loss and torch.equal(again[1].cpu().double(), g)


@pytest.mark.parametrize("offset", [100.0, 1000.0])
def test_centred_fit_reaches_the_centred_reference(cuda, offset):
    spec, ds = fit_data(offset)
    X, y = rows64(spec, ds)
    ref = fit_reference(X - X.mean(0), y, num_classes=spec.K, reg_param=REG)
    margin = 1e-3 * max(1.0, abs(ref.objective))
    f = F32Fitter(spec, cuda, FitOptions(reg_param=REG), center=True)
    res = f.fit(ds)
    raw = raw_objective(spec, ds, res)
    warm = f.fit(ds, w0=res.w)
    print(f"offset {offset}: iters {res.iters} evals {res.evals} reason {res.reason} objective {res.objective:.9g} raw float64 "
          f"{raw:.9g} (reference {ref.iters}, {ref.reason}, {ref.objective:.9g}); warm {warm.iters}, {warm.reason}, "
          f"{warm.objective:.9g}")
    assert res.reason == "tol" and abs(res.objective - ref.objective) <= margin
    assert abs(raw - ref.objective) <= margin
    assert warm.reason == "tol" and abs(warm.objective - ref.objective) <= margin
    again = F32Fitter(spec, cuda, FitOptions(reg_param=REG), center=True).fit(ds)
    assert torch.equal(again.w, res.w) and again.history == res.history and torch.equal(again.center, res.center)


def test_centred_score_outputs(cuda):
    N, FP, K = 70, 512, 6
    spec, ds, w = case(N, FP, K)
    ds.X[:, 2] += 900.0  # 1000 + N(0,1)
    ds.y[5] = 9  # outside [0, K)
    X, yl = rows64(spec, ds)
    c = X.mean(0).float()
    W, b = spec.coef(w).double(), spec.intercept(w).double()
    z = X @ W.t() + b
    top = z.topk(2, 1).values
    dz = margin_err(X - c.double(), W, b + W @ c.double(), spec.F)
    assert bool((top[:, 0] - top[:, 1] > 2 * dz).all())  # no prediction hangs on the rounding
    ok = (yl >= 0) & (yl < K)
    nll = torch.logsumexp(z, 1) - z.gather(1, yl.clamp(0, K - 1).view(-1, 1)).view(-1)
    r = f32_score(spec, w, ds, cuda, proba=True, center=c)
    assert torch.equal(r.pred.cpu().long(), z.argmax(1))
    perr = (r.proba.cpu().double() - torch.softmax(z, 1)).abs().max(1).values
    got = r.nll.cpu().double()
    nbound = 2 * dz + 1e-6 * z.abs().max()
    nerr = (got - nll).abs()[ok]
    print(f"centred score: largest proba err/bound {(perr / (dz + 1e-6)).max().item():.4f}, "
          f"nll {(nerr / nbound[ok]).max().item():.4f}")
    assert bool((perr <= dz + 1e-6).all())
    assert bool((nerr <= nbound[ok]).all()) and bool(torch.isnan(got[5])) and r.rows_out_of_range == 1

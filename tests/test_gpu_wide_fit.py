"""Wide full-batch fit on MI355X (csrc/kernels/wide_fit_kernels.hip,
csrc/solver/wide_fit.hip): one evaluation against float64 under the derived bound of
tests/_wide_fit_cases.py, the statistics, short trajectories and converged fits against
the float64 oracle (fit_reference on the dense matrix of the touched columns), bit
reproducibility, the dense fitter as a cross-check, the phantom class, an end-to-end
fit with a checkpoint round trip against the CPU path, and the validation path.

Measured on an MI355X (profiles/r13/README.md): the largest gradient error of test 1
is 0.054 of its bound (loss: 0.022); the converged fits end 2.4e-5 .. 7.8e-5 of the
largest standardised coefficient away from the oracle (bound 1e-2); the end-to-end
objective is 2.6e-7 relative from the CPU path's (bound 1e-3)."""
import math

import pytest
import torch

from _fit_cases import fit_case
from _wide_fit_cases import (CONVERGED, check_validation, converged_oracle, csr64, eval_oracle, eval_weights,
                             from_dense, oracle_fit, sparse_case, touched, warm_start)
from psx import _native
from psx.models.reference import feature_std
from psx.models.wide import WideSpec
from psx.ops.fit import BatchFitter, FitOptions
from psx.ops.score import Scorer
from psx.ops.wide_fit import WideFitter, wide_loss_grad
from psx.utils.data import synth_sparse

pytestmark = pytest.mark.gpu

# (N, K, col_chunk, max_wg, weight scale, first label, features 0 and 1 in every row); F = 5000
EVAL_CASES = [
    (1, 1, None, None, 0.05, 0, True),
    (1, 6, None, None, 0.05, 0, True),
    (5, 2, None, None, 0.05, 0, True),
    (5, 3, 64, 3, 0.05, 0, False),  # row 3 has no entry at all
    (229, 1, 64, None, 0.05, 0, True),  # the 229-entry column: 3 chunks of 64 and one of 37
    (229, 3, None, 3, 0.05, 0, True),  # 12 waves share the rows
    (229, 6, 64, 3, 0.05, 0, True),
    (229, 16, 64, None, 0.05, 0, True),
    (229, 6, 64, 3, 0.05, 0, False),  # an empty row among many waves' rows, no full column, chunked columns
    (2000, 1, None, None, 0.05, 0, True),
    (2000, 2, 64, None, 0.05, 0, True),  # the 2000-entry column: 31 chunks and one of 16
    (2000, 6, None, None, 0.05, 0, True),  # default chunk: every column one item, the long ones a wave each
    (2000, 16, None, 3, 0.05, 0, True),
    (2000, 6, 64, None, 1.0, 0, True),  # weight scale 1: max |margin| 7
    (2000, 6, None, None, 4.0, 0, True),  # margins in the tens
    (2000, 6, None, None, 0.05, 1, True),  # labels 1..5 with K = 6: class 0 is absent
]


# ---- 1. one evaluation ------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,col_chunk,max_wg,wscale,first,full", EVAL_CASES)
def test_loss_grad_within_the_derived_bound(cuda, N, K, col_chunk, max_wg, wscale, first, full):
    spec, ds = sparse_case(N, 5000, K, seed=1, labels_from=first, full_cols=full)
    w = eval_weights(spec, wscale=wscale)
    loss64, g64, bl, bg, zmax = eval_oracle(spec, ds, w)
    loss, g = wide_loss_grad(spec, ds, w.to(cuda), cuda, max_wg=max_wg, col_chunk=col_chunk)
    g = g.cpu().double()
    assert g.shape == (spec.P,) and bool(torch.isfinite(g).all())
    err = (g - g64).abs()
    ratio = err / bg.clamp_min(1e-300)
    print(f"[{N}x5000 K{K} chunk{col_chunk} wg{max_wg} w{wscale}] max|z| {zmax:.1f} loss err {abs(loss - loss64):.3e} "
          f"(bound {bl:.3e}) max grad err {err.max().item():.3e}, largest err/bound "
          f"{ratio[bg > 0].max().item() if bool((bg > 0).any()) else 0.0:.3f}")
    assert abs(loss - loss64) <= bl
    assert bool((err <= bg).all())
    if first:
        assert int(ds.y.min()) >= 1
    if wscale >= 4.0:
        assert zmax > 20
    # untouched features and padding classes: exactly zero
    G = g[: spec.F * spec.KP].view(spec.F, spec.KP)
    out = torch.ones(spec.F, dtype=torch.bool)
    out[touched(ds)] = False
    assert bool((G[out] == 0).all()) and bool((G[:, spec.K:] == 0).all())
    assert bool((g[spec.F * spec.KP + spec.K:] == 0).all())


# ---- 2. statistics ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(600, 1), (229, 6)])
def test_statistics_and_touched_features(cuda, N, K):
    spec, ds = sparse_case(N, 5000, K, seed=2)
    res = WideFitter(spec, cuda, FitOptions(max_iter=1)).fit(ds)
    f = touched(ds)
    assert torch.equal(res.features.cpu().long(), f) and res.features.dtype == torch.int32
    ref = feature_std(csr64(ds)[:, f])
    std = res.std.cpu().double()
    assert std.shape == ref.shape and torch.allclose(std, ref, rtol=1e-6, atol=0)
    assert int(f[0]) == 0 and float(std[0]) == 0.0


# ---- 3. short trajectories ----------------------------------------------------------------------
@pytest.mark.parametrize("N,F,K", [(1000, 20000, 6), (600, 5000, 1)])
@pytest.mark.parametrize("lam", [0.0, 0.05])
def test_short_trajectory_matches_the_oracle(cuda, N, F, K, lam):
    spec, ds = sparse_case(N, F, K, seed=11)
    w0 = warm_start(spec, seed=3)
    f, ref = oracle_fit(spec, ds, w0, reg_param=lam, max_iter=4, ls_max=6)
    res = WideFitter(spec, cuda, FitOptions(max_iter=4, ls_max=6, reg_param=lam)).fit(ds, w0=w0)
    assert res.iters == ref.iters, (res.iters, ref.iters, res.evals, ref.evals)
    assert abs(res.objective - ref.objective) <= 1e-3 * abs(ref.objective)
    w = res.w.cpu()
    sd = ref.std
    c0 = spec.coef(w0)[:, f].double()
    dref = (ref.coef - c0) * sd
    dgot = (spec.coef(w)[:, f].double() - c0) * sd
    err = (dgot - dref).abs().max().item() / max(dref.abs().max().item(), 1e-6)
    bref = ref.intercept - spec.intercept(w0).double()
    errb = (spec.intercept(w).double() - spec.intercept(w0).double() - bref).abs().max().item() / max(
        bref.abs().max().item(), 1e-6)
    print(f"[{N}x{F} K{K} lam {lam}] iters {res.iters} evals {res.evals}/{ref.evals} objective {res.objective:.9g} "
          f"oracle {ref.objective:.9g} beta change err {err:.3e} intercepts {errb:.3e}")
    assert err <= 2e-2
    assert len(res.history) == res.iters + 1


# ---- 4. converged fits ----------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CONVERGED)))
def test_converged_fit_matches_the_oracle(cuda, i):
    """max|beta - beta_ref| / max|beta_ref| measured on an MI355X (bound 1e-2): 3.6e-5, 7.8e-5 and
    2.4e-5 for the three cases; intercepts 8.8e-5, 2.3e-3 and 2.0e-6 away (printed, not bounded).  The
    comparison is on beta = coef * sigma: half the columns have one entry, so sigma ~ |v| / sqrt(N) and
    |coef| reaches 40-50, which would drown the comparison.  (The case generator is written from the
    issue's description, not its author's script: the oracle takes 53 / 172 / 32 iterations here.)"""
    spec, ds, f, ref = converged_oracle(i)
    K = spec.K
    res = WideFitter(spec, cuda, FitOptions(max_iter=CONVERGED[i][3], tol=0.0, reg_param=0.1)).fit(ds)
    w = res.w.cpu()
    coef = spec.coef(w)[:, f].double()
    sd = res.std.cpu().double()
    beta, beta_ref = coef * sd, ref.coef * ref.std
    top = float(beta_ref.abs().max())
    err = float((beta - beta_ref).abs().max())
    b = spec.intercept(w).double()
    errb = float((b - ref.intercept).abs().max())
    csum = float(beta.sum(0).abs().max())
    print(f"case {CONVERGED[i]}: U {f.numel()} iters {res.iters} evals {res.evals} reason {res.reason} (oracle "
          f"{ref.iters}, {ref.reason}) beta err / max|beta| {err / top:.3e} intercepts {errb:.3e} "
          f"|sum_c beta| / max|beta| {csum / float(beta.abs().max()):.3e} objective {res.objective:.9g} "
          f"oracle {ref.objective:.9g} max|coef| {float(ref.coef.abs().max()):.1f}")
    assert all(b1 <= a1 for a1, b1 in zip(ref.history, ref.history[1:]))
    assert err <= 1e-2 * top
    if K >= 2:
        assert abs(float(b.sum())) <= K * 2.0 ** -22 * max(1.0, float(b.abs().max()))
        assert csum <= 1e-3 * float(beta.abs().max())
    assert all(b1 <= a1 for a1, b1 in zip(res.history, res.history[1:]))
    assert int(f[0]) == 0 and bool((coef[:, 0] == 0).all()) and float(res.std[0]) == 0.0
    out = torch.ones(spec.F, dtype=torch.bool)
    out[f] = False
    assert bool((spec.coef(w)[:, out] == 0).all())


# ---- 5. reproducibility ----------------------------------------------------------------------------
def test_fits_are_bit_reproducible(cuda):
    spec, ds = sparse_case(229, 5000, 6, seed=2)
    _, other = sparse_case(100, 5000, 6, seed=4)
    f = WideFitter(spec, cuda, FitOptions(max_iter=6, max_wg=3, reg_param=0.01), col_chunk=64)
    a = f.fit(ds)
    b = f.fit(ds)
    f.fit(other, w0=warm_start(spec, seed=9))  # an unrelated fit in between
    c = f.fit(ds)
    assert a.iters >= 3
    for r in (b, c):
        assert torch.equal(r.w, a.w) and r.history == a.history and (r.iters, r.evals) == (a.iters, a.evals)


# ---- 6. the dense fitter on the same values ------------------------------------------------------
def test_dense_fitter_cross_check(cuda):
    dspec, dds, const = fit_case(300, 100, 6)
    sds = from_dense(dds)
    opts = FitOptions(reg_param=0.05, max_iter=30)
    dense = BatchFitter(dspec, cuda, opts).fit(dds)
    wide = WideFitter(WideSpec(100, 6), cuda, opts).fit(sds)
    print(f"dense {dense.iters} iterations objective {dense.objective:.9g}, wide {wide.iters} iterations "
          f"objective {wide.objective:.9g}")
    for r in (dense, wide):
        assert all(b <= a for a, b in zip(r.history, r.history[1:]))
    assert abs(wide.objective - dense.objective) <= 1e-3 * abs(dense.objective)
    assert wide.features.numel() == 100
    assert torch.allclose(wide.std.cpu(), dense.std.cpu(), rtol=1e-5, atol=0) and float(wide.std[const]) == 0.0


# ---- 7. phantom class -------------------------------------------------------------------------------
def test_phantom_class_stays_finite_and_is_never_predicted(cuda):
    spec, ds = sparse_case(500, 5000, 6, seed=7, labels_from=1)
    assert int(ds.y.min()) == 1
    res = WideFitter(spec, cuda, FitOptions(max_iter=50, reg_param=0.01)).fit(ds)
    assert bool(torch.isfinite(res.w).all())
    assert all(b <= a for a, b in zip(res.history, res.history[1:])) and res.objective < res.history[0]
    pred = Scorer(spec, res.w, cuda).predict(ds.to(cuda))
    assert int((pred == 0).sum()) == 0


# ---- 8. end to end -----------------------------------------------------------------------------------
def test_end_to_end_fit_checkpoint_and_score(cuda, tmp_path):
    train = synth_sparse(20000, 1 << 16, "finefood", seed=0)
    test = synth_sparse(2000, 1 << 16, "finefood", seed=1)
    spec = WideSpec(1 << 16, 6)
    opts = FitOptions(reg_param=1e-3)
    res = WideFitter(spec, cuda, opts).fit(train)
    assert _native.hip_loaded_path() is not None
    assert res.reason in ("tol", "max_iter")
    freq = torch.bincount(train.y.long(), minlength=6).double() / train.rows
    entropy = -sum(float(p) * math.log(float(p)) for p in freq if p > 0)  # the intercept-only model's log-loss
    assert res.log_loss < entropy and res.log_loss <= res.objective
    sc = Scorer(spec, res.w, cuda).score(test.to(cuda))
    res.save(str(tmp_path))
    again = Scorer.from_checkpoint(str(tmp_path), cuda).score(test.to(cuda))
    assert (again.accuracy, again.f1, again.log_loss) == (sc.accuracy, sc.f1, sc.log_loss)
    assert torch.equal(again.confusion, sc.confusion)
    cpu = WideFitter(spec, "cpu", opts).fit(train)  # the yardstick
    sc_cpu = Scorer(spec, cpu.w, "cpu").score(test)
    print(f"end to end: U {res.features.numel()} iters {res.iters} evals {res.evals} reason {res.reason} seconds "
          f"{res.seconds:.3f} pass {res.pass_seconds * 1e3:.3f} ms objective {res.objective:.9g} (cpu {cpu.objective:.9g}, "
          f"{cpu.iters} iterations, relative difference {abs(res.objective - cpu.objective) / cpu.objective:.3e}) "
          f"entropy {entropy:.4f} test accuracy {sc.accuracy:.4f} (cpu {sc_cpu.accuracy:.4f})")
    assert abs(res.objective - cpu.objective) <= 1e-3 * abs(cpu.objective)


# ---- 9. validation on the device -----------------------------------------------------------------------
def test_validation_on_the_device(cuda):
    check_validation(cuda)

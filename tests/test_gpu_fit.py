"""Full-batch fit on MI355X (csrc/kernels/fit_kernels.hip, csrc/solver/fit.hip):
one evaluation against float64 under the derived bound of tests/_fit_cases.py, short
trajectories and converged fits against the float64 oracle (fit_reference, itself
checked against sklearn in test_fit_cpu.py), bit reproducibility, the phantom class,
an end-to-end fit with a checkpoint round trip, and the validation path.

Measured on an MI355X (profiles/r12/README.md): the largest gradient error of test 1
is 0.020 of its bound (loss: 0.003); the converged fits end 6.5e-4 and 1.3e-3 of the
largest coefficient away from the oracle (bound 1e-2), their intercepts 1.2e-3 and
2.8e-2 away (printed, not bounded: see the test)."""
import pytest
import torch

from _fit_cases import (CONVERGED, check_validation, converged_oracle, eval_case, eval_oracle, fit_case, rows64,
                        warm_start)
from psx import _native
from psx.models.logreg import ModelSpec
from psx.models.reference import fit_reference
from psx.ops.fit import BatchFitter, FitOptions, loss_grad
from psx.ops.score import Scorer
from psx.utils.data import synth_finefood

pytestmark = pytest.mark.gpu

# (N, F, K, max_wg, weight scale, first label)
EVAL_CASES = [
    (1, 100, 2, None, 0.05, 0),
    (31, 100, 6, None, 0.05, 0),
    (33, 300, 5, None, 0.05, 0),
    (229, 1024, 6, 3, 0.05, 0),  # several tiles share a workgroup, the last tile is partial
    (40, 1024, 6, 8, 0.05, 0),  # some workgroups have no tile
    (2000, 2000, 16, None, 0.05, 0),
    (700, 512, 8, None, 0.05, 0),
    (700, 512, 8, None, 1.0, 0),  # margins in the tens
    (229, 1024, 6, None, 0.05, 1),  # labels 1..5 with K = 6: class 0 is absent
]


# ---- 1. one evaluation ------------------------------------------------------------------------
@pytest.mark.parametrize("N,F,K,max_wg,wscale,first", EVAL_CASES)
def test_loss_grad_within_the_derived_bound(cuda, N, F, K, max_wg, wscale, first):
    spec, ds, w = eval_case(N, F, K, wscale=wscale, labels_from=first)
    loss64, g64, bl, bg, zmax = eval_oracle(spec, ds, w)
    loss, g = loss_grad(spec, ds, w.to(cuda), cuda, max_wg=max_wg)
    g = g.cpu().double()
    assert g.shape == (spec.P,) and bool(torch.isfinite(g).all())
    err = (g - g64).abs()
    ratio = err / bg.clamp_min(1e-300)
    print(f"[{N}x{F} K{K} wg{max_wg} w{wscale}] max|z| {zmax:.1f} loss err {abs(loss - loss64):.3e} (bound {bl:.3e}) "
          f"max grad err {err.max().item():.3e}, largest err/bound {ratio.max().item():.3f}")
    assert abs(loss - loss64) <= bl
    assert bool((err <= bg).all())
    if wscale >= 1.0:
        assert zmax > 20
    pad = torch.ones(spec.K, spec.Fp, dtype=torch.bool)
    pad[:, : spec.F] = False
    assert bool((g[: spec.K * spec.Fp].view(spec.K, spec.Fp)[pad] == 0).all())  # padding features


# ---- 2. short trajectories ----------------------------------------------------------------------
@pytest.mark.parametrize("N,F", [(700, 1024), (300, 256)])
@pytest.mark.parametrize("lam", [0.0, 0.05])
def test_short_trajectory_matches_the_oracle(cuda, N, F, lam):
    spec = ModelSpec(F, 6)
    ds = synth_finefood(N, F, seed=11)
    w0 = warm_start(spec, seed=3)
    ref = fit_reference(ds.float_features(), ds.y.long(), spec.coef(w0), spec.intercept(w0), reg_param=lam,
                        max_iter=4, ls_max=6)
    res = BatchFitter(spec, cuda, FitOptions(max_iter=4, ls_max=6, reg_param=lam)).fit(ds, w0=w0)
    assert res.iters == ref.iters, (res.iters, ref.iters, res.evals, ref.evals)
    assert abs(res.objective - ref.objective) <= 1e-3 * max(1.0, abs(ref.objective))
    w = res.w.cpu()
    dref = ref.coef.float() - spec.coef(w0)
    dgot = spec.coef(w) - spec.coef(w0)
    err = (dgot - dref).abs().max().item() / max(dref.abs().max().item(), 1e-6)
    bref = ref.intercept.float() - spec.intercept(w0)
    errb = (spec.intercept(w) - spec.intercept(w0) - bref).abs().max().item() / max(bref.abs().max().item(), 1e-6)
    print(f"[{N}x{F} lam {lam}] iters {res.iters} evals {res.evals}/{ref.evals} objective {res.objective:.9g} "
          f"oracle {ref.objective:.9g} coefficient change err {err:.3e} intercepts {errb:.3e}")
    assert err <= 2e-2 and errb <= 2e-2
    assert len(res.history) == res.iters + 1


# ---- 3. converged fits ----------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CONVERGED)))
def test_converged_fit_matches_the_oracle(cuda, i):
    spec, ds, const, ref = converged_oracle(i)
    res = BatchFitter(spec, cuda, FitOptions(max_iter=CONVERGED[i][3], tol=0.0, reg_param=0.1)).fit(ds)
    w = res.w.cpu()
    coef = spec.coef(w).double()
    top = float(ref.coef.abs().max())
    err = float((coef - ref.coef).abs().max())
    errb = float((spec.intercept(w).double() - ref.intercept).abs().max())
    beta = coef * res.std.cpu().double()
    csum = float(beta.sum(0).abs().max())
    print(f"case {CONVERGED[i]}: iters {res.iters} evals {res.evals} reason {res.reason} (oracle {ref.iters}, "
          f"{ref.reason}) coef err / max|coef| {err / top:.3e} intercepts {errb:.3e} "
          f"|sum_c beta| / max|beta| {csum / float(beta.abs().max()):.3e} objective {res.objective:.9g} "
          f"oracle {ref.objective:.9g}")
    assert err <= 1e-2 * top
    # (the intercepts are printed, not bounded: with uncentred features they absorb -sum_f coef_f mean_f, the
    # flattest direction of the objective, and move by several 1e-2 while the fp32 evaluation can no longer
    # tell the objectives apart -- see profiles/r12/README.md; centred they must be)
    b = spec.intercept(w).double()
    assert abs(float(b.sum())) <= spec.K * 2.0 ** -22 * max(1.0, float(b.abs().max()))
    assert bool((coef[:, const] == 0).all()) and float(res.std[const]) == 0.0
    assert csum <= 1e-3 * float(beta.abs().max())
    assert all(b <= a for a, b in zip(res.history, res.history[1:]))
    assert torch.allclose(res.std.cpu().double(), ref.std, rtol=1e-6, atol=0)


# ---- 4. reproducibility ----------------------------------------------------------------------------
def test_fits_are_bit_reproducible(cuda):
    spec, ds, _ = fit_case(229, 1024, 6, seed=2)
    other_spec, other, _ = fit_case(100, 1024, 6, seed=4)
    f = BatchFitter(spec, cuda, FitOptions(max_iter=6, max_wg=3, reg_param=0.01))
    a = f.fit(ds)
    b = f.fit(ds)
    f.fit(other, w0=warm_start(spec, seed=9))  # an unrelated fit in between
    c = f.fit(ds)
    assert a.iters >= 3
    for r in (b, c):
        assert torch.equal(r.w, a.w) and r.history == a.history and (r.iters, r.evals) == (a.iters, a.evals)


# ---- 5. phantom class -------------------------------------------------------------------------------
def test_phantom_class_stays_finite_and_is_never_predicted(cuda):
    spec, ds, _ = fit_case(500, 100, 6, seed=7, labels_from=1)
    assert int(ds.y.min()) == 1
    X, y = rows64(spec, ds)
    ref = fit_reference(X, y, num_classes=6, reg_param=0.01, max_iter=50)
    res = BatchFitter(spec, cuda, FitOptions(max_iter=50, reg_param=0.01)).fit(ds)
    assert bool(torch.isfinite(res.w).all())
    assert all(b <= a for a, b in zip(res.history, res.history[1:])) and res.objective < res.history[0]
    print(f"phantom: iters {res.iters} (oracle {ref.iters}) objective {res.objective:.9g} oracle {ref.objective:.9g}")
    if res.iters == ref.iters:
        assert abs(res.objective - ref.objective) <= 1e-3 * abs(ref.objective)
    pred = Scorer(spec, res.w, cuda).predict(ds.to(cuda))
    assert int((pred == 0).sum()) == 0


# ---- 6. end to end -----------------------------------------------------------------------------------
def test_end_to_end_fit_checkpoint_and_score(cuda, tmp_path):
    train, test = synth_finefood(20000, seed=0), synth_finefood(2000, seed=1)
    spec = ModelSpec(train.num_features, 6)
    res = BatchFitter(spec, cuda, FitOptions(reg_param=1e-3)).fit(train)
    assert _native.hip_loaded_path() is not None
    sc = Scorer(spec, res.w, cuda).score(test.to(cuda))
    print(f"end to end: iters {res.iters} evals {res.evals} reason {res.reason} seconds {res.seconds:.3f} "
          f"pass {res.pass_seconds * 1e3:.3f} ms test accuracy {sc.accuracy:.4f} f1 {sc.f1:.4f}")
    assert sc.accuracy > 0.35
    assert res.reason in ("tol", "max_iter") and res.log_loss <= res.objective
    res.save(str(tmp_path))
    again = Scorer.from_checkpoint(str(tmp_path), cuda).score(test.to(cuda))
    assert (again.accuracy, again.f1, again.log_loss) == (sc.accuracy, sc.f1, sc.log_loss)
    assert torch.equal(again.confusion, sc.confusion)


# ---- 7. validation on the device -----------------------------------------------------------------------
def test_validation_on_the_device(cuda):
    check_validation(cuda)

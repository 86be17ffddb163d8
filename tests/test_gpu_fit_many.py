"""Many dense fits per read of the rows on MI355X (csrc/kernels/fit_many.hip,
csrc/solver/fit_many.hip) against the float64 weighted oracles of psx/models/reference.py.

One evaluation keeps the derived bounds of _fit_cases.eval_oracle for each job's own
weight vector (the bounds of the weighted single-model test); the short fits keep the
bounds of check_short_fit.  100 rows: four tiles, the last with 4 real rows."""
import functools
from dataclasses import replace

import pytest
import torch

from _fit_cases import CONVERGED, eval_case, eval_oracle, fit_case, rows64
from psx.models.reference import fit_reference, weighted_feature_std, weighted_loss_grad
from psx.ops.fit import BatchFitter, FitJob, FitOptions, cross_validate
from test_gpu_fit_weighted import N_ROWS, check_short_fit, draw_weights

pytestmark = pytest.mark.gpu

HOLDOUTS = (None, 0, 1, 2)


def kp_of(K):
    return next(p for p in (2, 4, 8, 16) if p >= K)


def capacity(FP, K):  # the (FP, KP) -> GP table of csrc/kernels/fit_many.h
    return (4 if FP <= 512 else 3 if FP == 1024 else 1) * (16 // kp_of(K))


def effective(wts, y, h):
    v = (wts.sample_weight * wts.class_weight.float()[y]).double()
    held = wts.fold == h if h is not None else torch.zeros_like(y, dtype=torch.bool)
    return torch.where(held, v * 0, v), torch.where(held, v, v * 0)


@functools.lru_cache(maxsize=None)
def eval_reference(FP, K):
    """capacity + 1 jobs (weight vector m, held-out fold HOLDOUTS[m % 4]): float64 loss, held-out loss,
    gradient and the derived bounds of every job."""
    spec, ds, _ = eval_case(N_ROWS, FP - 3, K, seed=5)
    wts = replace(draw_weights(N_ROWS, K), holdout=None)
    X, y = rows64(spec, ds)
    jobs = []
    for m in range(capacity(FP, K) + 1):
        w, h = eval_case(8, FP - 3, K, seed=100 + m)[2], HOLDOUTS[m % 4]
        W, b = spec.coef(w).double(), spec.intercept(w).double()
        u, ho = effective(wts, y, h)
        loss, gc, gb = weighted_loss_grad(X, y, W, b, u)
        _, _, bl, bg, _ = eval_oracle(spec, ds, w)
        g64 = torch.cat([torch.nn.functional.pad(gc, (0, FP - spec.F)).reshape(-1), gb])
        ho64 = float(weighted_loss_grad(X, y, W, b, ho)[0]) if h is not None else 0.0
        jobs.append((w, h, float(loss), ho64, g64, bl, bg))
    return spec, ds, wts, jobs


@pytest.mark.parametrize("max_wg", [3, None])
@pytest.mark.parametrize("nj", ["one", "second_group", "second_pass"])
@pytest.mark.parametrize("K", [2, 3, 6, 16])
@pytest.mark.parametrize("FP", [128, 1024, 2048])
def test_loss_grad_many_against_float64(cuda, FP, K, nj, max_wg):
    spec, ds, wts, jobs = eval_reference(FP, K)
    assert spec.Fp == FP
    M = {"one": 1, "second_group": 16 // kp_of(K) + 1, "second_pass": capacity(FP, K) + 1}[nj]
    f = BatchFitter(spec, cuda, FitOptions(max_wg=max_wg))
    loss, g, ho = f.loss_grad_many(ds, torch.stack([j[0] for j in jobs[:M]]).to(cuda), wts, [j[1] for j in jobs[:M]])
    assert f.many_capacity == capacity(FP, K)
    for m, (_, h, loss64, ho64, g64, bl, bg) in enumerate(jobs[:M]):
        err = (g[m].cpu().double() - g64).abs()
        print(f"[FP{FP} K{K} M{M} wg{max_wg} job {m} holdout {h}] loss err {abs(float(loss[m]) - loss64):.3e} held-out "
              f"err {abs(float(ho[m]) - ho64):.3e} (bound {bl:.3e}) grad err/bound {(err / bg.clamp_min(1e-300)).max():.3f}")
        assert abs(float(loss[m]) - loss64) <= bl and abs(float(ho[m]) - ho64) <= bl
        assert bool((err <= bg).all())


def same(a, b):
    return (torch.equal(a.w, b.w) and torch.equal(a.std, b.std) and a.history == b.history
            and a.holdout_log_loss == b.holdout_log_loss and (a.iters, a.reason) == (b.iters, b.reason))


def test_a_job_does_not_see_its_neighbours_or_its_slot(cuda):
    spec, ds, _ = fit_case(N_ROWS, 20, 6, seed=3)  # capacity 8: ten jobs are two passes
    wts = replace(draw_weights(N_ROWS, 6, seed=2), holdout=None)
    f = BatchFitter(spec, cuda, FitOptions(max_iter=5, max_wg=3))
    j = FitJob(0.05, 2)
    others = [FitJob(10.0 ** -(m % 4), HOLDOUTS[m % 4]) for m in range(8)]
    batch = others[:2] + [j] + others[2:] + [j]  # slot 2 of the first pass, slot 1 of the second
    a, b, solo = f.fit_many(ds, batch, wts), f.fit_many(ds, batch, wts), f.fit_many(ds, [j], wts)[0]
    assert f.many_capacity == 8 and solo.iters >= 3 and solo.holdout_log_loss > 0
    assert same(a[2], solo) and same(a[9], solo)
    assert all(same(x, y) for x, y in zip(a, b))


def test_short_fits_match_the_oracle(cuda):
    N, F, K, _ = CONVERGED[0]
    spec, ds, _ = fit_case(N, F, K, seed=0)
    wts = replace(draw_weights(N, K, seed=1), holdout=None)
    X, y = rows64(spec, ds)
    jobs = [FitJob(0.1, 0), FitJob(0.01, 1), FitJob(0.1, None)]
    # a penalty that large makes for long line searches: the other jobs' slots are inactive while it runs on
    res = BatchFitter(spec, cuda, FitOptions(max_iter=8, tol=0.0)).fit_many(ds, jobs + [FitJob(1e4, 0)], wts)
    print("evaluations per job", [r.evals for r in res], [r.reason for r in res])
    assert len({r.evals for r in res}) > 1
    for j, r in zip(jobs, res):
        u, h = effective(wts, y, j.holdout)
        ref = fit_reference(X, y, num_classes=K, reg_param=j.reg_param, tol=0.0, max_iter=8,
                            std=weighted_feature_std(X, u), loss_grad=lambda ce, bb: weighted_loss_grad(X, y, ce, bb, u))
        check_short_fit(spec, r, ref)
        if j.holdout is None:
            assert r.holdout_log_loss is None
            continue
        ho64 = float(weighted_loss_grad(X, y, ref.coef, ref.intercept, h)[0])
        assert abs(r.holdout_log_loss - ho64) <= 1e-3 * max(1.0, ho64)


def test_cross_validate_batched_agrees_with_sequential(cuda):
    N, F, K, _ = CONVERGED[0]
    spec, ds, _ = fit_case(N, F, K, seed=0)
    kw = dict(folds=3, seed=4, device=cuda, opts=FitOptions(max_iter=30))
    seq = cross_validate(spec, ds, [0.3, 0.003], **kw)
    for batch in ("auto", 4):
        cv = cross_validate(spec, ds, [0.3, 0.003], batch=batch, **kw)
        assert cv.best_reg_param == seq.best_reg_param and torch.equal(cv.fold, seq.fold)
        for a, b in zip(sum(cv.losses, []), sum(seq.losses, [])):
            assert abs(a - b) <= 1e-3 * max(1.0, b)

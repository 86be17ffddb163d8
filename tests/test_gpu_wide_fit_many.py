"""Many wide fits per read of the rows on MI355X (csrc/kernels/wide_fit_many.hip,
csrc/solver/wide_fit_many.hip) against float64 on the bf16 values as stored.

One evaluation keeps, per job, the derived bounds of test_gpu_wide_fit_weighted.bounds
under that job's effective weights: they hold for any summation order and count exactly
the roundings these kernels make (sample weight x class weight, u x residual).  The
short fits and the cross-validation keep the bounds of the weighted single-model tests."""
import functools
from dataclasses import replace

import pytest
import torch

from _wide_fit_cases import CONVERGED, csr64, eval_weights, sparse_case, touched
from psx.models.reference import fit_reference, weighted_feature_std, weighted_loss_grad
from psx.ops.fit import FitJob, FitOptions, cross_validate
from psx.ops.wide_fit import WideFitter
from test_gpu_wide_fit_weighted import bounds, draw_weights, same_trajectory

pytestmark = pytest.mark.gpu

HOLDOUTS = (None, 0, 1, 2)


def effective(wts, y, h):
    v = (wts.sample_weight * wts.class_weight[y]).double()
    held = wts.fold == h if h is not None else torch.zeros_like(y, dtype=torch.bool)
    return torch.where(held, v * 0, v), torch.where(held, v, v * 0)


@functools.lru_cache(maxsize=None)
def eval_reference(N, K, full):
    """slots + 1 jobs (weights of seed m, held-out fold HOLDOUTS[m % 4]): float64 loss, held-out loss, gradient
    and the derived bounds of every job."""
    spec, ds = sparse_case(N, 5000, K, seed=1, full_cols=full)
    wts = replace(draw_weights(ds, K)[0], holdout=None)
    jobs = []
    for m in range(32 // spec.KP + 1):
        w, h = eval_weights(spec, seed=m), HOLDOUTS[m % 4]
        u, ho = effective(wts, ds.y.long(), h)
        loss64, g64, bl, bg = bounds(spec, ds, w, u)
        ho64, bh = (bounds(spec, ds, w, ho)[0::2] if h is not None else (0.0, 0.0))
        jobs.append((w, h, loss64, ho64, g64, bl, bh, bg))
    return spec, ds, wts, jobs


@pytest.mark.parametrize("N,K,nj,col_chunk,max_wg,full",
                         [(229, K, nj, cc, wg, True) for K in (1, 2, 3, 6, 16) for nj in ("one", "slots", "second_pass")
                          for cc, wg in ((64, 3), (None, None))]
                         + [(5, 3, "second_pass", 64, 3, False), (2000, 6, "second_pass", None, None, True)])
def test_loss_grad_many_against_float64(cuda, N, K, nj, col_chunk, max_wg, full):
    spec, ds, wts, jobs = eval_reference(N, K, full)
    slots = 32 // spec.KP
    M = {"one": 1, "slots": slots, "second_pass": slots + 1}[nj]
    f = WideFitter(spec, cuda, FitOptions(max_wg=max_wg), col_chunk=col_chunk)
    loss, g, ho = f.loss_grad_many(ds, torch.stack([j[0] for j in jobs[:M]]).to(cuda), wts, [j[1] for j in jobs[:M]])
    assert f.many_capacity == slots
    out = torch.ones(spec.F, dtype=torch.bool)
    out[touched(ds)] = False
    for m, (_, h, loss64, ho64, g64, bl, bh, bg) in enumerate(jobs[:M]):
        gm = g[m].cpu().double()
        err = (gm - g64).abs()
        print(f"[{N} K{K} M{M} chunk{col_chunk} wg{max_wg} job {m} holdout {h}] loss err/bound "
              f"{abs(float(loss[m]) - loss64) / bl:.3f} held-out err {abs(float(ho[m]) - ho64):.3e} (bound {bh:.3e}) "
              f"largest grad err/bound {(err / bg.clamp_min(1e-300))[bg > 0].max().item():.3f}")
        assert abs(float(loss[m]) - loss64) <= bl and abs(float(ho[m]) - ho64) <= bh
        assert bool((err <= bg).all())
        G = gm[: spec.F * spec.KP].view(spec.F, spec.KP)
        assert bool((G[out] == 0).all()) and bool((G[:, spec.K:] == 0).all())
        assert bool((gm[spec.F * spec.KP + spec.K:] == 0).all())


def same(a, b):
    return (torch.equal(a.w, b.w) and torch.equal(a.std, b.std) and a.history == b.history
            and a.holdout_log_loss == b.holdout_log_loss and (a.iters, a.reason) == (b.iters, b.reason))


def test_a_job_does_not_see_its_neighbours_or_its_slot(cuda):
    spec, ds = sparse_case(229, 5000, 6, seed=3)  # 4 slots: six jobs are two passes
    wts = replace(draw_weights(ds, 6, seed=2)[0], holdout=None)
    f = WideFitter(spec, cuda, FitOptions(max_iter=5, max_wg=3), col_chunk=64)
    j = FitJob(0.05, 2)
    others = [FitJob(10.0 ** -(m % 4), HOLDOUTS[m % 4]) for m in range(4)]
    batch = others[:2] + [j] + others[2:] + [j]  # slot 2 of the first pass, slot 1 of the second
    a, b, solo = f.fit_many(ds, batch, wts), f.fit_many(ds, batch, wts), f.fit_many(ds, [j], wts)[0]
    assert f.many_capacity == 4 and solo.iters >= 3 and solo.holdout_log_loss > 0
    assert same(a[2], solo) and same(a[5], solo)
    assert all(same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("i", [0, 2])
def test_short_fits_match_the_oracle(cuda, i):
    N, F, K, _ = CONVERGED[i]
    spec, ds = sparse_case(N, F, K, seed=i)
    wts = replace(draw_weights(ds, K, seed=1)[0], holdout=None)
    ft = touched(ds)
    X, y = csr64(ds)[:, ft], ds.y.long()
    jobs = [FitJob(0.1, 1), FitJob(0.01, 0), FitJob(0.1, None)]
    # a penalty that large makes for long line searches: the other jobs' slots are inactive while it runs on
    res = WideFitter(spec, cuda, FitOptions(max_iter=8, tol=0.0)).fit_many(ds, jobs + [FitJob(1e4, 0)], wts)
    print("evaluations per job", [r.evals for r in res], [r.reason for r in res])
    assert len({r.evals for r in res}) > 1
    for j, r in zip(jobs, res):
        u, h = effective(wts, y, j.holdout)
        ref = fit_reference(X, y, num_classes=K, reg_param=j.reg_param, tol=0.0, max_iter=8,
                            std=weighted_feature_std(X, u), loss_grad=lambda ce, bb: weighted_loss_grad(X, y, ce, bb, u))
        same_trajectory(r, ref)
        err = float((spec.coef(r.w.cpu())[:, ft].double() - ref.coef).abs().max() / ref.coef.abs().max())
        print(f"reg {j.reg_param} holdout {j.holdout}: iters {r.iters} coefficient err {err:.3e}")
        assert err <= 1e-2 and torch.equal(r.features.cpu().long(), ft)
        if j.holdout is None:
            assert r.holdout_log_loss is None
            continue
        ho64 = float(weighted_loss_grad(X, y, ref.coef, ref.intercept, h)[0])
        assert abs(r.holdout_log_loss - ho64) <= 1e-3 * max(1.0, ho64)


def test_cross_validate_batched_agrees_with_sequential(cuda):
    """The two paths round differently (8 entry groups a row against 64 lanes), so their iterates separate; what
    keeps the RETURNED points together is the objective's strong convexity.  Both fits stop within a slack d of the
    same minimum, so |beta_a - beta_b| <= 2 sqrt(2 d / reg): these 600 rows touch about 1,200 features, the data
    give no curvature in more than half the directions and there reg is all of it.  Hence penalties >= 0.1, run to
    the stopping test.  A first version took the dense test's penalties (0.3, 0.003) and 30 iterations: 5 of its 6
    jobs agreed to 5e-5, the job (0.003, fold 1) missed the bound with 1.15e-2 against 2.2e-3 -- histories equal
    to 1e-9 through 12 iterations, both ended by `tol` at objectives 4e-7 apart."""
    N, F, K, _ = CONVERGED[0]
    spec, ds = sparse_case(N, F, K, seed=0)
    kw = dict(folds=3, seed=4, device=cuda, opts=FitOptions(max_iter=100))
    seq = cross_validate(spec, ds, [1.0, 0.1], **kw)
    for batch in ("auto", 4):
        cv = cross_validate(spec, ds, [1.0, 0.1], batch=batch, **kw)
        assert cv.best_reg_param == seq.best_reg_param and torch.equal(cv.fold, seq.fold)
        for a, b in zip(sum(cv.losses, []), sum(seq.losses, [])):
            print(f"batch {batch}: held-out {a:.9g} sequential {b:.9g}")
            assert abs(a - b) <= 1e-3 * max(1.0, b)

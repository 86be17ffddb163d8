"""The weighted wide fit on MI355X (csrc/kernels/wide_fit_weighted.hip): row weights,
class weights and a held-out fold against float64 on the bf16 values as stored.

Bound of one evaluation: the derived bound of _wide_fit_cases.py restated with weights.
Row r's terms are multiplied by its weight u_r (the weight is exact in float64: the
fp32 product the kernels form), N becomes W = sum u, and the two extra roundings of a
weighted residual (sample weight x class weight, u x residual) turn (c_u + 8) into
(c_u + 10) and (N + 8) into (N + 10):

    |dg_uk| <= 1/W sum_e u_r (dz_r + 1e-6) |v_e|  +  (c_u + 10) u24 / W sum_e |u_r R_rk v_e|
    |dloss| <= 1/W sum_r u_r (2 dz_r + 1e-6 zmax) + (N + 10) u24 / W sum_r u_r |nll_r|

(the held-out loss: the same with the held-out weights)."""
import functools

import pytest
import torch

from _wide_fit_cases import CONVERGED, U24, csr64, eval_weights, pack64, sparse_case, touched
from psx import _native
from psx.apps.fit import _take_sparse
from psx.models.reference import fit_reference, weighted_feature_std, weighted_loss_grad
from psx.ops.fit import FitOptions, FitWeights, cross_validate
from psx.ops.wide_fit import WideFitter

pytestmark = pytest.mark.gpu


def draw_weights(ds, K, seed=0):
    """Sample weights in [0, 2] with exact zeros, a class table, 3 folds with fold 1 held out;
    rows 64..95 have weight 0, row 28 (700 entries) is held out, row 23 (65 entries) has weight 0."""
    N = ds.rows
    g = torch.Generator().manual_seed(977 + seed)
    sw = torch.rand(N, generator=g) * 2
    sw[torch.rand(N, generator=g) < 0.1] = 0.0
    fold = torch.randint(0, 3, (N,), generator=g).to(torch.uint8)
    sw[64:96] = 0.0
    if N > 28:
        fold[28], sw[28], sw[23] = 1, 1.25, 0.0
    wts = FitWeights(sw, 0.5 + torch.rand(max(K, 2), generator=g), fold, 1)
    v = (sw * wts.class_weight[ds.y.long()]).double()
    return wts, torch.where(fold == 1, v * 0, v), torch.where(fold == 1, v, v * 0)


def bounds(spec, ds, w, u):
    """float64 (loss, gradient [P], |dloss| bound, |dg| bound [P]) under the row weights u."""
    N, W = ds.rows, u.sum()
    X, Xa, y = csr64(ds), csr64(ds, absolute=True), ds.y.long()
    C, b = spec.coef(w).double(), spec.intercept(w).double()
    z = X @ C.t() + b
    loss, gc, gb = weighted_loss_grad(X, y, C, b, u)
    nll = torch.nn.functional.softplus(z[:, 0]) - (y > 0) * z[:, 0] if spec.K == 1 else \
        torch.logsumexp(z, 1) - z.gather(1, y.view(-1, 1)).view(-1)
    R = (torch.sigmoid(z) - (y > 0).double().view(-1, 1)) if spec.K == 1 else \
        torch.softmax(z, 1) - torch.nn.functional.one_hot(y, spec.K)
    uR = (R * u.view(-1, 1)).abs()
    dz = ((ds.indptr[1:] - ds.indptr[:-1]).double() + 8) * U24 * (Xa @ C.abs().t() + b.abs()).max(1).values
    row = u * (dz + 1e-6)
    cu = torch.bincount(ds.idx.long(), minlength=spec.F).double()
    bg_c = (row @ Xa) / W + (cu + 10) * U24 / W * (uR.t() @ Xa)
    bg_b = row.sum() / W + (N + 10) * U24 / W * uR.sum(0)
    zmax = max(1.0, float(z.abs().max()))
    bl = float(((u * (2 * dz + 1e-6 * zmax)).sum() + (N + 10) * U24 * (u * nll.abs()).sum()) / W)
    return float(loss), pack64(spec, gc, gb), bl, pack64(spec, bg_c, bg_b)


# ---- 1. one evaluation --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,col_chunk,max_wg,full", [
    (5, 3, 64, 3, False), (229, 1, 64, None, True), (229, 6, 64, 3, True), (229, 16, 64, None, True),
    (2000, 3, None, 3, True), (2000, 6, 64, None, True)])
def test_weighted_loss_grad_and_holdout_loss(cuda, N, K, col_chunk, max_wg, full):
    spec, ds = sparse_case(N, 5000, K, seed=1, full_cols=full)
    w = eval_weights(spec)
    wts, u, h = draw_weights(ds, K)
    loss64, g64, bl, bg = bounds(spec, ds, w, u)
    ho64, _, bh, _ = bounds(spec, ds, w, h)
    f = WideFitter(spec, cuda, FitOptions(max_wg=max_wg), col_chunk=col_chunk)
    loss, g = f.loss_grad(ds, w.to(cuda), weights=wts)
    ho = f.holdout_loss(ds, w.to(cuda), wts)
    assert _native.hip_loaded_path() is not None and f._native.weighted
    g = g.cpu().double()
    err = (g - g64).abs()
    print(f"[{N} K{K} chunk{col_chunk} wg{max_wg}] loss err/bound {abs(loss - loss64) / bl:.3f} held-out "
          f"{abs(ho - ho64) / bh:.3f} largest grad err/bound {(err / bg.clamp_min(1e-300))[bg > 0].max().item():.3f}")
    assert abs(loss - loss64) <= bl and abs(ho - ho64) <= bh
    assert bool((err <= bg).all())
    G = g[: spec.F * spec.KP].view(spec.F, spec.KP)
    out = torch.ones(spec.F, dtype=torch.bool)
    out[touched(ds)] = False
    assert bool((G[out] == 0).all()) and bool((G[:, spec.K:] == 0).all())
    assert bool((g[spec.F * spec.KP + spec.K:] == 0).all())


# ---- 2. sigma -------------------------------------------------------------------------------------
def test_weighted_sigma(cuda):
    spec, ds = sparse_case(229, 5000, 6, seed=2)
    wts, u, _ = draw_weights(ds, 6)
    res = WideFitter(spec, cuda, FitOptions(max_iter=1), col_chunk=64).fit(ds, weights=wts)
    f = touched(ds)
    X = csr64(ds)[:, f]
    ref, std = weighted_feature_std(X, u), res.std.cpu().double()
    dead = ((X != 0) & (u > 0).view(-1, 1)).sum(0) == 0  # touched by held-out or zero-weight rows only
    assert int(dead.sum()) >= 1 and bool((std[dead] == 0).all())
    assert bool((res.w.cpu()[: spec.F * spec.KP].view(spec.F, spec.KP)[f[dead]] == 0).all())
    assert int(f[0]) == 0 and float(std[0]) == 0.0 and float(ref[0]) == 0.0
    print(f"largest sigma error {float(((std - ref).abs() / ref.clamp_min(1e-300)).max()):.3e}, {int(dead.sum())} dead")
    assert bool(((std == 0) == (ref == 0)).all()) and torch.allclose(std, ref, rtol=1e-6, atol=0)


# ---- 3. unit weights ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 6])
@pytest.mark.parametrize("N", [229, 2000])
def test_unit_weights_are_the_plain_path(cuda, N, K):
    spec, ds = sparse_case(N, 5000, K, seed=1)
    w = eval_weights(spec).to(cuda)
    ones = FitWeights(sample_weight=torch.ones(N))
    f = WideFitter(spec, cuda, FitOptions(max_iter=3, max_wg=3, reg_param=0.01), col_chunk=64)
    loss, g = f.loss_grad(ds, w)
    assert not f._native.weighted
    loss_w, g_w = f.loss_grad(ds, w, weights=ones)
    assert f._native.weighted
    assert loss_w == loss and torch.equal(g_w, g)
    a, b = f.fit(ds), f.fit(ds, weights=ones)
    assert torch.equal(a.std, b.std) and torch.equal(a.w, b.w) and a.history == b.history
    assert b.holdout_log_loss is None


# ---- 4. short fits --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def short_fit(i):
    N, F, K, _ = CONVERGED[i]
    spec, ds = sparse_case(N, F, K, seed=i)
    wts, u, h = draw_weights(ds, K, seed=1)
    f = touched(ds)
    X, y = csr64(ds)[:, f], ds.y.long()
    ref = fit_reference(X, y, num_classes=K, reg_param=0.1, tol=0.0, max_iter=8, std=weighted_feature_std(X, u),
                        loss_grad=lambda ce, bb: weighted_loss_grad(X, y, ce, bb, u))
    return spec, ds, wts, f, ref, float(weighted_loss_grad(X, y, ref.coef, ref.intercept, h)[0])


def same_trajectory(a, b):
    assert (a.iters, a.reason) == (b.iters, b.reason) and len(a.history) == len(b.history)
    for x, y in zip(a.history, b.history):
        assert abs(x - y) <= 1e-3 * max(1.0, abs(y))


OPTS = dict(max_iter=8, tol=0.0, reg_param=0.1)


@pytest.mark.parametrize("i", [0, 2])
def test_short_weighted_fit_matches_the_oracle(cuda, i):
    spec, ds, wts, f, ref, ho64 = short_fit(i)
    res = WideFitter(spec, cuda, FitOptions(**OPTS)).fit(ds, weights=wts)
    same_trajectory(res, ref)
    err = float((spec.coef(res.w.cpu())[:, f].double() - ref.coef).abs().max() / ref.coef.abs().max())
    print(f"iters {res.iters} objective {res.objective:.9g} / {ref.objective:.9g} coefficient err {err:.3e} "
          f"held-out {res.holdout_log_loss:.9g} / {ho64:.9g}")
    assert err <= 1e-2 and abs(res.holdout_log_loss - ho64) <= 1e-3 * max(1.0, ho64)


# ---- 5. held out = removed ------------------------------------------------------------------------
def test_held_out_rows_equal_removed_rows(cuda):
    spec, ds, wts, *_ = short_fit(0)
    held = WideFitter(spec, cuda, FitOptions(**OPTS)).fit(ds, weights=FitWeights(fold=wts.fold, holdout=1))
    cut = WideFitter(spec, cuda, FitOptions(**OPTS)).fit(_take_sparse(ds, torch.nonzero(wts.fold != 1).view(-1)))
    same_trajectory(held, cut)
    assert held.features.numel() > cut.features.numel()
    assert float((held.w - cut.w).abs().max()) <= 1e-2 * float(cut.w.abs().max())
    sd = torch.zeros(spec.F, device=held.std.device).index_put_((held.features.long(),), held.std)
    assert torch.allclose(sd[cut.features.long()], cut.std, rtol=1e-6, atol=0)


# ---- 6. reproducibility and lifecycle -------------------------------------------------------------
def test_reproducibility_and_lifecycle(cuda):
    spec, ds, wts, *_ = short_fit(0)
    f = WideFitter(spec, cuda, FitOptions(max_iter=5, max_wg=3, reg_param=0.01), col_chunk=64)
    with pytest.raises(RuntimeError):
        f._native.set_weights()
    a, a2 = f.fit(ds, weights=wts), f.fit(ds, weights=wts)
    assert f._native.weighted and torch.equal(a.w, a2.w) and a.history == a2.history
    f.fit(sparse_case(100, spec.F, spec.K, seed=4)[1])  # a new dataset clears the weights
    assert not f._native.weighted
    b = f.fit(ds, weights=wts)
    assert a.iters >= 3 and torch.equal(a.w, b.w) and a.history == b.history
    assert a.holdout_log_loss == b.holdout_log_loss


# ---- 7. cross-validation --------------------------------------------------------------------------
def test_cross_validate_the_wide_model(cuda):
    spec, ds, *_ = short_fit(0)
    regs = [0.01, 1.0]
    cv = cross_validate(spec, ds, regs, folds=3, seed=2, device=cuda, opts=FitOptions(max_iter=10), col_chunk=64)
    for r, reg in enumerate(regs):
        for k in range(3):
            one = WideFitter(spec, cuda, FitOptions(max_iter=10, reg_param=reg), col_chunk=64).fit(
                ds, weights=FitWeights(fold=cv.fold, holdout=k))
            assert one.holdout_log_loss == cv.losses[r][k]
    assert cv.best_reg_param == regs[cv.means.index(min(cv.means))]

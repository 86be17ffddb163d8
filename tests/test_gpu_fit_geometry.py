"""The dense full-batch fitter (csrc/kernels/fit_kernels.hip, csrc/solver/fit.hip) at
every padded width and class count, one accepted step at a time:

  * ``loss_grad`` under the derived bound of _fit_cases.py on the 5 x 5 grid of
    (FP, K) cells plus the unpadded corners, F = 1 and K = 15, N = 97;
  * sigma against float64 ``feature_std`` at every FP, N in {2, 33, 97, 229} and grid
    in {1, 3, default}, with constant columns of awkward values, a single non-zero row
    and a column of two adjacent bf16 values around 100;
  * the invariant chain of _fit_chain.py (gradient, secant pairs, direction, trial
    point and finalisation, each on the device's own state) over 6 accepted steps on
    the diagonal cells, with and without L2, warm and zero start, and from a start
    whose line searches spend their budget;
  * history depths 1, 2, 10 and 16 over 20 accepted steps (every ring wraps);
  * ``zero_const = False``.

The tables, their seeds and the conditions that chose them are in
_fit_geometry_cases.py and test_fit_chain_cpu.py (no seed was chosen on a GPU result).
Measured tolerances and the GPU's share of them: profiles/r15/README.md."""
import pytest
import torch

import _fit_geometry_cases as gc
from _fit_cases import eval_case, eval_oracle, rows64, warm_start
from psx import _native
from psx.models.reference import feature_std, fit_reference
from psx.ops.fit import BatchFitter, FitOptions
from psx.ops.lr import stream_handle

pytestmark = pytest.mark.gpu


def _tiles(N):
    return (N + 31) // 32


# ---- 1. one evaluation on the whole grid ---------------------------------------------------------
@pytest.mark.parametrize("max_wg", [3, None])
@pytest.mark.parametrize("F,K", gc.EVAL_CELLS)
def test_loss_grad_on_the_grid(cuda, F, K, max_wg):
    N = gc.N_ROWS
    spec, ds, w = eval_case(N, F, K, seed=5)
    loss64, g64, bl, bg, zmax = eval_oracle(spec, ds, w)
    f = BatchFitter(spec, cuda, FitOptions(max_wg=max_wg))
    loss, g = f.loss_grad(ds, w.to(cuda))
    assert _native.hip_loaded_path() is not None
    if max_wg:
        assert f._native.grid == min(max_wg, _tiles(N))
    else:
        assert f._native.grid == _tiles(N)
    assert f._native.n == spec.P and f._native.nv == (spec.P + 63) // 64 * 64
    g = g.cpu().double()
    err = (g - g64).abs()
    print(f"[F{F} FP{spec.Fp} K{K} wg{max_wg}] loss err {abs(loss - loss64):.3e} (bound {bl:.3e}) "
          f"largest grad err/bound {(err / bg.clamp_min(1e-300)).max().item():.3f}")
    assert abs(loss - loss64) <= bl
    assert bool((err <= bg).all())
    pad = torch.ones(spec.K, spec.Fp, dtype=torch.bool)
    pad[:, : spec.F] = False
    assert bool((g[: spec.K * spec.Fp].view(spec.K, spec.Fp)[pad] == 0).all())


# ---- 2. statistics ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", gc.STAT_ROWS)
@pytest.mark.parametrize("FP", gc.FPS)
def test_sigma_at_every_width(cuda, FP, N):
    """rtol 1e-6 against the two-pass float64 sigma.  The column of adjacent bf16 values
    (mean / sigma about 200) gets 1e-6 + 4 x what FLOAT64 loses on the kernel's one-pass
    formula against the two-pass oracle (measured here, below 1e-9: see test_fit_chain_cpu.py)."""
    spec, ds, special = gc.stat_case(N, FP)
    ref = feature_std(ds.X[:, : spec.F].double())
    for max_wg in gc.STAT_WG:
        f = BatchFitter(spec, cuda, FitOptions(max_wg=max_wg))
        with torch.cuda.device(f.device):
            f._load(ds)
            std = torch.empty(spec.Fp, dtype=torch.float32, device=f.device)
            f._native.read_std(std.data_ptr(), stream_handle(f.device))
        assert f._native.grid == min(max_wg or _tiles(N), _tiles(N))
        std = std.cpu().double()
        assert bool((std[spec.F:] == 0).all())
        rtol = torch.full((spec.F,), 1e-6, dtype=torch.float64)
        for col, kind in special.items():
            if kind == "const":
                assert float(std[col]) == 0.0 and float(ref[col]) == 0.0, (col, float(std[col]))
            elif kind == "adjacent":
                rtol[col] += 4 * gc.one_pass_loss(ds.X[:, col].double())
        rel = (std[: spec.F] - ref).abs() / ref.clamp_min(1e-300)
        rel[ref == 0] = 0
        print(f"[FP{FP} N{N} wg{max_wg}] largest sigma error {float(rel.max()):.3e}")
        assert bool(((std[: spec.F] - ref).abs() <= rtol * ref).all()), float(rel.max())
    assert _native.hip_loaded_path() is not None


def test_constant_columns_are_excluded_from_the_fit(cuda):
    spec, ds, special = gc.stat_case(97, 256)
    f = BatchFitter(spec, cuda, FitOptions(max_iter=3, max_wg=3))
    res = f.fit(ds)
    assert _native.hip_loaded_path() is not None and f._native.grid == 3
    w = spec.coef(res.w.cpu())
    for col, kind in special.items():
        if kind == "const":
            assert float(res.std[col]) == 0.0 and bool((w[:, col] == 0).all())


# ---- 3. the chain on the diagonal ----------------------------------------------------------------
@pytest.mark.parametrize("reg", gc.CHAIN_REG)
@pytest.mark.parametrize("warm", [True, False], ids=["warm", "zero"])
@pytest.mark.parametrize("FP,K", gc.CHAIN_CELLS)
def test_chain_on_the_diagonal(cuda, FP, K, warm, reg):
    spec, ds, _ = gc.dense_fit_inputs(FP, K)
    ch, nat = gc.drive_dense(cuda, spec, ds, gc.dense_start(spec, warm), reg, max_wg=3)
    print(f"[FP{FP} K{K} {'warm' if warm else 'zero'} reg {reg}] evals {nat.evals} {ch.report()}")
    assert _native.hip_loaded_path() is not None and nat.grid == 3
    assert ch.steps == gc.CHAIN_STEPS and ch.pushes + ch.declined == gc.CHAIN_STEPS


def test_chain_where_line_searches_spend_their_budget(cuda):
    r = gc.RETRY
    spec, ds, _ = gc.dense_fit_inputs(r["FP"], r["K"])
    w0 = gc.dense_start(spec, True, scale=r["scale"])
    X, y = rows64(spec, ds)
    ref = fit_reference(X, y, spec.coef(w0), spec.intercept(w0), reg_param=r["reg"], tol=0.0,
                        max_iter=gc.CHAIN_STEPS + 1, ls_max=r["ls_max"])
    assert ref.ls_fail >= 1  # the oracle's own replay first
    ch, nat = gc.drive_dense(cuda, spec, ds, w0, r["reg"], ls_max=r["ls_max"])
    print(f"[retry] evals {nat.evals} ls_fail {nat.ls_fail} (oracle {ref.ls_fail}) {ch.report()}")
    assert _native.hip_loaded_path() is not None and nat.grid == _tiles(gc.N_ROWS)
    assert nat.ls_fail >= 1 and nat.evals > nat.accepted + 1
    assert ch.steps == gc.CHAIN_STEPS


# ---- 4. history depth ------------------------------------------------------------------------------
@pytest.mark.parametrize("H", gc.HIST)
def test_history_depth(cuda, H):
    N, F, K = gc.HIST_DENSE
    spec, ds, _ = gc.dense_fit_inputs(256, K, N=N, F=F, seed=gc.HIST_DENSE_SEED)
    reg = gc.HIST_REG
    ch, nat = gc.drive_dense(cuda, spec, ds, None, reg, hist=H, steps=gc.HIST_STEPS, max_wg=3)
    print(f"[hist {H}] evals {nat.evals} dir_reset {nat.dir_reset} {ch.report()}")
    assert _native.hip_loaded_path() is not None and nat.grid == 3
    assert ch.steps == gc.HIST_STEPS
    if nat.dir_reset == 0 and ch.declined == 0:
        assert ch.wraps == gc.HIST_STEPS - H
    # the first 4 steps against the oracle of the same depth
    X, y = rows64(spec, ds)
    ref = fit_reference(X, y, num_classes=K, reg_param=reg, max_iter=4, ls_max=6, hist=H)
    res = BatchFitter(spec, cuda, FitOptions(max_iter=4, ls_max=6, reg_param=reg, hist=H)).fit(ds)
    assert res.iters == ref.iters, (res.iters, ref.iters, res.evals, ref.evals)
    assert abs(res.objective - ref.objective) <= 1e-3 * max(1.0, abs(ref.objective))
    got, want = spec.coef(res.w.cpu()).double(), ref.coef
    err = float((got - want).abs().max() / want.abs().max())
    errb = float((spec.intercept(res.w.cpu()).double() - ref.intercept).abs().max() / ref.intercept.abs().max())
    print(f"[hist {H}] 4 steps: coefficient change err {err:.3e} intercepts {errb:.3e}")
    assert err <= 2e-2 and errb <= 2e-2


# ---- 5. zero_const = False -----------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.05])
def test_constant_columns_keep_their_start_without_zero_const(cuda, reg):
    spec, ds, const = gc.dense_fit_inputs(256, 3)
    w0 = warm_start(spec, seed=3)
    assert bool((spec.coef(w0)[:, const] != 0).all())
    ch, nat = gc.drive_dense(cuda, spec, ds, w0, reg, zero_const=False, max_wg=3)
    print(f"[zero_const off, reg {reg}] {ch.report()}")
    assert _native.hip_loaded_path() is not None and nat.grid == 3
    assert ch.steps == gc.CHAIN_STEPS
    wf = spec.coef(ch.prev["wfix"][: spec.P])
    assert torch.equal(wf[:, const], spec.coef(w0)[:, const]) and int((wf != 0).sum()) == spec.K
    X, y = rows64(spec, ds)
    ref = fit_reference(X, y, spec.coef(w0), spec.intercept(w0), reg_param=reg, max_iter=4, ls_max=6,
                        zero_const=False)
    res = BatchFitter(spec, cuda, FitOptions(max_iter=4, ls_max=6, reg_param=reg, zero_const=False)).fit(ds, w0=w0)
    assert res.iters == ref.iters and len(res.history) == len(ref.history)
    for a, b in zip(res.history, ref.history):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b))
    got = spec.coef(res.w.cpu())[:, const].double()
    want = ref.coef[:, const]
    assert bool((want != 0).all())
    assert bool(((got - want).abs() <= 2.0 ** -22 * want.abs().max()).all()), (got, want)
    if reg != 0.0:  # not centred: the start's own values, bit for bit
        assert torch.equal(spec.coef(res.w.cpu())[:, const], spec.coef(w0)[:, const])

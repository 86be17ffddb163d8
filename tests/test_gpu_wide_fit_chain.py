"""The wide full-batch fitter (csrc/kernels/wide_fit_kernels.hip, csrc/solver/wide_fit.hip)
iterated at every padded class count under the invariant chain of _fit_chain.py, and
evaluated where its loops change form:

  * the chain over 6 accepted steps at K in {1, 2, 3, 6, 16} (KP 1, 2, 4, 8, 16) with
    col_chunk in {64, default}, max_wg in {3, default}, with the full columns and with
    the empty row;
  * columns of exactly 1, 31, 32, 33, 63, 64, 65 and 129 entries (one with a repeated
    cell) at col_chunk in {1, 32, 33, 2048} and every KP: the short / long item split
    at ``wide_fit_short``;
  * a dataset whose vectors exceed one trip of the reduction (``wide_fit_reduce_cap``
    elements), so its grid-stride loop runs: one evaluation, sigma, 3 chain steps;
  * history depths 1, 2, 10, 16 over 20 accepted steps; ``zero_const = False``.

Tables and seeds: _fit_geometry_cases.py; their conditions: test_fit_chain_cpu.py."""
import random

import pytest
import torch

import _fit_geometry_cases as gc
from _fit_chain import WideProblem
from _fit_geometry_cases import wc
from psx import _native
from psx.models.wide import WideSpec
from psx.ops.fit import FitOptions
from psx.ops.lr import stream_handle
from psx.ops.sparse import SparseDataset
from psx.ops.wide_fit import WideFitter

pytestmark = pytest.mark.gpu


def _grid(N, max_wg):
    return min((N + 3) // 4, max_wg) if max_wg else None


# ---- 1. the chain at every KP ------------------------------------------------------------------------
@pytest.mark.parametrize("full", [True, False], ids=["full_cols", "empty_row"])
@pytest.mark.parametrize("max_wg", gc.WIDE_WG)
@pytest.mark.parametrize("col_chunk", gc.WIDE_CHUNK)
@pytest.mark.parametrize("K", gc.WIDE_K)
def test_chain_at_every_padded_class_count(cuda, K, col_chunk, max_wg, full):
    N, F = gc.WIDE_SHAPE
    spec, ds = wc.sparse_case(N, F, K, full_cols=full)
    if not full:
        assert int(ds.indptr[4] - ds.indptr[3]) == 0  # the empty row
    ch, nat, d = gc.drive_wide(cuda, spec, ds, None, 0.05, max_wg=max_wg, col_chunk=col_chunk)
    print(f"[wide K{K} KP{spec.KP} chunk {col_chunk} wg {max_wg} full {full}] items {d.n_items} short "
          f"{d.short_items.numel()} long {d.long_items.numel()} evals {nat.evals} {ch.report()}")
    assert _native.hip_loaded_path() is not None
    if max_wg:
        assert nat.grid == _grid(N, max_wg)
    assert d.long_items.numel() > 0 and d.short_items.numel() > 0
    assert ch.steps == gc.CHAIN_STEPS


# ---- 2. directed column lengths -------------------------------------------------------------------------
LENGTHS = (1, 31, 32, 33, 63, 64, 65, 129)
N_DIRECTED = 131


def directed_case(K):
    """Column c (feature 7 c + 3) holds exactly LENGTHS[c] entries in rows drawn without
    replacement; the 33-entry column holds 32 distinct rows, one of them twice."""
    g = torch.Generator().manual_seed(9001 + K)
    F = 100
    rows, cols, vals = [], [], []
    for c, L in enumerate(LENGTHS):
        r = torch.randperm(N_DIRECTED, generator=g)[: L if L != 33 else 32]
        if L == 33:
            r = torch.cat([r, r[:1]])
        rows.append(r)
        cols.append(torch.full((L,), 7 * c + 3, dtype=torch.long))
        vals.append(torch.randn(L, generator=g))
    rows, cols, vals = torch.cat(rows), torch.cat(cols), torch.cat(vals)
    order = torch.sort(rows, stable=True).indices
    indptr = torch.zeros(N_DIRECTED + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N_DIRECTED), 0)
    y = torch.randint(0, max(K, 2), (N_DIRECTED,), generator=g).to(torch.int32)
    return WideSpec(F, K), SparseDataset(indptr, cols[order].to(torch.int32), vals[order].to(torch.bfloat16), y, F)


def expected_items(col_chunk, short_max):
    short = long = 0
    for L in LENGTHS:
        full, rest = divmod(L, col_chunk)
        for n in [col_chunk] * full + ([rest] if rest else []):
            if n <= short_max:
                short += 1
            else:
                long += 1
    return short, long


@pytest.mark.parametrize("col_chunk", [1, 32, 33, 2048])
@pytest.mark.parametrize("K", gc.WIDE_K)
def test_directed_column_lengths(cuda, K, col_chunk):
    spec, ds = directed_case(K)
    counts = torch.bincount(ds.idx.long(), minlength=spec.F)
    assert sorted(int(c) for c in counts[counts > 0]) == list(LENGTHS)
    w = wc.eval_weights(spec, wscale=0.5)
    loss64, g64, bl, bg, _ = wc.eval_oracle(spec, ds, w)
    f = WideFitter(spec, cuda, FitOptions(max_wg=3), col_chunk=col_chunk)
    loss, g = f.loss_grad(ds, w.to(cuda))
    d = f._data
    short_max = int(_native.hip().wide_fit_short)
    assert (int(d.short_items.numel()), int(d.long_items.numel())) == expected_items(col_chunk, short_max)
    assert _native.hip_loaded_path() is not None and f._native.grid == 3
    err = (g.cpu().double() - g64).abs()
    print(f"[directed K{K} chunk {col_chunk}] short {d.short_items.numel()} long {d.long_items.numel()} "
          f"loss err {abs(loss - loss64):.3e} (bound {bl:.3e}) largest grad err/bound "
          f"{float((err / bg.clamp_min(1e-300)).max()):.3f}")
    assert abs(loss - loss64) <= bl
    assert bool((err <= bg).all())


# ---- 3. the reduction's second trip ------------------------------------------------------------------------
def stride_case():
    N, per, F, K = 700, 40, 1 << 20, 16
    g = torch.Generator().manual_seed(20240)
    rnd = random.Random(20240)
    idx = torch.tensor([rnd.sample(range(F), per) for _ in range(N)]).view(-1)
    v = torch.randn(N * per, generator=g)
    v = torch.sign(v) * (v.abs() + 0.1) / per ** 0.5
    y = torch.randint(0, K, (N,), generator=g).to(torch.int32)
    return WideSpec(F, K), SparseDataset(torch.arange(N + 1, dtype=torch.int64) * per, idx.to(torch.int32),
                                         v.to(torch.bfloat16), y, F)


def test_the_reduction_takes_its_second_trip(cuda):
    spec, ds = stride_case()
    p = WideProblem(spec, ds, 0.05, compact=True)
    cap = int(_native.hip().wide_fit_reduce_cap)
    assert p.U > 26000 and p.n > cap  # elements beyond one trip of the capped grid
    # one evaluation under the bound (the oracle on the touched columns)
    g = torch.Generator().manual_seed(3)
    wc_, wb = torch.randn(spec.K, p.U, generator=g) * 0.5, torch.randn(spec.K, generator=g) * 0.5
    w = torch.zeros(spec.P)
    w[: spec.F * spec.KP].view(spec.F, spec.KP)[p.f, : spec.K] = wc_.t()
    w[spec.F * spec.KP: spec.F * spec.KP + spec.K] = wb
    loss64, g64, bl, bg, _ = wc.eval_oracle(p.ospec, p.ods, p.ospec.pack(wc_, wb))
    f = WideFitter(spec, cuda, FitOptions(max_wg=3))
    loss, gd = f.loss_grad(ds, w.to(cuda))
    gd = gd.cpu()
    got = torch.cat([gd[: spec.F * spec.KP].view(spec.F, spec.KP)[p.f].reshape(-1), gd[spec.F * spec.KP:]]).double()
    err = (got - g64).abs()
    print(f"[stride] U {p.U} n {p.n} loss err {abs(loss - loss64):.3e} (bound {bl:.3e}) largest grad err/bound "
          f"{float((err / bg.clamp_min(1e-300)).max()):.3f}")
    assert abs(loss - loss64) <= bl and bool((err <= bg).all())
    rest = gd[: spec.F * spec.KP].view(spec.F, spec.KP).clone()
    rest[p.f] = 0
    assert not bool(rest.any())  # nothing outside the touched features
    assert _native.hip_loaded_path() is not None and f._native.grid == 3 and f._native.n == p.n
    # sigma, two-pass
    std = torch.empty(p.U, dtype=torch.float32, device=f.device)
    f._native.read_std(std.data_ptr(), stream_handle(f.device))
    assert torch.allclose(std.cpu().double(), p.sigma, rtol=1e-6, atol=0)
    # three steps of the chain
    ch, nat, _ = gc.drive_wide(cuda, spec, ds, None, 0.05, steps=3, max_wg=3, problem=p)
    print(f"[stride] evals {nat.evals} {ch.report()}")
    assert ch.steps == 3 and nat.grid == 3


# ---- 4. history depth ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", gc.HIST)
def test_history_depth(cuda, H):
    spec, ds = wc.sparse_case(*gc.HIST_WIDE, seed=gc.HIST_WIDE_SEED)
    reg = gc.HIST_REG
    ch, nat, _ = gc.drive_wide(cuda, spec, ds, None, reg, hist=H, steps=gc.HIST_STEPS, max_wg=3)
    print(f"[wide hist {H}] evals {nat.evals} dir_reset {nat.dir_reset} {ch.report()}")
    assert _native.hip_loaded_path() is not None and nat.grid == 3
    assert ch.steps == gc.HIST_STEPS
    if nat.dir_reset == 0 and ch.declined == 0:
        assert ch.wraps == gc.HIST_STEPS - H
    feats, ref = wc.oracle_fit(spec, ds, reg_param=reg, max_iter=4, ls_max=6, hist=H)
    res = WideFitter(spec, cuda, FitOptions(max_iter=4, ls_max=6, reg_param=reg, hist=H)).fit(ds)
    assert res.iters == ref.iters, (res.iters, ref.iters, res.evals, ref.evals)
    assert abs(res.objective - ref.objective) <= 1e-3 * max(1.0, abs(ref.objective))
    w = res.w.cpu()
    got = spec.coef(w)[:, feats].double()
    err = float((got - ref.coef).abs().max() / ref.coef.abs().max())
    errb = float((spec.intercept(w).double() - ref.intercept).abs().max() / ref.intercept.abs().max())
    print(f"[wide hist {H}] 4 steps: coefficient change err {err:.3e} intercepts {errb:.3e}")
    assert err <= 2e-2 and errb <= 2e-2


# ---- 5. zero_const = False --------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.05])
def test_constant_columns_keep_their_start_without_zero_const(cuda, reg):
    N, F = gc.WIDE_SHAPE
    spec, ds = wc.sparse_case(N, F, 3)
    w0 = wc.warm_start(spec, seed=3)
    assert bool((spec.coef(w0)[:, 0] != 0).all())  # feature 0 is 1.5 in every row
    ch, nat, _ = gc.drive_wide(cuda, spec, ds, w0, reg, zero_const=False, max_wg=3)
    print(f"[wide zero_const off, reg {reg}] {ch.report()}")
    assert _native.hip_loaded_path() is not None and nat.grid == 3
    assert ch.steps == gc.CHAIN_STEPS
    wf = ch.prev["wfix"][: ch.p.n].view(ch.p.U + 1, spec.KP)
    assert ch.p.f[0] == 0 and torch.equal(wf[0, : spec.K], spec.coef(w0)[:, 0]) and int((wf != 0).sum()) == spec.K
    feats, ref = wc.oracle_fit(spec, ds, w0, reg_param=reg, max_iter=4, ls_max=6, zero_const=False)
    res = WideFitter(spec, cuda, FitOptions(max_iter=4, ls_max=6, reg_param=reg, zero_const=False)).fit(ds, w0=w0)
    assert res.iters == ref.iters and len(res.history) == len(ref.history)
    for a, b in zip(res.history, ref.history):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b))
    got = spec.coef(res.w.cpu())[:, 0].double()
    want = ref.coef[:, 0]
    assert bool((want != 0).all())
    assert bool(((got - want).abs() <= 2.0 ** -22 * want.abs().max()).all()), (got, want)
    if reg != 0.0:
        assert torch.equal(spec.coef(res.w.cpu())[:, 0], spec.coef(w0)[:, 0])

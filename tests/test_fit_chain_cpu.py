"""The chain checker of _fit_chain.py on states built in float64 (no GPU): it accepts
a correct state and names the broken link of a state with one planted defect; and the
conditions on the inputs of the GPU sweeps (_fit_geometry_cases.py), which are all
properties of the float64 reference."""
import pytest
import torch

import _fit_geometry_cases as gc
from _fit_chain import Chain, ChainError, DenseProblem, WideProblem, emulate, two_loop
from _fit_geometry_cases import wc
from psx import _native
from psx.models.logreg import ModelSpec
from psx.models.reference import fit_reference
from psx.models.wide import WideSpec

H_SELF, STEPS_SELF = 3, 8  # the ring wraps twice


def _hip_or_skip():
    try:
        return _native.hip()
    except RuntimeError as e:  # extension not built
        pytest.skip(str(e))


_STATE = {}


def _synthetic():
    if not _STATE:
        spec, ds, _ = gc.dense_fit_inputs(128, 3, seed=1)
        p = DenseProblem(spec, ds, 0.05)
        _STATE["p"] = p
        _STATE["snaps"] = emulate(p, gc.dense_x0(p, gc.dense_start(spec, True)), H_SELF, STEPS_SELF)
    return _STATE["p"], [dict(s) for s in _STATE["snaps"]]


def _feed(p, snaps):
    ch = Chain(p, H_SELF)
    ch.begin(snaps[0])
    for s in snaps[1:]:
        ch.step(s, current=p.finalize(s["x"][: p.n].double(), s["wfix"][: p.n].double()).float())
    return ch


def test_a_correct_state_passes():
    p, snaps = _synthetic()
    ch = _feed(p, snaps)
    print(ch.report())
    assert ch.steps == STEPS_SELF and ch.pushes == STEPS_SELF and ch.wraps == STEPS_SELF - H_SELF
    assert max(t for t, _ in ch.dir_tol) <= 1e-3


def _slot_of_push(snaps, i):
    return [j for j in range(H_SELF) if not torch.equal(snaps[i]["S"][j], snaps[i - 1]["S"][j])][0]


def test_one_element_of_S_off_by_2m10_fails_the_pair_link():
    p, snaps = _synthetic()
    i = 5
    j = _slot_of_push(snaps, i)
    k = int(snaps[i]["S"][j].abs().argmax()) // 2 + 1
    assert snaps[i]["S"][j][k] != 0
    for s in snaps[i:]:
        s["S"] = s["S"].clone()
    snaps[i]["S"][j][k] *= 1.0 + 2.0 ** -10
    with pytest.raises(ChainError) as e:
        _feed(p, snaps)
    assert e.value.link == 2


def test_a_pair_dropped_from_the_two_loop_fails_the_direction_link():
    p, snaps = _synthetic()
    i, n = 5, p.n
    s = snaps[i]
    order = [(_slot_of_push(snaps, k)) for k in range(i - H_SELF + 1, i + 1)]  # the live pairs, oldest first
    keep = order[1:]
    d = two_loop([s["S"][j][:n].double() for j in keep], [s["Y"][j][:n].double() for j in keep], s["g_c"][:n].double())
    s["d"] = s["d"].clone()
    s["d"][:n] = d.float()
    s["beta_t"] = s["beta_t"].clone()
    s["beta_t"][:n] = (s["x"][:n].double() + s["d"][:n].double()).float()
    with pytest.raises(ChainError) as e:
        _feed(p, snaps)
    assert e.value.link == 3


def test_Y_written_one_slot_further_fails_the_pair_link():
    p, snaps = _synthetic()
    i = 5
    j = _slot_of_push(snaps, i)
    s = snaps[i]
    s["Y"] = s["Y"].clone()
    s["Y"][(j + 1) % H_SELF] = s["Y"][j]
    s["Y"][j] = snaps[i - 1]["Y"][j]
    with pytest.raises(ChainError) as e:
        _feed(p, snaps)
    assert e.value.link == 2


def test_one_reduce_workgroup_of_g_c_zeroed_fails_the_gradient_link():
    p, snaps = _synthetic()
    s = snaps[4]
    s["g_c"] = s["g_c"].clone()
    s["g_t"] = s["g_t"].clone()
    s["g_c"][64:128] = 0
    s["g_t"][64:128] = 0
    with pytest.raises(ChainError) as e:
        _feed(p, snaps)
    assert e.value.link == 1


def test_a_live_slot_overwritten_early_fails_the_pair_link():
    p, snaps = _synthetic()
    s = snaps[2]  # two pairs live of three: the second push lands on the first one's slot
    j1, j2 = _slot_of_push(snaps, 1), _slot_of_push(snaps, 2)
    for k in ("S", "Y"):
        s[k] = s[k].clone()
        s[k][j1] = s[k][j2]
        s[k][j2] = 0
    with pytest.raises(ChainError) as e:
        _feed(p, snaps)
    assert e.value.link == 2


# ---- the tables against the bindings ----------------------------------------------------------------
def test_tables_match_the_bindings():
    h = _hip_or_skip()
    assert all(h.fp_supported(FP) for FP in gc.FPS) and not h.fp_supported(64) and not h.fp_supported(4096)
    assert {ModelSpec(F, K).Fp for F, K in gc.EVAL_CELLS} == set(gc.FPS)
    assert len(gc.EVAL_CELLS) == 29 and len(set(gc.EVAL_CELLS)) == 29
    for FP, K in gc.CHAIN_CELLS:
        assert ModelSpec(gc.F_OF[FP], K).Fp == FP
    assert h.wide_fit_short == 32
    assert h.wide_fit_reduce_cap == 1024 * 256
    assert [WideSpec(5000, K).KP for K in gc.WIDE_K] == [1, 2, 4, 8, 16]
    assert max(gc.HIST) == 16 and gc.HIST_STEPS > max(gc.HIST)  # every ring wraps
    assert 3 + 2 * max(gc.HIST) + 1 == 36


# ---- conditions on the inputs (the float64 reference alone) -----------------------------------------
def _condition(p, x0, H, steps):
    snaps = emulate(p, x0, H, steps)
    ch = Chain(p, H)
    ch.begin(snaps[0])
    for s in snaps[1:]:
        ch.step(s)
    worst = max(t for t, _ in ch.dir_tol)
    assert worst <= 1e-3, worst
    return ch


@pytest.mark.parametrize("reg", gc.CHAIN_REG)
@pytest.mark.parametrize("warm", [True, False], ids=["warm", "zero"])
@pytest.mark.parametrize("FP,K", gc.CHAIN_CELLS)
def test_dense_chain_inputs_meet_the_direction_condition(FP, K, warm, reg):
    spec, ds, _ = gc.dense_fit_inputs(FP, K)
    p = DenseProblem(spec, ds, reg)
    ch = _condition(p, gc.dense_x0(p, gc.dense_start(spec, warm)), 10, gc.CHAIN_STEPS)
    print(f"[{FP} K{K} warm {warm} reg {reg}] {ch.report()}")


@pytest.mark.parametrize("full", [True, False], ids=["full_cols", "empty_row"])
@pytest.mark.parametrize("K", gc.WIDE_K)
def test_wide_chain_inputs_meet_the_direction_condition(K, full):
    spec, ds = wc.sparse_case(*gc.WIDE_SHAPE, K, full_cols=full)
    p = WideProblem(spec, ds, 0.05)
    ch = _condition(p, gc.wide_x0(p, None), 10, gc.CHAIN_STEPS)
    print(f"[wide K{K} full {full}] {ch.report()}")


@pytest.mark.parametrize("H", gc.HIST)
def test_history_inputs_meet_the_direction_condition(H):
    N, F, K = gc.HIST_DENSE
    spec, ds, _ = gc.dense_fit_inputs(256, K, N=N, F=F, seed=gc.HIST_DENSE_SEED)
    p = DenseProblem(spec, ds, gc.HIST_REG)
    ch = _condition(p, gc.dense_x0(p, None), H, gc.HIST_STEPS)
    assert ch.wraps == gc.HIST_STEPS - H
    spec, ds = wc.sparse_case(*gc.HIST_WIDE, seed=gc.HIST_WIDE_SEED)
    p = WideProblem(spec, ds, gc.HIST_REG)
    ch = _condition(p, gc.wide_x0(p, None), H, gc.HIST_STEPS)
    assert ch.wraps == gc.HIST_STEPS - H


def test_history_depths_are_distinguishable_on_the_oracle():
    """hist 1 against hist 16 after 20 steps: the float64 iterates differ by more than
    10 x the 2e-2 trajectory tolerance (relative to the larger coefficient change)."""
    N, F, K = gc.HIST_DENSE
    spec, ds, _ = gc.dense_fit_inputs(256, K, N=N, F=F, seed=gc.HIST_DENSE_SEED)
    X, y = gc.fc.rows64(spec, ds)
    kw = dict(num_classes=K, reg_param=gc.HIST_REG, tol=0.0, max_iter=gc.HIST_STEPS)
    a, b = fit_reference(X, y, hist=1, **kw), fit_reference(X, y, hist=16, **kw)
    gap = float((a.coef - b.coef).abs().max() / max(a.coef.abs().max(), b.coef.abs().max()))
    print(f"dense hist 1 vs 16: gap {gap:.3f}")
    assert a.iters == b.iters == gc.HIST_STEPS and gap >= 10 * 2e-2
    wspec, wds = wc.sparse_case(*gc.HIST_WIDE, seed=gc.HIST_WIDE_SEED)
    _, a = wc.oracle_fit(wspec, wds, hist=1, reg_param=gc.HIST_REG, tol=0.0, max_iter=gc.HIST_STEPS)
    _, b = wc.oracle_fit(wspec, wds, hist=16, reg_param=gc.HIST_REG, tol=0.0, max_iter=gc.HIST_STEPS)
    gap = float((a.coef - b.coef).abs().max() / max(a.coef.abs().max(), b.coef.abs().max()))
    print(f"wide hist 1 vs 16: gap {gap:.3f}")
    assert a.iters == b.iters == gc.HIST_STEPS and gap >= 10 * 2e-2


def test_the_retry_start_spends_a_line_search_budget_on_the_oracle():
    r = gc.RETRY
    spec, ds, _ = gc.dense_fit_inputs(r["FP"], r["K"])
    w0 = gc.dense_start(spec, True, scale=r["scale"])
    X, y = gc.fc.rows64(spec, ds)
    ref = fit_reference(X, y, spec.coef(w0), spec.intercept(w0), reg_param=r["reg"], tol=0.0,
                        max_iter=gc.CHAIN_STEPS + 1, ls_max=r["ls_max"])
    print(f"retry: iters {ref.iters} evals {ref.evals} ls_fail {ref.ls_fail} reason {ref.reason}")
    assert ref.ls_fail >= 1 and ref.iters == gc.CHAIN_STEPS + 1


def test_the_adjacent_value_column_loses_digits_in_one_pass():
    for N in gc.STAT_ROWS:
        spec, ds, special = gc.stat_case(N, 128)
        col = [f for f, kind in special.items() if kind == "adjacent"][0]
        x = ds.X[:, col].double()
        assert float(x.mean() / x.std()) > 190 or N == 2
        assert gc.one_pass_loss(x) < 1e-9  # float64 has room: the 1e-6 of the test is not consumed by it

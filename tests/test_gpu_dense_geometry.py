"""The dense solve kernels at every padded-width / class-count geometry.

The streaming solve (csrc/kernels/solve_kernels.hip, lanes_kernels.hip) is compiled once
per padded feature width FP in {128, 256, 512, 1024, 2048} and padded class count KP in
{2, 4, 8, 16}, in six forms: the launch chain (eager / one hipGraph), the one-launch
persistent solve (FP <= 1024, KP <= 8), the row-parallel form on bf16 and on fp32 rows
(fp32: FP <= 1024), the multi-lane round kernel (FP <= 1024, K <= 8) and the evaluation
bodies.  ``_dense_cases.TABLE`` holds one (F, K) per cell; CPU tests hold the table to the
code and the inputs to the stability condition of the float64 oracle.  On the GPU every
form solves every cell it supports against ``local_solve_reference`` with the tolerances of
test_gpu_kernels.py ``test_local_solve_matches_reference`` / ``test_persistent_solve_
matches_chain``, asserts the form that actually ran, and checks the output's structure:
padded features exactly 0, the constant column's delta exactly -w_old, a one-row window
moving only the intercepts, centred intercept deltas.  Evaluation counts are exact against
float64 decisions on rows that are safe by ``_score_cases``' margin bound.

(The asynchronous lanes kernel is not covered here: its float64 replay in
test_gpu_async_lanes.py builds its own dataset inline; profiles/r14/README.md.)
"""
import ctypes

import pytest
import torch

import _dense_cases as dc
from _dense_cases import CAP, DIAGONAL, ENTRIES, F_OF, K_OF, RETRY_CELLS, ROWS, SPREAD, TABLE, W0, cell, ident
from _score_cases import dense_case, oracle as decisions64, safe_rows
from psx import _native
from psx.models.logreg import ModelSpec
from psx.ops.lr import EvalScratch, EvalSet, Fragments, LocalSolveOp, stream_handle
from psx.runtime.buffer import DeviceRing


def _hip_or_skip():
    try:
        return _native.hip()
    except RuntimeError as e:  # extension not built
        pytest.skip(str(e))


# ---------------------------------------------------------------------------
# CPU: the table against the code, the inputs against the oracle's own stability
def test_geometry_table_matches_the_code():
    h = _hip_or_skip()
    assert len(TABLE) == 20 and len({(e.FP, e.KP) for e in TABLE}) == 20
    seen = {"FP": set(), "KP": set(), "forms": set()}
    for e in ENTRIES:
        spec = ModelSpec(e.F, e.K)
        assert spec.Fp == e.FP, f"{ident(e)}: the table says FP {e.FP}, the model pads to {spec.Fp}"
        assert dc.padded_classes(e.K) == e.KP
        assert spec.P == e.K * e.FP + e.K
        got = bool(h.lanes_supported(e.FP, e.K, dc.LANES_CAP))
        assert got == ("lanes" in e.forms), f"{ident(e)}: lanes_supported says {got}"
        assert {"chain", "graph", "rows_bf16"} <= e.forms
        seen["FP"].add(e.FP)
        seen["KP"].add(e.KP)
        seen["forms"] |= e.forms
    assert seen["FP"] == set(F_OF) and seen["KP"] == set(K_OF) and seen["forms"] == set(dc.FORMS)
    for e in TABLE:  # real sizes that are not the padded ones wherever the cell allows it
        assert e.F < e.FP and (e.K < e.KP or e.KP == 2)
    for form in dc.FORMS:  # every width and class count the form supports keeps a case
        mine = [e for e in ENTRIES if form in e.forms]
        fps = {e.FP for e in mine}
        kps = {e.KP for e in mine}
        assert fps == ({128, 256, 512, 1024} if form in ("persist", "rows_fp32", "lanes") else set(F_OF)), (form, fps)
        assert kps == ({2, 4, 8} if form in ("persist", "lanes") else set(K_OF)), (form, kps)
    assert not h.lanes_supported(1024, 9, dc.LANES_CAP) and not h.lanes_supported(2048, 2, dc.LANES_CAP)
    assert CAP % 32 == 0 and dc.LANES_CAP % 32 == 0 and SPREAD["cap"] % 32 == 0
    B, start = SPREAD["window"]
    assert ((start & 31) + B + 31) >> 5 == 34  # more window tiles than one XCD has workgroups (32)


_SOLVE_CASES = dc.solve_cases()


@pytest.mark.parametrize("F,K,rows,idx,model,retries", [c[:6] for c in _SOLVE_CASES], ids=[c[6] for c in _SOLVE_CASES])
def test_inputs_are_stable_on_the_oracle(F, K, rows, idx, model, retries):
    """Every (case, window, model) the GPU tests solve: with w_old perturbed by 2^-18 relative,
    and with its evaluations in float32, the oracle keeps (evals, accepted) and moves by
    <= 5e-3 of the delta's scale and 2.5e-4 max(1, |loss|); the retry model's line searches
    retry; fp32 rounding leaves room for the intercept deltas' sum (_dense_cases.stable)."""
    ok, fig = dc.stable(F, K, idx, model, rows, retries)
    print(fig)
    assert ok, fig


# ---------------------------------------------------------------------------
# GPU: the solve
_FORM_OPTS = {
    "chain": dict(use_graph=False, persist=False),
    "graph": dict(use_graph=True, persist=False),
    "persist": dict(use_graph=False, persist=True),
    "rows_bf16": dict(),
    "rows_fp32": dict(),
}


def _ring(cuda, ds, cap, dtype="bf16"):
    d = ds.as_dtype(dtype)
    ring = DeviceRing(cap, ds.Fp, cuda, dtype=dtype)
    ring.place(d.X[:cap], d.y[:cap], 0)  # slot i holds row i
    return ring


def _assert_form(op, ran):
    n = op._native
    got = ("rows" if n.rows_mode else "persist" if n.persistent else "chain" if n.eager else "graph")
    assert got == ran.split("_")[0], f"asked for {ran}, the solver ran {got}"
    assert bool(n.eager) == (ran != "graph")


def _check(tag, spec, const, op, w_old, ref, B):
    """The tolerances of test_local_solve_matches_reference + the exact structure of the output."""
    delta, stats, loss = op.delta.cpu(), op.stats.cpu().tolist(), op.loss.item()
    c, b = spec.coef(delta), spec.intercept(delta)
    sc = max(ref.delta_coef.abs().max().item(), 1e-6)
    sb = max(ref.delta_intercept.abs().max().item(), 1e-6)
    err = (c - ref.delta_coef).abs().max().item() / sc
    errb = (b - ref.delta_intercept).abs().max().item() / sb
    bsum = abs(b.double().sum().item()) / sb
    print(f"FIG {tag} B={B} evals={stats[0]}/{ref.evals} acc={stats[1]}/{ref.accepted} err={err:.3e} errb={errb:.3e} "
          f"dloss={abs(loss - ref.loss):.3e} loss={ref.loss:.6g} bsum={bsum:.3e}")
    assert stats[0] == ref.evals and stats[1] == ref.accepted, (stats, ref.evals, ref.accepted)
    assert abs(loss - ref.loss) < 1e-3 * max(1.0, abs(ref.loss)), (loss, ref.loss)
    assert err <= 2e-2 and errb <= 2e-2, (err, errb)
    assert op.barrier_errors() == 0 and stats[4] == 0
    F, K, Fp = spec.F, spec.K, spec.Fp
    pad = delta[: K * Fp].view(K, Fp)[:, F:]
    assert pad.numel() == 0 or pad.abs().max().item() == 0.0  # (a)
    if const is not None:
        assert torch.equal(c[:, const], -spec.coef(w_old)[:, const])  # (b)
    if B == 1:
        assert torch.equal(c, -spec.coef(w_old))  # (c)
    assert bsum <= 1e-5, bsum  # (d)
    return delta, loss, stats


def _solve(cuda, e, form, model, windows, ran=None, cap=CAP, rows=ROWS, xcd=0, tag=None):
    """One op and ring of the form; the windows solved consecutively, each against the oracle."""
    spec, ds, const = dc.window_case(e.F, e.K, rows)
    ring = _ring(cuda, ds, cap, "fp32" if form == "rows_fp32" else "bf16")
    if form.startswith("rows"):
        assert ring.rows_mode and ring.XT is None
    op = LocalSolveOp(spec, cap, cuda, dc.options(model, xcd=xcd, **_FORM_OPTS[form]))
    w = dc.start_model(spec, model)
    wd = w.to(cuda)
    out = []
    for B, start in windows:
        op.run(ring, B, start, wd)
        torch.cuda.synchronize()
        _assert_form(op, ran or form)
        ref = dc.oracle(e.F, e.K, dc.window_rows((B, start), cap), model, rows=rows)
        out.append(_check(f"form={tag or form} cell={ident(e)} model={model} win={B}@{start}", spec, const, op, w,
                          ref, B))
    return out, (op, ring, wd)


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1] == b[1] and a[2][:5] == b[2][:5]


def _windows(FP, KP, model):
    w = list(dc.windows_of(model))
    if (FP, KP) == dc.ONE_CELL and model == "small":
        w.append(dc.W_ONE)
    return w


def _with_models(entries, retry=lambda e: (e.FP, e.KP) in RETRY_CELLS and e in TABLE):
    out = [(e, "small") for e in entries] + [(e, "retry") for e in entries if retry(e)]
    return dict(argvalues=out, ids=[f"{ident(e)}-{m}" for e, m in out])


@pytest.mark.gpu
@pytest.mark.parametrize("e,model", **_with_models(ENTRIES, retry=lambda e: True))
def test_chain_matches_oracle(cuda, e, model):
    _solve(cuda, e, "chain", model, [W0])


@pytest.mark.gpu
@pytest.mark.parametrize("model", list(dc.MODELS))
@pytest.mark.parametrize("FP,KP", DIAGONAL)
def test_chain_window_shapes_consecutively(cuda, FP, KP, model):
    """Three tiles and a row, full + wrapped, wrapping the ring's end, two rows (and one row)
    on one op and ring; the last window's result equals a fresh op's bit for bit."""
    e, wins = cell(FP, KP), _windows(FP, KP, model)
    out, _ = _solve(cuda, e, "chain", model, wins)
    fresh, _ = _solve(cuda, e, "chain", model, wins[-1:])
    assert _same(out[-1], fresh[0])


@pytest.mark.gpu
@pytest.mark.parametrize("model", list(dc.MODELS))
@pytest.mark.parametrize("FP,KP", DIAGONAL)
def test_graph_equals_eager_chain(cuda, FP, KP, model):
    e, wins = cell(FP, KP), _windows(FP, KP, model)
    eager, _ = _solve(cuda, e, "chain", model, wins)
    graph, _ = _solve(cuda, e, "graph", model, wins)
    for win, a, b in zip(wins, eager, graph):
        assert _same(a, b), (win, (a[0] - b[0]).abs().max().item(), a[1], b[1], a[2], b[2])


def _persist_vs_chain(tag, pers, chain):
    """The tolerances of test_persistent_solve_matches_chain."""
    for (dp, lp, sp), (dk, lk, sk) in zip(pers, chain):
        scale = dk.abs().max().item()
        gap = (dp - dk).abs().max().item() / scale
        print(f"GAP {tag} persist-vs-chain={gap:.3e} dloss={abs(lp - lk):.3e}")
        assert sp[:4] == sk[:4] and sp[4] == 0, (sp, sk)
        assert gap <= 2e-3, gap
        assert abs(lp - lk) <= 1e-4 * max(1.0, abs(lk))


_PERSIST = [e for e in TABLE if "persist" in e.forms]


@pytest.mark.gpu
@pytest.mark.parametrize("e,model", **_with_models(_PERSIST, retry=lambda e: True))
def test_persistent_matches_oracle_and_chain(cuda, e, model):
    """Both starts at all 12 supported cells.  (The retry start at F 300 / K 2 and K 3 is the
    regression case of the padded classes' curvature pairs: the persistent forms read them
    from LDS words nobody had written, at KP 2 and 4 -- profiles/r14/README.md.)"""
    wins = _windows(e.FP, e.KP, model) if (e.FP, e.KP) in DIAGONAL else [W0]
    pers, _ = _solve(cuda, e, "persist", model, wins)
    chain, _ = _solve(cuda, e, "chain", model, wins)
    _persist_vs_chain(f"cell={ident(e)} model={model}", pers, chain)


@pytest.mark.gpu
@pytest.mark.parametrize("e", [e for e in TABLE if "persist" not in e.forms], ids=ident)
def test_persistent_request_runs_the_chain_where_unsupported(cuda, e):
    """K >= 9 (KP 16) and FP 2048 have no persistent kernel: the request runs the chain."""
    _solve(cuda, e, "persist", "small", [W0], ran="chain", tag="persist->chain")


@pytest.mark.gpu
def test_persistent_spread_form_away_from_1024(cuda):
    """34 window tiles at FP 256: more cooperating workgroups than one XCD holds, so the
    persistent solve spreads over the XCDs (sc1 hand-offs)."""
    e, cap, win = cell(*SPREAD["cell"]), SPREAD["cap"], SPREAD["window"]
    pers, _ = _solve(cuda, e, "persist", "small", [win], cap=cap, rows=cap, tag="persist-spread")
    chain, _ = _solve(cuda, e, "chain", "small", [win], cap=cap, rows=cap, tag="chain-1050")
    _persist_vs_chain("spread", pers, chain)


@pytest.mark.gpu
def test_persistent_placement_bit_equal(cuda):
    e, wins = cell(512, 4), [W0, (128, 100)]
    outs = {x: _solve(cuda, e, "persist", "small", wins, xcd=x, tag=f"persist-xcd{x}")[0] for x in (0, 3, -1)}
    for x in (3, -1):
        for a, b in zip(outs[0], outs[x]):
            assert _same(a, b), x


@pytest.mark.gpu
@pytest.mark.parametrize("e,model", **_with_models(TABLE))
def test_rows_bf16_matches_oracle(cuda, monkeypatch, e, model):
    monkeypatch.setenv("PSX_SOLVER_ROWS", "1")
    _solve(cuda, e, "rows_bf16", model, [W0])


@pytest.mark.gpu
@pytest.mark.parametrize("e,model", **_with_models([e for e in TABLE if "rows_fp32" in e.forms]))
def test_rows_fp32_matches_oracle(cuda, e, model):
    _solve(cuda, e, "rows_fp32", model, [W0])


@pytest.mark.gpu
@pytest.mark.parametrize("FP,KP,dtype", [(FP, KP, d) for FP, KP in DIAGONAL for d in ("bf16", "fp32")
                                         if "rows_" + d in cell(FP, KP).forms])
def test_rows_reduce_launch_over_64_workgroups(cuda, monkeypatch, FP, KP, dtype):
    """A ring of 66 tiles runs 67 row workgroups, more than kRowsReduceInBwd = 64: the partial
    gradients are summed by reduce_g_kernel and bwd_update reads the sum (gred), three launches
    per slot.  On the 128-row rings above bwd_update sums the partials itself."""
    e, cap = cell(FP, KP), 66 * 32
    monkeypatch.setenv("PSX_SOLVER_ROWS", "1")
    for model in dc.MODELS:
        _, (op, _, _) = _solve(cuda, e, "rows_" + dtype, model, [W0], cap=cap, tag=f"rows_{dtype}-gred")
        assert op._native.kernels_per_solve == 3 + 3 * op.opts.nslots


@pytest.mark.gpu
def test_rows_fp32_refuse_2048(cuda):
    """No fp32 row kernels at FP 2048: the solver refuses at construction, before any launch."""
    e = cell(2048, 4)
    spec = ModelSpec(e.F, e.K)
    ring = DeviceRing(CAP, spec.Fp, cuda, dtype="fp32")
    op = LocalSolveOp(spec, CAP, cuda, dc.options("small"))
    with pytest.raises(ValueError, match="fp32 rows"):
        op.run(ring, 97, 0, dc.start_model(spec, "small").to(cuda))
    assert op._native is None


# ---------------------------------------------------------------------------
# GPU: the lanes round kernel
_LANES = [e for e in TABLE if "lanes" in e.forms]


def _test_rows(spec, ds, cuda):
    return EvalSet(spec, ds.X[CAP:ROWS], ds.y[CAP:ROWS], cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("e,model", **_with_models(_LANES, retry=lambda e: True))
def test_lanes_round_per_cell(cuda, e, model):
    """Three lanes, 64-row rings, 50 rows each (a full and a partial tile), one round: lane
    1's delta against the oracle on its shard rows, the update, the padded features.  The
    retry start's four accepted steps store three curvature pairs in the kernel's LDS."""
    from test_gpu_lanes import _deltas, _loop

    spec, ds, const = dc.window_case(e.F, e.K)
    L, lr = 3, 0.25
    assert _native.hip().lanes_supported(spec.Fp, spec.K, dc.LANES_CAP)
    train, ev = ds.to(cuda), _test_rows(spec, ds, cuda)
    w_start = dc.start_model(spec, model)
    w0 = w_start.to(cuda)
    w = w0.clone()
    lp, keep = _loop(spec, list(range(L)), L, train, ev, w, cuda, rows=50, cap=dc.LANES_CAP, lr=lr,
                     opts=dc.options(model))
    assert lp.run(1, 0, stream_handle(cuda)) == 1
    d = _deltas(lp, L, spec, cuda)
    loss = torch.zeros(1, device=cuda)
    lp.copy_out(1, loss.data_ptr(), 0, stream_handle(cuda))
    torch.cuda.synchronize()
    lp.poll_errors()
    assert torch.allclose(w, w0 + lr * ((d[0] + d[1]) + d[2]), atol=2e-6, rtol=1e-5)
    ref = dc.oracle(e.F, e.K, dc.lane_rows(1, L, 50), model)
    got = d[1].cpu()
    c, b = spec.coef(got), spec.intercept(got)
    err = (c - ref.delta_coef).abs().max().item() / max(ref.delta_coef.abs().max().item(), 1e-6)
    errb = (b - ref.delta_intercept).abs().max().item() / max(ref.delta_intercept.abs().max().item(), 1e-6)
    print(f"FIG form=lanes cell={ident(e)} model={model} win=50 err={err:.3e} errb={errb:.3e} "
          f"dloss={abs(loss.item() - ref.loss):.3e} loss={ref.loss:.6g}")
    assert err <= 2e-2 and errb <= 2e-2, (err, errb)
    assert abs(loss.item() - ref.loss) < 1e-3 * max(1.0, abs(ref.loss)), (loss.item(), ref.loss)
    K, F, Fp = spec.K, spec.F, spec.Fp
    for v in d + [w]:
        assert v[: K * Fp].view(K, Fp)[:, F:].abs().max().item() == 0.0
    assert torch.equal(c[:, const], -spec.coef(w_start)[:, const])


@pytest.mark.gpu
@pytest.mark.parametrize("FP,KP", [(1024, 16), (2048, 2)])
def test_lanes_refuse_unsupported_cells(cuda, FP, KP):
    from test_gpu_lanes import _loop

    e = cell(FP, KP)
    spec, ds, _ = dc.window_case(e.F, e.K)
    assert not _native.hip().lanes_supported(spec.Fp, spec.K, dc.LANES_CAP)
    w = dc.start_model(spec, "small").to(cuda)
    with pytest.raises(ValueError, match="unsupported model"):
        _loop(spec, [0, 1, 2], 3, ds.to(cuda), _test_rows(spec, ds, cuda), w, cuda, rows=50, cap=dc.LANES_CAP)


# ---------------------------------------------------------------------------
# evaluation bodies: exact confusion counts against float64 decisions
EVAL_T = (1, 33, 97)
EVAL_K = (2, 3, 9, 16)
PAIR_K = (2, 3, 8)
RIDE_CELLS = [(256, 4), (512, 8)]
_PAIR = {}


def _pair_case(F, K, T):
    """dense_case + a second model on the same rows, every row safe for it too: the first
    seed (of 16) for which the float64 margins say so."""
    key = (F, K, T)
    if key not in _PAIR:
        case = dense_case(F, K, T)
        spec = case.spec
        X = case.ds.X[:, :F].double()
        for seed in range(16):
            g = torch.Generator().manual_seed(977 * seed + F + K + T)
            wb = spec.pack(torch.randn(K, F, generator=g), torch.randn(K, generator=g))
            z = X @ spec.coef(wb).double().t() + spec.intercept(wb).double()
            delta = torch.full((T,), 2e-5 * max(1.0, float(z.abs().max())), dtype=torch.float64)
            if bool(safe_rows(z, delta, K).all()):
                break
        else:
            raise AssertionError("no second model with every row safe")
        _PAIR[key] = (case, wb, z, delta)
    return _PAIR[key]


def _eval_cases():
    out = [(F_OF[FP], K, T) for FP in F_OF for K in EVAL_K for T in EVAL_T]
    out += [(cell(FP, KP).F, cell(FP, KP).K, T) for FP, KP in RIDE_CELLS for T in EVAL_T]
    return out


def test_eval_rows_are_decided():
    """The condition for exact counts, on the inputs alone and for every row: the float64
    top-two gap exceeds twice the margin bound (both models of the paired cases)."""
    for F, K, T in _eval_cases():
        case = dense_case(F, K, T)
        assert case.ds.rows == T and bool(safe_rows(case.z, case.delta, K).all()), (F, K, T)
    for FP in F_OF:
        for K in PAIR_K:
            for T in EVAL_T:
                case, wb, z, delta = _pair_case(F_OF[FP], K, T)
                assert bool(safe_rows(case.z, case.delta, K).all()) and bool(safe_rows(z, delta, K).all()), (FP, K, T)


def _counts64(z, y, K):
    return decisions64(z, y, K)[3]


def _standalone(cuda, ev, frag, w):
    out = torch.zeros(256, dtype=torch.int32, device=cuda)
    ev.confusion_async(frag, w, out)
    torch.cuda.synchronize()
    return out.cpu().long()


def _slot_counts(addr):
    return torch.tensor((ctypes.c_int32 * 256).from_address(addr)[:], dtype=torch.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("K", EVAL_K)
@pytest.mark.parametrize("FP", list(F_OF))
def test_standalone_eval_counts_exact(cuda, FP, K):
    for T in EVAL_T:
        case = dense_case(F_OF[FP], K, T)
        spec = case.spec
        assert spec.Fp == FP
        ev = EvalSet(spec, case.ds.X, case.ds.y, cuda)
        frag = Fragments(spec, cuda)
        wd = case.w.to(cuda)
        frag.refresh(wd)
        got = _standalone(cuda, ev, frag, wd)
        assert int(got.sum()) == T
        assert torch.equal(got, _counts64(case.z, case.ds.y, K)), (FP, K, T)


@pytest.mark.gpu
@pytest.mark.parametrize("K", PAIR_K)
@pytest.mark.parametrize("FP", list(F_OF))
def test_paired_eval_counts_exact_at_both_offsets(cuda, FP, K):
    """Model a in fragment columns [0, K), model b in [16 - K, 16) of one buffer: one paired
    pass, and single passes at either offset, each equal to the float64 counts."""
    from psx.utils.logsink import _HostSlots

    slots = _HostSlots(4, True)
    sb = _native.host.EVAL_SLOT_BYTES
    a = [slots.ptr + i * sb for i in range(4)]
    try:
        for i, T in enumerate(EVAL_T):
            case, wb, zb, _ = _pair_case(F_OF[FP], K, T)
            spec = case.spec
            ev, sc = EvalSet(spec, case.ds.X, case.ds.y, cuda), EvalScratch(cuda)
            fb = Fragments(spec, cuda, coff=16 - K)
            fa = Fragments(spec, cuda, coff=0, share=fb)
            wa_d, wb_d = case.w.to(cuda), wb.to(cuda)
            fa.refresh(wa_d)
            fb.refresh(wb_d)
            seq = 10 * i
            ev.eval_pair_to_slots(fa, wa_d, fb, wb_d, sc, a[0], seq + 1, None, a[1], seq + 2)
            fa1, fb1 = Fragments(spec, cuda, coff=0), Fragments(spec, cuda, coff=16 - K)  # buffers of their own
            fa1.refresh(wa_d)
            fb1.refresh(wb_d)
            ev.eval_to_slot(fa1, wa_d, sc, a[2], seq + 3, None)
            ev.eval_to_slot(fb1, wb_d, sc, a[3], seq + 4, None)
            torch.cuda.synchronize()
            got = [_slot_counts(p) for p in a]
            want_a, want_b = _counts64(case.z, case.ds.y, K), _counts64(zb, case.ds.y, K)
            assert torch.equal(got[0], want_a) and torch.equal(got[2], want_a), (FP, K, T)
            assert torch.equal(got[1], want_b) and torch.equal(got[3], want_b), (FP, K, T)
            assert sc.acc.abs().sum().item() == 0
            fb.coff = 17 - K  # one column past the buffer: refused before any launch
            with pytest.raises(ValueError, match="offset out of range"):
                ev.eval_to_slot(fb, wb_d, sc, a[3], seq + 5, None)
    finally:
        slots.free()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["chain", "persist"])
@pytest.mark.parametrize("FP,KP", RIDE_CELLS)
def test_riding_eval_counts_equal_standalone(cuda, FP, KP, form):
    """An evaluation pass riding in the solve's launches (spare workgroups of bwd_update /
    of the persistent launch) counts what the standalone kernel counts, and the solve it
    rides in still matches the oracle."""
    from psx.utils.logsink import _HostSlots

    e = cell(FP, KP)
    spec, ds, const = dc.window_case(e.F, e.K)
    ring = _ring(cuda, ds, CAP)
    w = dc.start_model(spec, "small")
    wd = w.to(cuda)
    slots = _HostSlots(1, True)
    try:
        for i, T in enumerate(EVAL_T):
            case = dense_case(e.F, e.K, T)
            ev, sc = EvalSet(spec, case.ds.X, case.ds.y, cuda), EvalScratch(cuda)
            frag = Fragments(spec, cuda)
            wm = case.w.to(cuda)
            frag.refresh(wm)
            alone = _standalone(cuda, ev, frag, wm)
            assert torch.equal(alone, _counts64(case.z, case.ds.y, e.K))
            op = LocalSolveOp(spec, CAP, cuda, dc.options("small", **_FORM_OPTS[form]))
            assert op.can_ride(ring, wd)
            op.run(ring, W0[0], W0[1], wd, ride=ev.ride_args(frag, None, sc, slots.ptr, i + 1, op.loss, 0, 0))
            torch.cuda.synchronize()
            _assert_form(op, form)
            assert torch.equal(_slot_counts(slots.ptr), alone), (form, T)
            assert sc.acc.abs().sum().item() == 0
            _check(f"form={form}+ride cell={ident(e)} model=small win=97@0", spec, const, op, w,
                   dc.oracle(e.F, e.K, dc.window_rows(W0), "small"), W0[0])
    finally:
        slots.free()

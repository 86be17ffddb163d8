"""The scoring kernels (csrc/kernels/score_kernels.hip) on an MI355X, through
psx.ops.score.Scorer, against the float64 oracle of _score_cases.py: every FP / KP
template, partial and multiple tiles, the grid caps, large margins, zero weights,
label edge cases, agreement with the training-time evaluation kernels,
determinism and chunking, and a checkpoint of a real run."""
import functools
import math

import pytest
import torch

from _score_cases import dense_case, wide_case, with_bad_labels
from psx import _native
from psx.ops.lr import EvalSet, Fragments, stream_handle
from psx.ops.score import Scorer
from psx.runtime.config import PSConfig
from psx.runtime.engine import LocalEngine
from psx.utils.checkpoint import load_server
from psx.utils.data import synth_finefood

pytestmark = pytest.mark.gpu

# (F, K): FP 128 / 128 / 256 / 512 / 512 / 1024 / 2048, padded feature columns at 99 / 200 / 300 / 2000
DENSE_FK = [(99, 2), (128, 16), (200, 3), (300, 6), (512, 6), (1024, 6), (2000, 11)]
DENSE_T = [1, 31, 32, 33, 97]  # a partial tile, an exact tile, one row over, three tiles and a bit
WIDE_K = [1, 2, 3, 6, 11, 16]  # every KP, and the sigmoid model
WIDE_T = [1, 3, 4, 5]  # 4 rows per workgroup


@functools.lru_cache(maxsize=None)
def _dense(F, K, T, scale=1.0, zero_w=False):
    return dense_case(F, K, T, scale=scale, zero_w=zero_w)


@functools.lru_cache(maxsize=None)
def _wide(K, T, zero_w=False):
    return wide_case(K, T, zero_w=zero_w)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, confusion=True):
    for name in ("pred", "proba", "nll"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert torch.equal(_bits(x), _bits(y)), name
    if confusion:
        assert torch.equal(a.confusion, b.confusion) and a.rows_out_of_range == b.rows_out_of_range
        assert a.log_loss == b.log_loss


# ---- 1 / 2: geometry -----------------------------------------------------------------
@pytest.mark.parametrize("T", DENSE_T)
@pytest.mark.parametrize("F,K", DENSE_FK)
def test_dense_geometry(cuda, F, K, T):
    case = _dense(F, K, T)
    case.check(Scorer(case.spec, case.w, cuda).score(case.ds, proba=True), f"dense F{F} K{K} T{T}")


def test_dense_past_the_grid_cap(cuda):
    """32 * 1024 + 5 rows: workgroups loop past the 1,024-workgroup grid (8 MB of rows)."""
    case = _dense(128, 6, 32 * 1024 + 5)
    case.check(Scorer(case.spec, case.w, cuda).score(case.ds, proba=True), "dense grid cap")


@pytest.mark.parametrize("T", WIDE_T)
@pytest.mark.parametrize("K", WIDE_K)
def test_wide_geometry(cuda, K, T):
    case = _wide(K, T)
    case.check(Scorer(case.spec, case.w, cuda).score(case.ds, proba=True), f"wide K{K} T{T}")


def test_wide_past_the_grid_cap(cuda):
    """4 * 1024 + 3 rows (every row length, 700 included): workgroups loop past the grid."""
    case = _wide(6, 4 * 1024 + 3)
    lens = (case.ds.indptr[1:] - case.ds.indptr[:-1]).tolist()
    assert {0, 1, 63, 64, 65, 700} <= set(lens)
    case.check(Scorer(case.spec, case.w, cuda).score(case.ds, proba=True), "wide grid cap")


# ---- 3: numerical range ----------------------------------------------------------------
def test_dense_large_margins(cuda):
    """w ~ 40 N(0,1) at F = 1024: margins in the hundreds; everything finite, rows sum to 1."""
    case = _dense(1024, 6, 97, 40.0)
    assert case.zmax > 100, case.zmax
    res = Scorer(case.spec, case.w, cuda).score(case.ds, proba=True)
    assert bool(torch.isfinite(res.proba).all()) and bool(torch.isfinite(res.nll).all())
    assert math.isfinite(res.log_loss)
    case.check(res, f"dense margins to {case.zmax:.0f}")


@pytest.mark.parametrize("kind", ["dense", "wide", "sigmoid"])
def test_zero_weights(cuda, kind):
    case = _dense(300, 6, 33, 1.0, True) if kind == "dense" else _wide(6 if kind == "wide" else 1, 17, True)
    res = Scorer(case.spec, case.w, cuda).score(case.ds, proba=True)
    C = case.spec.eval_classes
    assert int(res.pred.abs().sum()) == 0  # the lowest class wins the tie; binary: z > 0 is false
    dp = float((res.proba - 1.0 / C).abs().max())
    dn = float((res.nll - math.log(C)).abs().max())
    print(f"[w=0 {kind}] max |p - 1/C| {dp:.3e} max |nll - log C| {dn:.3e}")
    assert dp <= 1e-6
    case.check(res, f"w=0 {kind}")


# ---- 4: labels ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "wide", "sigmoid"])
def test_labels(cuda, kind):
    base = _dense(300, 6, 97) if kind == "dense" else _wide(6 if kind == "wide" else 1, 17)
    case = with_bad_labels(base)  # -1, K and 99 among the valid labels
    sc = Scorer(case.spec, case.w, cuda)
    res = sc.score(case.ds, proba=True)
    case.check(res, f"labels {kind}")  # NaN exactly there, log_loss over the valid rows, the clamped confusion
    nbad = 0 if kind == "sigmoid" else 3
    assert res.rows_out_of_range == nbad and int(torch.isnan(res.nll).sum()) == nbad
    none = sc.score(case.ds, labels=False, proba=True)
    case.check(none, f"no labels {kind}", labels=False)
    assert none.nll is None
    assert torch.equal(none.pred, res.pred) and torch.equal(_bits(none.proba), _bits(res.proba))
    assert torch.equal(sc.predict(case.ds), res.pred)
    assert torch.equal(_bits(sc.predict_proba(case.ds)), _bits(res.proba))
    assert sc.score(case.ds, labels=False).proba is None


# ---- 5: agreement with the training-time evaluation -------------------------------------------
@pytest.mark.parametrize("F,K", [(300, 6), (2000, 11)])
def test_dense_confusion_equals_evalset(cuda, F, K):
    case = _dense(F, K, 97)
    res = Scorer(case.spec, case.w, cuda).score(case.ds)
    wd = case.w.to(cuda)
    frag = Fragments(case.spec, cuda)
    frag.refresh(wd)
    out = torch.zeros(256, dtype=torch.int32, device=cuda)
    EvalSet(case.spec, case.ds.X, case.ds.y, cuda).confusion_async(frag, wd, out)
    assert torch.equal(res.confusion, out.cpu().view(16, 16)[:K, :K].long())


@pytest.mark.parametrize("K", [1, 6])
def test_wide_confusion_equals_wide_eval(cuda, K):
    case = _wide(K, 4 * 1024 + 3) if K == 6 else _wide(K, 17)
    spec, ds = case.spec, case.ds.to(cuda)
    res = Scorer(spec, case.w, cuda).score(case.ds)
    wd = case.w.to(cuda)
    acc = torch.zeros(512, dtype=torch.int32, device=cuda)
    _native.hip().wide_eval(spec.K, spec.KP, spec.F, ds.indptr.data_ptr(), ds.idx.data_ptr(), ds.val.data_ptr(),
                            ds.y.data_ptr(), ds.rows, wd.data_ptr(), 0, 0, 0, acc.data_ptr(),
                            stream=stream_handle(cuda))
    C = spec.eval_classes
    assert torch.equal(res.confusion, acc[:256].cpu().view(16, 16)[:C, :C].long())


# ---- 6: determinism and chunking ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "wide"])
def test_deterministic_and_chunk_invariant(cuda, kind):
    case = _dense(300, 6, 97) if kind == "dense" else _wide(6, 4 * 1024 + 3)
    if kind == "wide":  # 100 rows of it are enough here
        from _score_cases import Case

        case = Case(case.spec, case.ds.slice(0, 100), case.w, case.z[:100], case.delta[:100])
    sc = Scorer(case.spec, case.w, cuda)
    ref = sc.score(case.ds, proba=True)
    _same(sc.score(case.ds, proba=True), ref)
    for chunk in (1, 33, case.ds.rows):  # a row's result must not depend on its tile or launch
        _same(sc.score(case.ds, proba=True, chunk_rows=chunk), ref)
    on_device = sc.score(case.ds.to(cuda), proba=True)  # rows already on the device
    _same(on_device, ref)


# ---- 7: end to end ----------------------------------------------------------------------------------
def test_checkpoint_and_engine_end_to_end(cuda, tmp_path):
    train, test = synth_finefood(6000, seed=0), synth_finefood(500, seed=1)
    cfg = PSConfig(num_workers=2, consistency_model=0, producer_time_per_event=0, stream_mode="per_iter",
                   rows_per_iter=128, epochs=1000, max_iters=3, init="random", min_buffer_size=256,
                   max_buffer_size=256, checkpoint_dir=str(tmp_path), checkpoint_every=3)
    eng = LocalEngine(cfg, cuda, train=train, test=test)
    eng.run()
    torch.cuda.synchronize()
    assert load_server(str(tmp_path))["extra"]["step"] == 3
    ck = Scorer.from_checkpoint(str(tmp_path), cuda)
    live = Scorer.from_engine(eng)
    assert ck.spec == live.spec == eng.spec and torch.equal(ck.w, live.w)
    a, b = ck.score(test, proba=True), live.score(test, proba=True)
    _same(a, b)
    assert a.rows == 500 and a.rows_out_of_range == 0 and 0.0 < a.log_loss < 10.0
    frag = Fragments(eng.spec, cuda)
    frag.refresh(ck.w)
    out = torch.zeros(256, dtype=torch.int32, device=cuda)
    EvalSet(eng.spec, test.X, test.y, cuda).confusion_async(frag, ck.w, out)
    K = eng.spec.K
    assert torch.equal(a.confusion, out.cpu().view(16, 16)[:K, :K].long())
    assert _native.hip_loaded_path() is not None

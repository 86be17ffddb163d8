"""The score histogram of the scoring kernels (csrc/kernels/score_kernels.hip, ``curves=True``) on an
MI355X against the float64 oracle of _hist_cases.py: every table must lie between the oracle's
``lo`` and ``hi`` cell by cell with exact side totals, and repeat bit for bit.  Shapes: the smallest
at which each path can go wrong -- partial and multiple tiles, the largest LDS table beside an
FP 1024 and an FP 2048 tile, the global-atomics form beyond it, both end bins, several tiles per
workgroup, one hot bin per class, labels out of range; every KP of the wide kernel, its second
pass, large margins.  The other outputs of a ``curves=True`` call equal a plain call's bit for bit."""
import numpy as np
import pytest
import torch

import _hist_cases as H
from _hist_cases import hist_oracle, with_bad_labels
from psx import _native
from psx.ops.score import Scorer

pytestmark = pytest.mark.gpu


def _ids(v):
    return "-".join(str(x) for x in v)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check(case, cuda, tag, **kw):
    sc = Scorer(case.spec, case.w, cuda)
    res = sc.score(case.ds, curves=True, **kw)
    hist_oracle(case).check(res.hist, tag)
    again = sc.score(case.ds, curves=True, **kw)
    assert torch.equal(again.hist, res.hist), "the table differs between two runs"
    return sc, res


# ---- dense ----------------------------------------------------------------------------
@pytest.mark.parametrize("fkts", H.DENSE_GPU, ids=_ids)
def test_dense_table(cuda, fkts):
    F, K, T, scale = fkts
    case = H.dense(F, K, T, scale)
    _, res = _check(case, cuda, f"dense {fkts}")
    form = _native.hip().score_hist_form(case.spec.Fp, K)
    assert form == (2 if (F, K) == (2000, 16) else 1)  # only FP 2048 with more than 5 classes leaves the LDS table
    if scale == 20.0:
        assert int(res.hist[:, :, 0].sum()) > 0 and int(res.hist[:, :, H.NB - 1].sum()) > 0  # both end bins


@pytest.mark.parametrize("fkt", H.DENSE_ZERO, ids=_ids)
def test_dense_zero_weights_one_hot_bin_per_class(cuda, fkt):
    F, K, T = fkt
    case = H.dense(F, K, T, 1.0, True)
    _, res = _check(case, cuda, f"dense w=0 {fkt}")
    o = hist_oracle(case)
    assert torch.equal(o.lo, o.hi) and torch.equal(res.hist, o.lo)  # exact
    b = 256 + round(-16 * np.log(K - 1))
    assert int(res.hist[:, :, b].sum()) == T * K


def test_dense_bad_labels(cuda):
    case = with_bad_labels(H.dense(300, 5, 33))
    _, res = _check(case, cuda, "dense bad labels")
    assert int(res.hist.sum()) == (33 - 3) * 5 and res.rows_out_of_range == 3


@pytest.mark.parametrize("fkts", [(300, 5, 33, False), (1024, 16, 229, False), (2000, 5, 229, False),
                                  (128, 6, 40000, False), (100, 6, 64, True)], ids=_ids)
def test_dense_forms_give_the_same_table(cuda, monkeypatch, fkts):
    F, K, T, zero_w = fkts  # zero weights: every row of a class in one bin, the contended case of both forms
    case = H.dense(F, K, T, 1.0, zero_w)
    sc = Scorer(case.spec, case.w, cuda)
    tables = {}
    for form in ("lds", "global", "auto"):
        monkeypatch.setenv("PSX_SCORE_HIST_FORM", form)
        tables[form] = sc.score(case.ds, curves=True).hist
        hist_oracle(case).check(tables[form], f"dense {fkts} form {form}")
    assert torch.equal(tables["lds"], tables["global"]) and torch.equal(tables["lds"], tables["auto"])


def test_dense_lds_form_refused_where_it_does_not_fit(cuda, monkeypatch):
    case = H.dense(2000, 16, 229)
    sc = Scorer(case.spec, case.w, cuda)
    monkeypatch.setenv("PSX_SCORE_HIST_FORM", "lds")
    with pytest.raises(ValueError, match="does not fit"):
        sc.score(case.ds, curves=True)
    monkeypatch.setenv("PSX_SCORE_HIST_FORM", "global")
    hist_oracle(case).check(sc.score(case.ds, curves=True).hist, "dense 2000 x 16 global")
    monkeypatch.setenv("PSX_SCORE_HIST_FORM", "no-such-form")
    with pytest.raises(ValueError, match="PSX_SCORE_HIST_FORM"):
        sc.score(case.ds, curves=True)


@pytest.mark.parametrize("fkts", [(1024, 6, 229, 1.0), (2000, 16, 229, 1.0)], ids=_ids)
def test_dense_chunks_add_up(cuda, fkts):
    F, K, T, scale = fkts
    case = H.dense(F, K, T, scale)
    sc, ref = _check(case, cuda, f"dense {fkts}")
    for chunk in (32, 100, T):
        got = sc.score(case.ds, curves=True, chunk_rows=chunk)
        assert torch.equal(got.hist, ref.hist), chunk
    assert torch.equal(sc.score(case.ds.to(cuda), curves=True).hist, ref.hist)  # rows already on the device


# ---- wide -----------------------------------------------------------------------------
@pytest.mark.parametrize("kts", H.WIDE_GPU, ids=_ids)
def test_wide_table(cuda, kts):
    K, T, scale = kts
    case = H.wide(K, T, scale)
    lens = (case.ds.indptr[1:] - case.ds.indptr[:-1]).tolist()
    assert {0, 1, 63, 64, 65, 700} <= set(lens)
    _check(case, cuda, f"wide {kts}")


@pytest.mark.parametrize("kt", H.WIDE_ZERO, ids=_ids)
def test_wide_zero_weights(cuda, kt):
    K, T = kt
    case = H.wide(K, T, 1.0, True)
    _, res = _check(case, cuda, f"wide w=0 {kt}")
    o = hist_oracle(case)
    assert torch.equal(o.lo, o.hi) and torch.equal(res.hist, o.lo)
    b = 256 if K == 1 else 256 + round(-16 * np.log(K - 1))
    assert int(res.hist[:, :, b].sum()) == T * K


@pytest.mark.parametrize("K", [1, 6])
def test_wide_bad_labels(cuda, K):
    case = with_bad_labels(H.wide(K, 400))
    _, res = _check(case, cuda, f"wide bad labels K{K}")
    if K == 1:  # the binary model takes any label: y > 0
        assert int(res.hist.sum()) == 400 and res.rows_out_of_range == 0
    else:
        assert int(res.hist.sum()) == 397 * K and res.rows_out_of_range == 3


def test_wide_chunks_add_up(cuda):
    case = H.wide(6, 400)
    sc, ref = _check(case, cuda, "wide chunks")
    for chunk in (32, 100, 400):
        assert torch.equal(sc.score(case.ds, curves=True, chunk_rows=chunk).hist, ref.hist), chunk


# ---- the other outputs ------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda: H.dense(1024, 6, 229), lambda: H.dense(2000, 16, 229),
                                  lambda: with_bad_labels(H.dense(300, 5, 33)), lambda: H.wide(6, 400),
                                  lambda: H.wide(1, 400), lambda: H.wide(16, 400)],
                         ids=["dense-lds", "dense-global", "dense-bad-labels", "wide", "sigmoid", "wide-16"])
@pytest.mark.parametrize("proba", [False, True], ids=["", "proba"])
def test_curves_leave_the_other_outputs_alone(cuda, make, proba):
    case = make()
    sc = Scorer(case.spec, case.w, cuda)
    plain, curves = sc.score(case.ds, proba=proba), sc.score(case.ds, proba=proba, curves=True)
    assert plain.hist is None and plain.auc is None and plain.ece is None
    for f in ("pred", "nll", "confusion") + (("proba",) if proba else ()):
        assert torch.equal(_bits(getattr(plain, f)), _bits(getattr(curves, f))), f
    assert (plain.log_loss, plain.f1, plain.accuracy, plain.rows_out_of_range) == \
        (curves.log_loss, curves.f1, curves.accuracy, curves.rows_out_of_range)
    case.check(curves, "curves=True", proba=proba)  # and both meet the scoring oracle


def test_gpu_and_cpu_tables_share_their_bounds(cuda):
    for case in (H.dense(1024, 6, 229), H.wide(6, 400)):
        o = hist_oracle(case)
        g = Scorer(case.spec, case.w, cuda).score(case.ds, curves=True)
        c = Scorer(case.spec, case.w, "cpu").score(case.ds, curves=True)
        o.check(g.hist, "gpu")
        o.check(c.hist, "cpu")
        moved = int((g.hist != c.hist).sum())
        print(f"cells that differ between the GPU and the CPU table: {moved}")  # allowed: not asserted


def test_planted_auc_within_its_bound(cuda):
    case = H.planted()
    res = Scorer(case.spec, case.w, cuda).score(case.ds, curves=True)
    hist_oracle(case).check(res.hist, "gpu planted")
    H.check_planted_auc(res, case, "gpu planted")
    assert res.auc_macro > 0.6 and res.auc_weighted > 0.6 and 0.0 <= res.ece < 0.1
    assert _native.hip_loaded_path() is not None

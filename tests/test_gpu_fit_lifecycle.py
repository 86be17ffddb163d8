"""The lifecycle of the full-batch fitters on MI355X (csrc/solver/fit_driver.hip, shared
by the dense and the wide fitter): what ends a fit in progress, which calls need a
dataset or a begun fit, and that no state of one fit or evaluation reaches the next.
Smallest shapes with a partial last tile / wave and three workgroups (``max_wg=3``)."""
import pytest
import torch

from _fit_cases import fit_case
from _wide_fit_cases import sparse_case
from psx.ops.fit import BatchFitter, FitOptions
from psx.ops.lr import stream_handle
from psx.ops.wide_fit import WideFitter

pytestmark = pytest.mark.gpu

KINDS = ["dense", "wide", "wide-one-logit"]
_CASES = {}


def case(kind, seed):
    """(spec, dataset), built once: dense 67 x 100 (FP 128) K 3, wide 67 rows over 300 features K 3 / K 1."""
    if (kind, seed) not in _CASES:
        if kind == "dense":
            _CASES[kind, seed] = fit_case(67, 100, 3, seed=seed)[:2]
        else:
            _CASES[kind, seed] = sparse_case(67, 300, 3 if kind == "wide" else 1, seed=seed)
    return _CASES[kind, seed]


def fitter(kind, spec, dev):
    opts = FitOptions(max_iter=6, reg_param=0.01, max_wg=3)
    return (BatchFitter if kind == "dense" else WideFitter)(spec, dev, opts)


def begin(f, max_iter=6):
    f._native.begin(0, max_iter, 1e-6, 0.01, 20, True, stream_handle(f.device))


def run(f, steps=1):
    return f._native.run(steps, stream_handle(f.device))


@pytest.mark.parametrize("kind", KINDS)
def test_run_needs_a_begun_fit_and_begin_a_dataset(cuda, kind):
    spec, ds = case(kind, 0)
    f = fitter(kind, spec, cuda)
    with torch.cuda.device(cuda):
        with pytest.raises(RuntimeError):
            run(f)
        with pytest.raises(RuntimeError):
            begin(f)
        f._load(ds)
        assert f._native.done
        with pytest.raises(RuntimeError):
            run(f)
        begin(f)
        assert not f._native.done
        assert run(f) is False and f._native.accepted == 1 and not f._native.done


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ender", ["loss_grad", "load"])
def test_an_evaluation_or_a_new_dataset_ends_the_fit(cuda, kind, ender):
    spec, ds = case(kind, 0)
    f = fitter(kind, spec, cuda)
    with torch.cuda.device(cuda):
        f._load(ds)
        begin(f)
        assert run(f) is False
        if ender == "loss_grad":
            f.loss_grad(ds, torch.zeros(spec.P, device=cuda))
        else:
            f._load(case(kind, 1)[1])
        assert f._native.done
        with pytest.raises(RuntimeError):
            run(f)
        begin(f)  # and a new fit starts from scratch
        assert not f._native.done and f._native.accepted == 0 and f._native.evals == 0
        assert list(f._native.history) == [] and list(f._native.eval_seconds) == []
        assert run(f) is False and f._native.accepted == 1


@pytest.mark.parametrize("kind", KINDS)
def test_fits_in_a_row_equal_fits_on_fresh_fitters(cuda, kind):
    (spec, a), (_, b) = case(kind, 0), case(kind, 1)
    f = fitter(kind, spec, cuda)
    for ds in (a, b):
        got, want = f.fit(ds), fitter(kind, spec, cuda).fit(ds)
        assert torch.equal(got.w, want.w)
        assert got.history == want.history and len(got.history) == got.iters + 1
        assert (got.iters, got.evals, got.reason) == (want.iters, want.evals, want.reason)
        assert got.iters >= 1 and len(f._native.eval_seconds) == got.evals


@pytest.mark.parametrize("kind", KINDS)
def test_loss_grad_twice_is_bit_equal_and_reuses_the_resident_copy(cuda, kind):
    spec, ds = case(kind, 0)
    f = fitter(kind, spec, cuda)
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(spec.P, generator=g) * 0.05).to(cuda)
    l0, g0 = f.loss_grad(ds, w)
    data = f._data
    assert data is not None and data.src is ds
    l1, g1 = f.loss_grad(ds, w)
    assert f._data is data
    assert l0 == l1 and torch.equal(g0, g1)
    assert list(f._native.eval_seconds) == []  # a single evaluation is not a fit's

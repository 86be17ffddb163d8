"""The entry points bound with a raw padded width / class count refuse a value
their kernels are not built for (csrc/kernels/dispatch.h): a ValueError on the
host, before any launch, and the output buffer stays as it was.  At a supported
value the same call still launches.  Tiny inputs: 32 dense rows, 4 sparse rows,
2 classes."""
import pytest
import torch

from psx import _native
from psx.models.logreg import ModelSpec
from psx.models.reference import predict
from psx.ops.lr import Fragments, stream_handle

pytestmark = pytest.mark.gpu

T, F, K = 32, 100, 2
SENTINEL = -7


class _Dense:
    """32 bf16 rows of a 100-feature, 2-class model (padded width 128) and its fragments."""

    def __init__(self, cuda):
        self.spec = spec = ModelSpec(F, K)
        assert spec.Fp == 128
        g = torch.Generator().manual_seed(17)
        X = torch.zeros(T, spec.Fp)
        X[:, :F] = torch.randn(T, F, generator=g) * 0.05
        self.Xb = X.to(torch.bfloat16)
        self.w = spec.pack(torch.randn(K, F, generator=g) * 0.1, torch.randn(K, generator=g) * 0.1)
        self.X = self.Xb.to(cuda)
        self.y = (torch.arange(T) % K).to(torch.int32).to(cuda)
        self.frag = Fragments(spec, cuda)
        self.frag.refresh(self.w.to(cuda))
        self.s = stream_handle(cuda)

    def logits(self, FP, out):
        f = self.frag
        _native.hip().logits(FP, K, self.X.data_ptr(), T, f.hi.data_ptr(), f.lo.data_ptr(), f.b.data_ptr(),
                             out.data_ptr(), self.s)

    def test_eval(self, FP, conf):
        f = self.frag
        _native.hip().test_eval(FP, K, self.X.data_ptr(), self.y.data_ptr(), T, f.hi.data_ptr(), f.lo.data_ptr(),
                                f.b.data_ptr(), conf.data_ptr(), self.s)

    def score(self, FP, pred):
        f = self.frag
        _native.hip().score(FP, K, self.X.data_ptr(), 0, T, f.hi.data_ptr(), f.lo.data_ptr(), f.b.data_ptr(),
                            pred.data_ptr(), stream=self.s)


class _Wide:
    """4 CSR rows over 16 features; the model is sized for the widest class count tried."""

    F, ROWS, KPMAX = 16, 4, 32

    def __init__(self, cuda):
        g = torch.Generator().manual_seed(23)
        self.indptr = torch.tensor([0, 3, 4, 9, 12], dtype=torch.int64, device=cuda)
        self.idx = torch.tensor([0, 5, 9, 15, 1, 2, 3, 8, 13, 4, 5, 6], dtype=torch.int32, device=cuda)
        self.valb = (torch.randn(12, generator=g) * 0.5).to(torch.bfloat16)
        self.val = self.valb.to(cuda)
        self.y = torch.tensor([0, 1, 1, 0], dtype=torch.int32, device=cuda)
        self.wc = torch.randn(self.F * self.KPMAX + self.KPMAX, generator=g) * 0.1
        self.w = self.wc.to(cuda)
        self.s = stream_handle(cuda)

    def _csr(self):
        return self.indptr.data_ptr(), self.idx.data_ptr(), self.val.data_ptr()

    def logits(self, KP, out):
        _native.hip().wide_logits(min(K, KP), KP, self.F, *self._csr(), self.ROWS, self.w.data_ptr(), out.data_ptr(),
                                  self.s)

    def eval(self, KP, acc):
        _native.hip().wide_eval(min(K, KP), KP, self.F, *self._csr(), self.y.data_ptr(), self.ROWS, self.w.data_ptr(),
                                0, 0, 0, acc.data_ptr(), stream=self.s)

    def score(self, KP, pred):
        _native.hip().wide_score(min(K, KP), KP, self.F, *self._csr(), 0, self.ROWS, self.w.data_ptr(),
                                 pred.data_ptr(), stream=self.s)


def _filled(n, dtype, cuda):
    return torch.full((n,), SENTINEL, dtype=dtype, device=cuda)


def _untouched(buf):
    torch.cuda.synchronize()
    return bool((buf == SENTINEL).all())


def _once(make):  # (module scope is set up before the function-scoped `cuda` could skip)
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return make("cuda:0")


@pytest.fixture(scope="module")
def dense():
    return _once(_Dense)


@pytest.fixture(scope="module")
def wide():
    return _once(_Wide)


@pytest.mark.parametrize("FP", [192, 4096])
def test_dense_entry_points_refuse_unlisted_widths(cuda, dense, FP):
    out = _filled(T * K, torch.float32, cuda)
    with pytest.raises(ValueError, match=str(FP)):
        dense.logits(FP, out)
    assert _untouched(out)
    conf = _filled(256, torch.int32, cuda)
    with pytest.raises(ValueError, match=str(FP)):
        dense.test_eval(FP, conf)
    assert _untouched(conf)


def test_score_refuses_unlisted_width(cuda, dense):
    pred = _filled(T, torch.int32, cuda)
    with pytest.raises(ValueError):
        dense.score(192, pred)
    assert _untouched(pred)


@pytest.mark.parametrize("KP", [3, 32])
def test_wide_entry_points_refuse_unlisted_class_counts(cuda, wide, KP):
    out = _filled(wide.ROWS * KP, torch.float32, cuda)
    with pytest.raises(ValueError, match=str(KP)):
        wide.logits(KP, out)
    assert _untouched(out)
    acc = _filled(512, torch.int32, cuda)
    with pytest.raises(ValueError, match=str(KP)):
        wide.eval(KP, acc)
    assert _untouched(acc)
    pred = _filled(wide.ROWS, torch.int32, cuda)
    with pytest.raises(ValueError):
        wide.score(KP, pred)
    assert _untouched(pred)


def test_supported_dense_values_still_launch(cuda, dense):
    spec, w = dense.spec, dense.w
    out = _filled(T * K, torch.float32, cuda)
    dense.logits(128, out)
    torch.cuda.synchronize()
    # float64 on the bf16 rows, the bound of test_gpu_kernels.test_logits_match_fp32
    ref = dense.Xb[:, :F].double() @ spec.coef(w).double().t() + spec.intercept(w).double()
    z = out.view(T, K).cpu().double()
    err = (z - ref).abs().max().item()
    tol = 2e-5 * max(1.0, ref.abs().max().item())
    assert err < tol, err
    # the reference's decision, where its margin decides beyond that bound
    decided = (ref[:, 0] - ref[:, 1]).abs() > 2 * tol
    want = predict(dense.Xb[:, :F], spec.coef(w), spec.intercept(w))
    assert bool((z.argmax(1)[decided] == want[decided]).all())

    conf = _filled(256, torch.int32, cuda)
    dense.test_eval(128, conf)
    torch.cuda.synchronize()
    assert int((conf - SENTINEL).sum()) == T  # one count per row, added to what was there

    pred = _filled(T, torch.int32, cuda)
    dense.score(128, pred)
    torch.cuda.synchronize()
    assert bool((pred.cpu()[decided] == want[decided].to(torch.int32)).all()) and not bool((pred == SENTINEL).any())


def test_supported_wide_values_still_launch(cuda, wide):
    KP, Fw, R = 2, wide.F, wide.ROWS
    out = _filled(R * KP, torch.float32, cuda)
    wide.logits(KP, out)
    torch.cuda.synchronize()
    coef, b = wide.wc[: Fw * KP].view(Fw, KP).double(), wide.wc[Fw * KP: Fw * KP + KP].double()
    ip, idx, val = wide.indptr.cpu(), wide.idx.cpu().long(), wide.valb.double()
    ref = torch.stack([(val[ip[r]:ip[r + 1], None] * coef[idx[ip[r]:ip[r + 1]]]).sum(0) + b for r in range(R)])
    # <= 5 products of magnitude < 1 summed in fp32: far inside the dense bound
    assert (out.view(R, KP).cpu().double() - ref).abs().max().item() < 2e-5

    acc = _filled(512, torch.int32, cuda)
    wide.eval(KP, acc)
    torch.cuda.synchronize()
    assert int((acc - SENTINEL).sum()) == R

    pred = _filled(R, torch.int32, cuda)
    wide.score(KP, pred)
    torch.cuda.synchronize()
    decided = (ref[:, 0] - ref[:, 1]).abs() > 4e-5
    assert bool((pred.cpu().long()[decided] == ref.argmax(1)[decided]).all()) and not bool((pred == SENTINEL).any())

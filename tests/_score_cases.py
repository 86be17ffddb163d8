"""Inputs, float64 oracle and bounds shared by the scoring tests (test_score_cpu.py,
test_gpu_score.py).

Oracle: float64 margins of the bf16 values as stored, then float64 softmax /
logsumexp.  Margin bound ``delta`` per row:
  * dense: 2e-5 max(1, max|z|), the bound test_logits_match_fp32 holds the same
    forward path to;
  * wide: (nnz + 8) 2^-24 (sum |v w| + |b|), the fp32 recursive-sum bound of
    _margins64 in test_gpu_wide_geometry.py (copied here), the row's largest class.
Probabilities: |dp| <= delta + 1e-6 (the softmax Jacobian's row sums are
2p(1-p) <= 1/2; 1e-6 covers the fp32 exponential and divide on values <= 1).
Per-row loss: |dnll| <= 2 delta + 1e-6 max(1, max|z|).  log_loss: the mean of the
rows' bounds (a mean of entries each within its bound).  Predictions and confusion
are compared exactly on every row: a row is *safe* when its float64 top-two gap
(|z| for the binary model) exceeds 2 delta, and the builders redraw unsafe rows from
the same seeded generator (at most 8 passes) and assert that every row is safe.
"""
import torch

from psx.models.logreg import ModelSpec
from psx.models.wide import WideSpec
from psx.ops.sparse import SparseDataset
from psx.utils.data import Dataset
from psx.utils.metrics import metrics_from_confusion

U24 = 2.0 ** -24
MAX_REDRAWS = 8


# ---- oracle ------------------------------------------------------------------
def oracle(z, y, K):
    """float64 (pred, proba [T, C], nll with NaN markers, confusion [256], rows out of range)."""
    y = y.long()
    if K == 1:
        z0 = z[:, 0]
        pred = (z0 > 0).long()
        proba = torch.stack([torch.sigmoid(-z0), torch.sigmoid(z0)], 1)
        yb = (y > 0)
        nll = torch.logaddexp(torch.zeros_like(z0), z0) - yb.double() * z0
        ok = torch.ones_like(yb)
        cl = yb.long()
    else:
        pred = z.argmax(1)
        proba = torch.softmax(z, 1)
        ok = (y >= 0) & (y < K)
        v = torch.logsumexp(z, 1) - z.gather(1, y.clamp(0, K - 1).view(-1, 1)).view(-1)
        nll = torch.where(ok, v, torch.full_like(v, float("nan")))
        cl = y.clamp(0, 15)
    conf = torch.zeros(256, dtype=torch.int64)
    conf.index_add_(0, cl * 16 + pred, torch.ones_like(pred))
    return pred, proba, nll, conf, int((~ok).sum())


def safe_rows(z, delta, K):
    if K == 1:
        return z[:, 0].abs() > 2 * delta
    top = z.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) > 2 * delta


class Case:
    """ds + weights + the oracle's margins z [T, K] (float64) and the per-row bound delta [T]."""

    def __init__(self, spec, ds, w, z, delta):
        self.spec, self.ds, self.w, self.z, self.delta = spec, ds, w, z, delta
        self.zmax = max(1.0, float(z.abs().max())) if z.numel() else 1.0

    def check(self, res, tag="", labels=True, proba=True):
        """Compare a ScoreResult with the oracle under the module's bounds; prints each figure first."""
        K, C, T = self.spec.K, self.spec.eval_classes, self.ds.rows
        pred, pr, nll, conf, oor = oracle(self.z, self.ds.y, K)
        assert res.rows == T and res.pred.dtype == torch.int32 and tuple(res.pred.shape) == (T,)
        wrong = int((res.pred.cpu().long() != pred).sum())
        print(f"[{tag}] rows {T} wrong predictions {wrong}")
        assert wrong == 0
        if proba:
            got = res.proba.cpu().double()
            assert tuple(got.shape) == (T, C) and res.proba.dtype == torch.float32
            assert bool(torch.isfinite(got).all())
            dp = (got - pr).abs().max(1).values
            ds_ = (got.sum(1) - 1).abs().max().item()
            print(f"[{tag}] max |dp| {dp.max().item():.3e} (bound at that row "
                  f"{(self.delta + 1e-6)[dp.argmax()].item():.3e}) max |sum p - 1| {ds_:.3e}")
            assert bool((dp <= self.delta + 1e-6).all())
            assert ds_ <= 1e-6
        else:
            assert res.proba is None
        if not labels:
            assert res.nll is None and res.confusion is None and res.log_loss is None
            assert res.f1 is None and res.accuracy is None and res.rows_out_of_range == 0
            return
        got = res.nll.cpu().double()
        assert res.nll.dtype == torch.float32 and tuple(got.shape) == (T,)
        assert torch.equal(torch.isnan(got), torch.isnan(nll)), "NaN markers differ"
        assert not bool(torch.isinf(got).any())
        ok = ~torch.isnan(nll)
        bound = 2 * self.delta + 1e-6 * self.zmax
        if bool(ok.any()):
            dn = (got[ok] - nll[ok]).abs()
            ll = float(nll[ok].mean())
            print(f"[{tag}] max |dnll| {dn.max().item():.3e} (bound there {bound[ok][dn.argmax()].item():.3e}) "
                  f"log_loss {res.log_loss:.9g} oracle {ll:.9g} bound {bound[ok].mean().item():.3e}")
            assert bool((dn <= bound[ok]).all())
            assert abs(res.log_loss - ll) <= bound[ok].mean().item()
        else:
            assert res.log_loss is None
        assert res.rows_out_of_range == oor
        assert res.confusion.dtype == torch.int64 and tuple(res.confusion.shape) == (C, C)
        assert torch.equal(res.confusion, conf.view(16, 16)[:C, :C])
        f1, acc = metrics_from_confusion(res.confusion.numpy())
        assert res.f1 == f1 and res.accuracy == acc


# ---- dense -------------------------------------------------------------------
def dense_case(F, K, T, scale=1.0, seed=0, zero_w=False):
    """X ~ 0.05 N(0,1) in bf16, w ~ scale N(0,1), intercepts N(0,1); labels uniform in [0, K)."""
    spec = ModelSpec(F, K)
    g = torch.Generator().manual_seed(1000 * F + 10 * K + T + seed)
    X = torch.zeros(T, spec.Fp)
    X[:, :F] = torch.randn(T, F, generator=g) * 0.05
    Xb = X.to(torch.bfloat16)
    if zero_w:
        w = torch.zeros(spec.P)
    else:
        w = spec.pack(torch.randn(K, F, generator=g) * scale, torch.randn(K, generator=g))
    y = torch.randint(0, K, (T,), generator=g).to(torch.int32)
    W, b = spec.coef(w).double(), spec.intercept(w).double()

    def margins():
        z = Xb[:, :F].double() @ W.t() + b
        return z, torch.full((T,), 2e-5 * max(1.0, float(z.abs().max())), dtype=torch.float64)

    z, delta = margins()
    if not zero_w:
        for _ in range(MAX_REDRAWS):
            bad = ~safe_rows(z, delta, K)
            if not bool(bad.any()):
                break
            n = int(bad.sum())
            Xb[bad, :F] = (torch.randn(n, F, generator=g) * 0.05).to(torch.bfloat16)
            z, delta = margins()
        assert bool(safe_rows(z, delta, K).all()), "unsafe rows after the redraw passes"
    return Case(spec, Dataset(Xb, y, F), w, z, delta)


# ---- wide --------------------------------------------------------------------
def _row(ds, r):
    a, b = int(ds.indptr[r]), int(ds.indptr[r + 1])
    return ds.idx[a:b].long(), ds.val[a:b]


def _margins64(spec, ds, w):
    """float64 margins [T, K] of the bf16 values as stored, and the fp32 recursive-sum bound
    (nnz + 8) 2^-24 (sum |v w| + |b|) per row and class."""
    K, KP, F = spec.K, spec.KP, spec.F
    W = w[: F * KP].view(F, KP)[:, :K].double()
    b = w[F * KP: F * KP + K].double()
    z = torch.zeros(ds.rows, K, dtype=torch.float64)
    bound = torch.zeros(ds.rows, K, dtype=torch.float64)
    for r in range(ds.rows):
        ids, v = _row(ds, r)
        t = v.double()[:, None] * W[ids]
        z[r] = t.sum(0) + b
        bound[r] = (len(ids) + 8) * U24 * (t.abs().sum(0) + b.abs())
    return z, bound


WIDE_F = 5000
WIDE_LENS = {1: [700], 3: [0, 65, 700], 4: [1, 63, 64, 700], 5: [0, 1, 64, 65, 63]}


def wide_lens(T):
    """Row lengths of a T-row wide case: 0, 1, 63, 64, 65 and 700 all occur over T in {1, 3, 4, 5}
    and within any T >= 8."""
    if T in WIDE_LENS:
        return WIDE_LENS[T]
    cyc = [0, 1, 63, 64, 65, 7, 20, 33]
    lens = [cyc[i % len(cyc)] for i in range(T)]
    lens[5] = 700
    return lens


def wide_case(K, T, scale=1.0, seed=0, zero_w=False, F=WIDE_F):
    """CSR rows of the lengths of wide_lens(T); every row of >= 2 entries repeats its first id
    once (an id repeated within a row counts as the sum of its entries)."""
    spec = WideSpec(F, K)
    g = torch.Generator().manual_seed(100 * K + T + seed)
    lens = wide_lens(T)

    def draw(n):
        ids = torch.randperm(F, generator=g)[:n]
        if n >= 2:
            ids[-1] = ids[0]
        v = torch.randn(n, generator=g)
        return ids.to(torch.int32), (torch.sign(v) * (v.abs() + 0.1) / max(n, 1) ** 0.5).to(torch.bfloat16)

    rows = [draw(n) for n in lens]
    if zero_w:
        w = torch.zeros(spec.P)
    else:
        w = spec.pack(torch.randn(K, F, generator=g) * scale, torch.randn(K, generator=g))
    y = torch.randint(0, max(K, 2), (T,), generator=g).to(torch.int32)

    def build():
        indptr = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0)
        return SparseDataset(indptr, torch.cat([r[0] for r in rows]), torch.cat([r[1] for r in rows]), y, F)

    ds = build()
    z, bound = _margins64(spec, ds, w)
    delta = bound.max(1).values
    if not zero_w:
        for _ in range(MAX_REDRAWS):
            bad = ~safe_rows(z, delta, K)
            if not bool(bad.any()):
                break
            for r in bad.nonzero().view(-1).tolist():
                rows[r] = draw(lens[r])
            ds = build()
            z, bound = _margins64(spec, ds, w)
            delta = bound.max(1).values
        assert bool(safe_rows(z, delta, K).all()), "unsafe rows after the redraw passes"
    return Case(spec, ds, w, z, delta)


def with_bad_labels(case, bad=(-1, None, 99)):
    """The case with labels -1, K and 99 planted among the valid ones (rows 1, 3 and the last)."""
    K, T = case.spec.K, case.ds.rows
    y = case.ds.y.clone()
    for pos, v in zip((1, 3, T - 1), bad):
        y[pos] = K if v is None else v
    ds = case.ds
    ds2 = Dataset(ds.X, y, ds.num_features) if hasattr(ds, "X") else SparseDataset(ds.indptr, ds.idx, ds.val, y,
                                                                                  ds.num_features)
    return Case(case.spec, ds2, case.w, case.z, case.delta)

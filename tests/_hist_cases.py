"""Float64 oracle of the score histogram (psx.ops.score with ``curves=True``), shared by
test_score_hist_cpu.py and test_gpu_score_hist.py.  Inputs and margin bounds are those of
_score_cases.py, unchanged.

Per row and class the one-vs-rest log-odds are l = z_c - logsumexp_{j != c}(z_j) (binary:
z_0), in float64 from ``case.z``.  Their error bound is the one _score_cases.py gives the
per-row loss, which has the same form (a margin minus a logsumexp of margins):
eps = 2 delta + 1e-6 zmax.  The bins an entry may land in are those of every value within
eps of l64: 256 + clamp(round(16 v), -256, 255) for |v - l64| <= eps.  An entry is *sure*
when that is one bin -- 16 l64 further than 16 eps from every half-integer, or beyond the
clamp by that margin -- and *unsure* otherwise (two adjacent bins while 16 eps < 1/2).  The
oracle gives per cell ``lo`` (the sure entries) and ``hi`` (``lo`` plus the unsure entries
that may land there); a correct table lies between them, and its side totals are exact.

MAX_UNSURE caps the share of unsure entries of every case the tests use.  It is asserted
from the oracle alone (test_score_hist_cpu.py), so a loose bound cannot hide a wrong kernel.
"""
import functools

import numpy as np
import torch

from _score_cases import Case, _margins64, dense_case, oracle, wide_case, with_bad_labels  # noqa: F401
from psx.utils.data import Dataset

NB = 512
MAX_UNSURE = 0.06

# (F, K, T, scale): the cases the cap was worked out for, then the rest of the GPU test's shapes
DENSE_TABLE = [(100, 2, 229, 1.0), (100, 6, 2000, 1.0), (1024, 6, 2000, 1.0), (2000, 16, 2000, 1.0),
               (512, 8, 2000, 20.0), (1024, 6, 2000, 20.0), (300, 5, 2000, 100.0), (128, 6, 40000, 1.0)]
DENSE_GPU = [(100, 2, 1, 1.0), (100, 6, 31, 1.0), (300, 5, 33, 1.0), (1024, 6, 229, 1.0), (1024, 16, 229, 1.0),
             (2000, 5, 229, 1.0), (2000, 16, 229, 1.0), (512, 8, 700, 20.0), (128, 6, 40000, 1.0)]
DENSE_ZERO = [(100, 6, 64), (100, 2, 64)]
# (K, T, scale)
WIDE_GPU = [(1, 400, 1.0), (2, 400, 1.0), (3, 400, 1.0), (6, 400, 1.0), (16, 400, 1.0), (6, 5000, 1.0),
            (6, 400, 30.0)]
WIDE_ZERO = [(6, 400), (1, 400)]


@functools.lru_cache(maxsize=None)
def dense(F, K, T, scale=1.0, zero_w=False):
    return dense_case(F, K, T, scale=scale, zero_w=zero_w)


@functools.lru_cache(maxsize=None)
def wide(K, T, scale=1.0, zero_w=False):
    return wide_case(K, T, scale=scale, zero_w=zero_w)


@functools.lru_cache(maxsize=None)
def planted(F=100, K=6, T=4000):
    """dense_case with the labels drawn from the model's own softmax (seeded): AUC well above 1/2."""
    base = dense(F, K, T)
    g = torch.Generator().manual_seed(7)
    y = torch.multinomial(torch.softmax(base.z, 1), 1, generator=g).view(-1).to(torch.int32)
    return Case(base.spec, Dataset(base.ds.X, y, F), base.w, base.z, base.delta)


def log_odds64(z, K):
    if K == 1:
        return z[:, :1].clone()
    cols = []
    for c in range(K):
        others = torch.cat([z[:, :c], z[:, c + 1:]], 1)
        cols.append(z[:, c] - torch.logsumexp(others, 1))
    return torch.stack(cols, 1)


def sides(y, K):
    """(side [T, Ch] in {0, 1}, ok [T]): the label side of every entry, and the rows that enter the table."""
    y = y.long()
    if K == 1:
        return (y > 0).long().view(-1, 1), torch.ones_like(y, dtype=torch.bool)
    return (y.view(-1, 1) == torch.arange(K).view(1, -1)).long(), (y >= 0) & (y < K)


class HistOracle:
    def __init__(self, case):
        K = case.spec.K
        self.K, self.Ch = K, K
        self.l64 = log_odds64(case.z, K)
        eps = (2 * case.delta + 1e-6 * case.zmax).view(-1, 1)
        x, e16 = 16 * self.l64, 16 * eps
        first = torch.ceil(x - e16 - 0.5).clamp(-256, 255).long() + 256  # lowest bin within eps
        last = torch.floor(x + e16 + 0.5).clamp(-256, 255).long() + 256  # highest
        self.side, self.ok = sides(case.ds.y, K)
        self.unsure = (last > first) & self.ok.view(-1, 1)
        self.entries = int(self.ok.sum()) * self.Ch
        self.unsure_share = float(self.unsure.sum()) / max(self.entries, 1)
        cls = torch.arange(self.Ch).view(1, -1).expand_as(first)
        base = (cls * 2 + self.side) * NB
        ok2 = self.ok.view(-1, 1).expand_as(first)
        sure = ok2 & ~self.unsure
        self.lo = torch.zeros(self.Ch * 2 * NB, dtype=torch.int64)
        self.lo.index_add_(0, (base + first)[sure], torch.ones(int(sure.sum()), dtype=torch.int64))
        self.hi = self.lo.clone()
        for k in range(int((last - first).max()) + 1 if first.numel() else 0):
            m = self.unsure & (first + k <= last)
            self.hi.index_add_(0, (base + first + k)[m], torch.ones(int(m.sum()), dtype=torch.int64))
        self.lo, self.hi = self.lo.view(self.Ch, 2, NB), self.hi.view(self.Ch, 2, NB)
        # exact side totals, and the unsure entries per class and side
        self.total = torch.stack([((self.side == s) & ok2).sum(0) for s in (0, 1)], 1)  # [Ch, 2]
        self.unsure_by_side = torch.stack([((self.side == s) & self.unsure).sum(0) for s in (0, 1)], 1)

    def check(self, hist, tag=""):
        """lo <= hist <= hi cell by cell, exact side totals; prints the figures first."""
        assert hist.dtype == torch.int64 and tuple(hist.shape) == (self.Ch, 2, NB)
        below, above = int((hist < self.lo).sum()), int((hist > self.hi).sum())
        print(f"[{tag}] entries {self.entries} unsure {100 * self.unsure_share:.2f} % cells below lo {below} "
              f"above hi {above} cells free to move {int((self.hi > self.lo).sum())}")
        assert below == 0 and above == 0
        assert torch.equal(hist.sum(2), self.total)

    def auc_exact(self):
        """Per-class ROC AUC of l64, pair-counted in float64 (ties one half); NaN without both sides."""
        out = np.full(self.Ch, np.nan)
        for c in range(self.Ch):
            pos = self.l64[:, c][self.ok & (self.side[:, c] == 1)]
            neg = self.l64[:, c][self.ok & (self.side[:, c] == 0)]
            if pos.numel() == 0 or neg.numel() == 0:
                continue
            wins = 0.0
            for p in pos.split(1024):
                wins += float((p.view(-1, 1) > neg.view(1, -1)).sum()) + 0.5 * float(
                    (p.view(-1, 1) == neg.view(1, -1)).sum())
            out[c] = wins / (pos.numel() * neg.numel())
        return out


_ORACLES = {}


def hist_oracle(case):
    """One oracle per case object (the builders above cache their cases)."""
    if id(case) not in _ORACLES:
        _ORACLES[id(case)] = (case, HistOracle(case))
    return _ORACLES[id(case)][1]


def check_planted_auc(res, case, tag=""):
    """|auc_hist - auc_exact| <= resolution + unsure_pos / P + unsure_neg / N per class: binning moves the
    AUC by at most the resolution, and one positive row in another bin by at most 1 / P, one negative by 1 / N."""
    o = hist_oracle(case)
    exact = o.auc_exact()
    P, N = o.total[:, 1].double().numpy(), o.total[:, 0].double().numpy()
    bound = res.auc_resolution + o.unsure_by_side[:, 1].numpy() / P + o.unsure_by_side[:, 0].numpy() / N
    for c in range(o.Ch):
        print(f"[{tag}] class {c} auc {res.auc[c]:.6f} exact {exact[c]:.6f} |d| {abs(res.auc[c] - exact[c]):.2e} "
              f"bound {bound[c]:.2e} (resolution {res.auc_resolution[c]:.2e})")
    assert float(np.nanmin(exact)) > 0.6, "the planted labels do not follow the scores"
    assert bool((np.abs(res.auc - exact) <= bound).all())
    return exact

"""Tables and drivers of the fitter sweeps (test_gpu_fit_geometry.py,
test_gpu_wide_fit_chain.py, test_fit_chain_cpu.py): which shapes are evaluated, which
are iterated under the invariant chain of _fit_chain.py, and how a native fitter is
driven one accepted step at a time.

Seeds are chosen on the float64 reference alone (test_fit_chain_cpu.py holds every
condition): the measured direction tolerance stays below 1e-3 max|d| along the
reference's own L-BFGS (``_fit_chain.emulate``), the float64 iterates of hist 1 and
hist 16 part by more than 10 x the 2e-2 trajectory tolerance after 20 steps, and the
retry start makes ``fit_reference`` spend a line-search budget (ls_fail >= 1)."""
import torch

import _fit_cases as fc
import _wide_fit_cases as wc
from _dense_cases import F_OF
from _fit_chain import DenseProblem, WideProblem, run_chain
from psx.ops.fit import BatchFitter, FitOptions
from psx.ops.lr import stream_handle
from psx.ops.wide_fit import DEFAULT_COL_CHUNK, WideFitter

N_ROWS = 97  # three 32-row tiles and one row
FPS = (128, 256, 512, 1024, 2048)
EVAL_K = (2, 3, 5, 9, 16)
# (F, K): the 25 cells, then nothing padded (twice), a single feature, K = 15
EVAL_CELLS = [(F_OF[FP], K) for FP in FPS for K in EVAL_K] + [(128, 4), (2048, 16), (1, 2), (129, 15)]
STAT_ROWS = (2, 33, 97, 229)
STAT_WG = (1, 3, None)
STAT_CONSTANTS = (0.1, -3.3, 1e-3, 240.0)  # rounded to bf16 by the dataset

# dense chain: (FP, K)
CHAIN_CELLS = [(128, 2), (256, 3), (512, 5), (1024, 9), (2048, 16), (2048, 2), (128, 16)]
CHAIN_STEPS = 6
CHAIN_REG = (0.0, 0.05)
RETRY = dict(FP=256, K=3, scale=8.0, ls_max=3, reg=0.05)
HIST = (1, 2, 10, 16)
HIST_STEPS = 20
HIST_DENSE = (229, 129, 3)  # N, F, K: the (256, 3) cell
HIST_WIDE = (229, 5000, 3)  # sparse_case(N, F, K)
# no penalty, and the seeds at which the oracle's hist 1 and hist 16 iterates part most after 20 steps
# (dense seeds 0..3: 0.20, 0.69, 0.68, 0.86 of the largest coefficient; wide seeds 0, 1: 0.44, 0.11)
HIST_REG = 0.0
HIST_DENSE_SEED = 1
HIST_WIDE_SEED = 0

WIDE_K = (1, 2, 3, 6, 16)  # KP 1, 2, 4, 8, 16
WIDE_SHAPE = (229, 5000)
WIDE_CHUNK = (64, None)
WIDE_WG = (3, None)


def stat_case(N, FP):
    """Rows for the statistics: N(0,1) x scales 0.2..5 + means, then the awkward columns
    (last F columns): four constants, one column with a single non-zero row, one whose
    rows alternate between two adjacent bf16 values around 100 (100 and 100.5)."""
    spec, ds, _ = fc.fit_case(N, F_OF[FP], 2, seed=FP + N)
    F = spec.F
    X = ds.X.float()
    special = {}
    for i, c in enumerate(STAT_CONSTANTS):
        X[:, F - 1 - i] = c
        special[F - 1 - i] = "const"
    X[:, F - 5] = 0.0
    X[N // 2, F - 5] = 0.75
    special[F - 5] = "single"
    X[:, F - 6] = 100.0
    X[1::2, F - 6] = 100.5
    special[F - 6] = "adjacent"
    ds.X = X.to(torch.bfloat16)
    assert torch.equal(ds.X[:, F - 6].float(), X[:, F - 6])  # both values are bf16 numbers
    return spec, ds, special


def one_pass_loss(col64):
    """Relative error of float64 on the one-pass formula sqrt((sum x^2 - n mean^2) / (n - 1))
    against the two-pass sigma, for one column."""
    n = col64.numel()
    two = float(col64.var(unbiased=True).sqrt())
    mean = float(col64.sum()) / n
    one = max((float((col64 * col64).sum()) - n * mean * mean) / (n - 1), 0.0) ** 0.5
    return abs(one - two) / two


# ---- dense fits ------------------------------------------------------------------------------
def dense_fit_inputs(FP, K, N=N_ROWS, F=None, seed=0):
    return fc.fit_case(N, F_OF[FP] if F is None else F, K, seed=seed)


def dense_start(spec, warm, scale=0.05, seed=3):
    return fc.warm_start(spec, seed=seed, scale=scale) if warm else None


def dense_x0(problem, w0):
    """The standardised start the device forms from w0 (float64)."""
    spec = problem.spec
    if w0 is None:
        return torch.zeros(problem.n, dtype=torch.float64)
    return problem.pack(spec.coef(w0).double() * problem.sigma, spec.intercept(w0).double())


def drive_dense(device, spec, ds, w0, reg, hist=10, steps=CHAIN_STEPS, ls_max=20, zero_const=True, max_wg=None,
                seed=0):
    """begin + ``steps`` accepted steps of the native dense fitter under the chain -> (Chain, native fitter)."""
    f = BatchFitter(spec, device, FitOptions(hist=hist, max_wg=max_wg))
    st = stream_handle(f.device)
    with torch.cuda.device(f.device):
        f._load(ds)
        nat = f._native
        w0d = None if w0 is None else w0.to(f.device, torch.float32).contiguous()
        nat.begin(w0d.data_ptr() if w0d is not None else 0, steps + 1, 0.0, float(reg), ls_max, zero_const, st)
        w = torch.empty(spec.P, dtype=torch.float32, device=f.device)
        ch = run_chain(nat, DenseProblem(spec, ds, reg), hist, steps, f.device, st, w_out=w,
                       current_of=lambda v: v, seed=seed)
    return ch, nat


# ---- wide fits -------------------------------------------------------------------------------
def drive_wide(device, spec, ds, w0, reg, hist=10, steps=CHAIN_STEPS, ls_max=20, zero_const=True, max_wg=None,
               col_chunk=None, seed=0, problem=None):
    f = WideFitter(spec, device, FitOptions(hist=hist, max_wg=max_wg, zero_const=zero_const, reg_param=reg),
                   col_chunk=col_chunk)
    st = stream_handle(f.device)
    p = problem or WideProblem(spec, ds, reg)
    with torch.cuda.device(f.device):
        d = f._load(ds)
        assert torch.equal(d.uniq.cpu().long(), p.f)
        nat = f._native
        w0d = None if w0 is None else w0.to(f.device, torch.float32).contiguous()
        nat.begin(w0d.data_ptr() if w0d is not None else 0, steps + 1, 0.0, float(reg), ls_max, zero_const, st)
        w = f._untouched(w0)
        ch = run_chain(nat, p, hist, steps, f.device, st, w_out=w, current_of=p.compact_current, seed=seed)
    return ch, nat, d


def wide_x0(problem, w0):
    spec = problem.spec
    if w0 is None:
        return torch.zeros(problem.n, dtype=torch.float64)
    c = spec.coef(w0).double()[:, problem.f]
    return problem.pack(c * problem.sigma, spec.intercept(w0).double())


__all__ = ["CHAIN_CELLS", "CHAIN_REG", "CHAIN_STEPS", "DEFAULT_COL_CHUNK", "EVAL_CELLS", "EVAL_K", "FPS", "HIST",
           "HIST_DENSE", "HIST_DENSE_SEED", "HIST_REG", "HIST_STEPS", "HIST_WIDE", "HIST_WIDE_SEED", "N_ROWS",
           "RETRY", "STAT_ROWS", "STAT_WG", "WIDE_CHUNK", "WIDE_K", "WIDE_SHAPE", "WIDE_WG", "dense_fit_inputs",
           "dense_start", "dense_x0", "drive_dense", "drive_wide", "one_pass_loss", "stat_case", "wc", "wide_x0"]

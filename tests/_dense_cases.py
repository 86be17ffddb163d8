"""Geometry table, inputs and float64 oracle cache of the dense solve tests
(test_gpu_dense_geometry.py).

The dense solve kernels are compiled once per padded feature width FP and padded
class count KP.  ``TABLE`` holds one entry per (FP, KP) cell with a real (F, K) that is
not the padded size, ``EXTRAS`` the boundary shapes; every entry records which forms of
the solver must take it.  Inputs come from ``window_case`` (bf16 rows, uncentred
features of scales 0.2 .. 5, one constant column, labels from a softmax model), the
reference is ``local_solve_reference`` in float64 on the window's rows in window order.

Two starting models: ``small`` (coefficients 0.05 N(0,1), iters 2: every line search
accepts early) and ``retry`` (8.0 N(0,1), iters 4, ls_max 6: line searches retry, so
the tail's slots run).  The solve centres the new intercepts, so the intercept deltas sum
to zero when the start's do -- to the fp32 rounding of the intercepts themselves, K 2^-24
max|b|.  For that to sit inside 1e-5 of the deltas' scale the start intercepts must not
dwarf the deltas: ``small`` starts from zero intercepts (as ``ModelSpec.init`` does; its
intercept deltas are as small as 6e-6 on a two-row window), ``retry`` from 0.1 N(0,1),
centred (its deltas are 0.02 .. 2); ``stable`` asserts the room per case.

``SEEDS`` are picked on the oracle alone (``stable``), never on a GPU result:
  * under a relative perturbation of w_old by 2^-18 -- what the bf16 hi + lo fragments
    lose -- the float64 oracle keeps (evals, accepted) and moves by at most a quarter of
    the delta tolerance (and of the loss tolerance);
  * the same oracle with every objective / gradient evaluated in float32 does too (what
    the fp32 accumulation of any device solve loses; the retry start puts margins in the
    hundreds, where a float32 loss can flip a line-search decision);
  * the retry start's line searches retry: evals > accepted + 1.
"""
import math
from collections import namedtuple

import torch

from psx.models import reference
from psx.models.logreg import ModelSpec
from psx.models.reference import local_solve_reference
from psx.ops.lr import SolverOptions
from psx.utils.data import Dataset

CAP = 128  # ring rows of the solve tests: 4 tiles
ROWS = 160  # rows per case: the ring's 128 + enough for three 50-row lane shards
FORMS = ("chain", "graph", "persist", "rows_bf16", "rows_fp32", "lanes")
F_OF = {128: 100, 256: 129, 512: 300, 1024: 1000, 2048: 2000}
K_OF = {2: 2, 4: 3, 8: 5, 16: 9}
# limits of the forms as the table records them: the CPU test holds the lanes flag to
# lanes_supported, the GPU tests assert the form that ran (persistent / rows_mode / eager)
PERSIST_MAX = (1024, 8)  # FP, KP
ROWS_F32_MAX_FP = 1024
LANES_MAX = (1024, 8)  # FP, K
LANES_CAP = 64

Entry = namedtuple("Entry", "FP KP F K forms")


def padded_classes(K):
    return 2 if K <= 2 else 4 if K <= 4 else 8 if K <= 8 else 16


def _entry(FP, KP, F, K):
    forms = {"chain", "graph", "rows_bf16"}
    if FP <= PERSIST_MAX[0] and KP <= PERSIST_MAX[1]:
        forms.add("persist")
    if FP <= ROWS_F32_MAX_FP:
        forms.add("rows_fp32")
    if FP <= LANES_MAX[0] and K <= LANES_MAX[1]:
        forms.add("lanes")
    return Entry(FP, KP, F, K, frozenset(forms))


TABLE = [_entry(FP, KP, F_OF[FP], K_OF[KP]) for FP in F_OF for KP in K_OF]
EXTRAS = [
    _entry(128, 4, 128, 4),  # nothing padded
    _entry(2048, 16, 2048, 16),  # nothing padded
    _entry(128, 2, 1, 2),  # a single real feature
    _entry(128, 8, 100, 8),  # K == KP at a narrow width
    _entry(256, 16, 129, 16),
]
ENTRIES = TABLE + EXTRAS
DIAGONAL = [(128, 2), (256, 4), (512, 8), (1024, 16), (2048, 16), (2048, 2)]
# the retry model runs in every form on the diagonal, the (., 16) and the (2048, .) cells
RETRY_CELLS = sorted(set(DIAGONAL) | {(FP, 16) for FP in F_OF} | {(2048, KP) for KP in K_OF})

W0 = (97, 0)  # three tiles and one row
WINDOWS = [W0, (128, 100), (33, 120), (2, 31)]  # full + wrapped; wraps the ring end; smallest with a variance
W_ONE = (1, 5)  # n = 1: every std 0, only the intercepts move
ONE_CELL = (256, 4)
SPREAD = dict(cell=(256, 4), cap=1088, window=(1050, 40))  # 34 tiles: more than one XCD's workgroups

MODELS = {"small": dict(scale=0.05, iters=2, ls_max=4), "retry": dict(scale=8.0, iters=4, ls_max=6)}
U18 = 2.0 ** -18
STABLE_TOL = 5e-3  # a quarter of the 2e-2 delta tolerance
STABLE_LOSS = 2.5e-4  # a quarter of the 1e-3 max(1, |loss|) loss tolerance

# (F, K, rows) -> generator seed: the first that passes ``stable`` for every window and
# model of the case.  Passed over (all with the retry start): F 1 K 2 seed 0 and F 100 K 2
# seed 1 (no line search retries); F 100 K 2 seed 0, F 129 K 2 seeds 0 .. 2, F 129 K 3
# seed 0, F 300 K 3 seed 0 and F 2000 K 2 seeds 0, 1 (the perturbed oracle's loss moves by
# 2.5e-4 .. 6.8e-2 of its size, its delta by up to 1.0e-1 of scale).
SEEDS = {(1, 2, ROWS): 1, (100, 2, ROWS): 2, (129, 2, ROWS): 3, (129, 3, ROWS): 1, (300, 3, ROWS): 1,
         (2000, 2, ROWS): 2}


def cell(FP, KP):
    return next(e for e in TABLE if (e.FP, e.KP) == (FP, KP))


def ident(e):
    return f"F{e.F}-K{e.K}"


def options(model, **kw):
    m = MODELS[model]
    return SolverOptions(iters=m["iters"], ls_max=m["ls_max"], **kw)


_DATA = {}
_ORACLE = {}


def window_case(F, K, rows=ROWS):
    """(spec, Dataset [rows][Fp] bf16, constant column or None), built once."""
    key = (F, K, rows)
    if key not in _DATA:
        spec = ModelSpec(F, K)
        g = torch.Generator().manual_seed(104729 * SEEDS.get(key, 0) + 13 * rows + F + K)
        scale = torch.logspace(math.log10(0.2), math.log10(5.0), F)[torch.randperm(F, generator=g)]
        mean = torch.randn(F, generator=g) * scale
        Z = torch.randn(rows, F, generator=g)
        X = Z * scale + mean
        const = F // 2 if F > 1 else None  # (F = 1: the one feature stays live)
        if const is not None:
            X[:, const] = 1.5
            Z[:, const] = 0.0
        W = torch.randn(K, F, generator=g) * (2.0 / math.sqrt(F))
        logits = Z @ W.t()
        if K > 2:
            logits[:, 0] = -1e9  # the phantom class 0 is absent
        y = torch.multinomial(torch.softmax(logits, 1), 1, generator=g).view(-1).to(torch.int32)
        Xp = torch.zeros(rows, spec.Fp)
        Xp[:, :F] = X
        _DATA[key] = (spec, Dataset(Xp.to(torch.bfloat16), y, F), const)
    return _DATA[key]


def start_model(spec, model, perturbed=False):
    """w_old [P] of a starting model; ``perturbed``: every entry times 1 +- 2^-18."""
    g = torch.Generator().manual_seed(4242 + spec.F + 31 * spec.K)
    coef = torch.randn(spec.K, spec.F, generator=g).double() * MODELS[model]["scale"]
    b = torch.randn(spec.K, generator=g).double() * (0.1 if model == "retry" else 0.0)
    b = b - b.mean()
    if perturbed:
        coef = coef * (1 + U18 * (2 * torch.randint(0, 2, coef.shape, generator=g) - 1))
        b = b * (1 + U18 * (2 * torch.randint(0, 2, b.shape, generator=g) - 1))
    return spec.pack(coef, b)


def window_rows(window, cap=CAP):
    B, start = window
    return (torch.arange(B) + start) % cap


def lane_rows(lane=1, L=3, n=50):
    return lane + L * torch.arange(n)


def _loss_grad32(X, y, coef_eff, b):
    loss, gc, gb = _loss_grad64(X.float(), y, coef_eff.float(), b.float())
    return loss.double(), gc.double(), gb.double()


_loss_grad64 = reference.multinomial_loss_grad


def oracle(F, K, rows_idx, model, variant="f64", rows=ROWS):
    """local_solve_reference on the case's rows ``rows_idx`` (in that order) from the model's
    start.  Variants for ``stable`` only: "pert" (w_old perturbed), "f32" (evaluations in float32)."""
    key = (F, K, rows, tuple(rows_idx.tolist()), model, variant)
    if key not in _ORACLE:
        spec, ds, _ = window_case(F, K, rows)
        o = options(model)
        w = start_model(spec, model, variant == "pert")
        reference.multinomial_loss_grad = _loss_grad32 if variant == "f32" else _loss_grad64
        try:
            _ORACLE[key] = local_solve_reference(ds.float_features()[rows_idx], ds.y[rows_idx].long(), spec.coef(w),
                                                 spec.intercept(w), iters=o.iters, hist=o.hist, ls_max=o.ls_max,
                                                 nslots=o.nslots)
        finally:
            reference.multinomial_loss_grad = _loss_grad64
    return _ORACLE[key]


def stable(F, K, rows_idx, model, rows=ROWS, retries=None):
    """The input condition, on the oracle alone: (ok, figures).  ``retries``: the line searches
    must retry (default: with the retry start)."""
    a = oracle(F, K, rows_idx, model, "f64", rows)
    sc, sb = max(a.delta_coef.abs().max().item(), 1e-6), max(a.delta_intercept.abs().max().item(), 1e-6)
    ok, fig = True, dict(evals=a.evals, accepted=a.accepted)
    for variant in ("pert", "f32"):
        b = oracle(F, K, rows_idx, model, variant, rows)
        mc = (a.delta_coef - b.delta_coef).abs().max().item() / sc
        mb = (a.delta_intercept - b.delta_intercept).abs().max().item() / sb
        ml = abs(a.loss - b.loss) / max(1.0, abs(a.loss))
        ok = ok and (a.evals, a.accepted) == (b.evals, b.accepted) and max(mc, mb) <= STABLE_TOL and ml <= STABLE_LOSS
        fig[variant] = (b.evals, b.accepted, mc, mb, ml)
    if model == "retry" if retries is None else retries:
        ok = ok and a.evals > a.accepted + 1
    # room for the centred intercept deltas' sum inside 1e-5 of their scale (module docstring)
    spec = ModelSpec(F, K)
    bmax = max(a.intercept.abs().max().item(), spec.intercept(start_model(spec, model)).abs().max().item())
    fig["b_rounding"] = K * 2.0 ** -24 * bmax / sb
    ok = ok and fig["b_rounding"] <= 0.25e-5
    return ok, fig


def solve_cases():
    """(F, K, rows of the case, row indices, model, retries, tag) of every solve of the GPU tests."""
    out = []
    for e in ENTRIES:
        for model in MODELS:
            out.append((e.F, e.K, ROWS, window_rows(W0), model, None, f"{ident(e)}-{model}-w97"))
        if "lanes" in e.forms and e in TABLE:
            # (the lanes' retry start is about four accepted steps -- three stored curvature
            # pairs --, whether or not a line search of the 50-row shard retries)
            for model in MODELS:
                out.append((e.F, e.K, ROWS, lane_rows(), model, False, f"{ident(e)}-{model}-lane1"))
    for FP, KP in DIAGONAL:
        e = cell(FP, KP)
        for model in MODELS:
            for w in windows_of(model)[1:]:
                out.append((e.F, e.K, ROWS, window_rows(w), model, None, f"{ident(e)}-{model}-w{w[0]}"))
    e = cell(*ONE_CELL)
    out.append((e.F, e.K, ROWS, window_rows(W_ONE), "small", None, f"{ident(e)}-small-w1"))
    e = cell(*SPREAD["cell"])
    out.append((e.F, e.K, SPREAD["cap"], window_rows(SPREAD["window"], SPREAD["cap"]), "small", None,
                f"{ident(e)}-spread"))
    return out


def windows_of(model):
    """The window shapes a diagonal cell runs consecutively: all four from the small start; the
    retry start on the three of at least a tile (the two-row and one-row windows are about the
    window statistics' edge, which does not depend on the start)."""
    return WINDOWS if model == "small" else WINDOWS[:3]

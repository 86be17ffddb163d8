"""Throughput of the scoring kernels against the unfused path they replace.

One process, device events, one warm-up and three timed repeats per variant, the
variants alternating inside every repeat:
  * baseline  -- the pieces that existed before the scoring kernels: ``logits`` /
    ``wide_logits`` into a [T][K] buffer, then torch softmax, argmax and NLL on
    the device;
  * fused     -- ``score`` / ``wide_score`` without probabilities (pred, nll, confusion);
  * fused+p   -- the same with the [T][C] probabilities.
Reported per variant: ms (min / median / max of the repeats), the input bytes per
second (rows and labels; the wide model's weight gathers are not counted) and that
rate as a share of the HBM peak -- the bound that applies: these passes do a few
FLOPs per byte.

``--curves`` measures the score histogram instead (``score(curves=True)``), with the
same protocol:
  * plain      -- ``score`` / ``wide_score`` as above (pred, nll, confusion): the pass
    the histogram rides in;
  * proba+hist -- what the tree offered for the same table before: the [T][C]
    probabilities from the kernel, then torch on the device (log-odds, bins, one
    ``bincount`` over the class / side / bin cells);
  * curves     -- the kernel with the histogram (pred, nll, confusion, table);
and, for the dense model, the same three on 2,048-wide rows with 16 classes (half the
rows), where the table does not fit in LDS and the kernel adds to the global table.

Usage: python tools/bench_score.py [--model dense|wide|both] [--rows N] [--curves] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from psx import _native  # noqa: E402
from psx.models.logreg import ModelSpec  # noqa: E402
from psx.models.wide import WideSpec  # noqa: E402
from psx.ops.lr import stream_handle  # noqa: E402
from psx.ops.score import HIST_FORMS, Scorer  # noqa: E402
from psx.ops.sparse import SparseDataset  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E (datasheet)
REPEATS = 3


def _time(variants: dict, repeats: int = REPEATS) -> dict:
    for fn in variants.values():  # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():  # alternate the variants inside a repeat
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def _report(name: str, ms: dict, nbytes: int) -> dict:
    out = {"case": name, "input_bytes": nbytes, "variants": {}}
    for k, v in ms.items():
        s = sorted(v)
        med = s[len(s) // 2]
        rate = nbytes / (med * 1e-3)
        out["variants"][k] = {"ms": v, "ms_min": s[0], "ms_median": med, "ms_max": s[-1], "input_bytes_per_s": rate,
                              "share_of_hbm_peak": rate / HBM_PEAK}
        print(f"{name:6s} {k:10s} ms min/med/max {s[0]:8.3f} {med:8.3f} {s[-1]:8.3f}   {rate / 1e12:6.3f} TB/s input   "
              f"{100 * rate / HBM_PEAK:5.1f} % of HBM peak (bandwidth bound)")
    return out


def _torch_tail(z, y, K):
    p = torch.softmax(z, 1)
    pred = z.argmax(1)
    nll = torch.logsumexp(z, 1) - z.gather(1, y.long().clamp(0, K - 1).view(-1, 1)).view(-1)
    return p, pred, nll


def _torch_hist(p, y, K):
    """The table from [T][C] probabilities: log-odds, the kernels' bins, one bincount."""
    if K == 1:
        l = (torch.log(p[:, 1]) - torch.log(p[:, 0])).view(-1, 1)
        side = (y > 0).long().view(-1, 1)
    else:
        l = torch.log(p) - torch.log1p(-p)
        side = (y.view(-1, 1) == torch.arange(K, device=p.device).view(1, -1)).long()
    b = 256 + torch.clamp(torch.round(16.0 * l), -256, 255).long()
    cell = (torch.arange(l.shape[1], device=p.device).view(1, -1) * 2 + side) * 512 + b
    return torch.bincount(cell.view(-1), minlength=l.shape[1] * 1024)


def bench_dense(dev, T: int, F: int = 1024, K: int = 6, curves: bool = False, hist_form: int = 0) -> dict:
    spec = ModelSpec(F, K)
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.empty(T, spec.Fp, dtype=torch.bfloat16, device=dev)
    for r0 in range(0, T, 1 << 16):
        r1 = min(T, r0 + (1 << 16))
        X[r0:r1] = (torch.randn(r1 - r0, spec.Fp, generator=g, device=dev) * 0.05).to(torch.bfloat16)
    y = torch.randint(0, K, (T,), generator=g, device=dev).to(torch.int32)
    sc = Scorer(spec, spec.init("random", seed=1, scale=1.0), dev)
    sc._hist_form = hist_form
    h, st, f = _native.hip(), stream_handle(dev), sc.frag
    z = torch.empty(T, K, dtype=torch.float32, device=dev)
    pred = torch.empty(T, dtype=torch.int32, device=dev)
    nll = torch.empty(T, dtype=torch.float32, device=dev)
    pr = torch.empty(T, K, dtype=torch.float32, device=dev)
    counts = torch.zeros(257, dtype=torch.int32, device=dev)

    def baseline():
        h.logits(spec.Fp, K, X.data_ptr(), T, f.hi.data_ptr(), f.lo.data_ptr(), f.b.data_ptr(), z.data_ptr(), st)
        return _torch_tail(z, y, K)

    def proba_hist():
        sc._dense_gpu(X, y, True, (pred, pr, nll, None), counts)
        return _torch_hist(pr, y, K)

    if curves:
        hist = torch.zeros(K * 1024, dtype=torch.int32, device=dev)
        ms = _time({"plain": lambda: sc._dense_gpu(X, y, True, (pred, None, nll, None), counts),
                    "proba+hist": proba_hist,
                    "curves": lambda: sc._dense_gpu(X, y, True, (pred, None, nll, hist), counts)})
        assert int(hist.sum()) == 4 * T * K  # the warm-up and the three repeats; no sync inside the timing
        return _report(f"dense F{F} K{K}", ms, T * spec.Fp * 2 + T * 4)
    ms = _time({"baseline": baseline,
                "fused": lambda: sc._dense_gpu(X, y, True, (pred, None, nll, None), counts),
                "fused+p": lambda: sc._dense_gpu(X, y, True, (pred, pr, nll, None), counts)})
    return _report("dense", ms, T * spec.Fp * 2 + T * 4)


def bench_wide(dev, T: int, nnz: int = 128, F: int = 1 << 20, K: int = 6, curves: bool = False) -> dict:
    spec = WideSpec(F, K)
    g = torch.Generator(device=dev).manual_seed(0)
    ds = SparseDataset(torch.arange(T + 1, dtype=torch.int64, device=dev) * nnz,
                       torch.randint(0, F, (T * nnz,), generator=g, device=dev).to(torch.int32),
                       (torch.randn(T * nnz, generator=g, device=dev) / nnz ** 0.5).to(torch.bfloat16),
                       torch.randint(0, K, (T,), generator=g, device=dev).to(torch.int32), F)
    sc = Scorer(spec, spec.init("random", seed=1, scale=1.0), dev)
    h, st = _native.hip(), stream_handle(dev)
    z = torch.empty(T, spec.KP, dtype=torch.float32, device=dev)
    pred = torch.empty(T, dtype=torch.int32, device=dev)
    nll = torch.empty(T, dtype=torch.float32, device=dev)
    pr = torch.empty(T, K, dtype=torch.float32, device=dev)
    counts = torch.zeros(257, dtype=torch.int32, device=dev)

    def baseline():
        h.wide_logits(K, spec.KP, F, ds.indptr.data_ptr(), ds.idx.data_ptr(), ds.val.data_ptr(), T, sc.w.data_ptr(),
                      z.data_ptr(), st)
        return _torch_tail(z[:, :K], ds.y, K)

    def proba_hist():
        sc._wide_gpu(ds, True, (pred, pr, nll, None), counts)
        return _torch_hist(pr, ds.y, K)

    if curves:
        hist = torch.zeros(K * 1024, dtype=torch.int32, device=dev)
        ms = _time({"plain": lambda: sc._wide_gpu(ds, True, (pred, None, nll, None), counts),
                    "proba+hist": proba_hist,
                    "curves": lambda: sc._wide_gpu(ds, True, (pred, None, nll, hist), counts)})
        assert int(hist.sum()) == 4 * T * K
        return _report(f"wide K{K}", ms, T * nnz * 6 + (T + 1) * 8 + T * 4)
    ms = _time({"baseline": baseline,
                "fused": lambda: sc._wide_gpu(ds, True, (pred, None, nll, None), counts),
                "fused+p": lambda: sc._wide_gpu(ds, True, (pred, pr, nll, None), counts)})
    return _report("wide", ms, T * nnz * 6 + (T + 1) * 8 + T * 4)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="both", choices=["dense", "wide", "both"])
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--curves", action="store_true", help="measure the score histogram (see the module text)")
    ap.add_argument("--hist_form", default="auto", choices=sorted(HIST_FORMS),
                    help="with --curves: the dense kernel's histogram form at the 1,024-wide shape")
    ap.add_argument("--out", default=None, help="also write the results as JSON")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_score: no GPU -- not measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    res = []
    if a.model in ("dense", "both"):
        res.append(bench_dense(dev, a.rows, curves=a.curves, hist_form=HIST_FORMS[a.hist_form]))
        if a.curves:
            torch.cuda.empty_cache()
            res.append(bench_dense(dev, max(a.rows // 2, 1), F=2048, K=16, curves=True))
            torch.cuda.empty_cache()
    if a.model in ("wide", "both"):
        res.append(bench_wide(dev, a.rows, curves=a.curves))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Measurements of the full-batch fit (psx/ops/fit.py) on one GPU.

  eval     one evaluation (loss + gradient, ``loss_grad``) over --rows x 1,024 bf16 rows,
           K = 6, against what the streaming solver offers for the same thing: a
           rows-mode ``LocalSolveOp`` solve on a ring holding the same rows, as total
           solve time / evaluations and as the slope between a 1-slot and a 9-slot solve
           (which takes the solve's statistics pass out).  One process, device events,
           one warm-up, three repeats, the variants alternating inside every repeat.
  truth    BASELINE.md's ground-truth row: fit the 90k-row synthetic fine-food set with
           default options, score the 4,877-row test set.
  ceiling  a fit of --ceiling_rows x 1,024 rows drawn on the device from a planted
           softmax model (a size whose float64 copy no host holds).

Usage: python tools/bench_fit.py [--what eval,truth,ceiling] [--rows N] [--ceiling_rows N] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from psx.models.logreg import ModelSpec  # noqa: E402
from psx.ops.fit import BatchFitter  # noqa: E402
from psx.ops.lr import LocalSolveOp, SolverOptions  # noqa: E402
from psx.ops.score import Scorer  # noqa: E402
from psx.runtime.buffer import DeviceRing  # noqa: E402
from psx.utils.data import Dataset, synth_finefood  # noqa: E402

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


def _mmm(v):
    s = sorted(v)
    return s[0], s[len(s) // 2], s[-1]


def planted(dev, rows: int, F: int, K: int, seed: int, W=None, chunk: int = 1 << 18):
    """Rows ~ 0.05 N(0,1) in bf16 and labels 1..K-1 drawn from a planted softmax model, built on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    if W is None:
        W = torch.randn(K, F, generator=g, device=dev)
    X = torch.empty(rows, F, dtype=torch.bfloat16, device=dev)
    y = torch.empty(rows, dtype=torch.int32, device=dev)
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        xb = (torch.randn(r1 - r0, F, generator=g, device=dev) * 0.05).to(torch.bfloat16)
        X[r0:r1] = xb
        y[r0:r1] = torch.multinomial(torch.softmax(_logits(xb, W), 1), 1, generator=g).view(-1).to(torch.int32)
    return Dataset(X, y, F), W


def _logits(X, W):
    z = X.float() @ W.t()
    z[:, 0] = float("-inf")  # the phantom class never occurs
    return z


def bench_eval(dev, rows: int, F: int = 1024, K: int = 6) -> dict:
    spec = ModelSpec(F, K)
    ds, _ = planted(dev, rows, spec.Fp, K, seed=0)
    ring = DeviceRing(rows, spec.Fp, dev)
    ring.place(ds.X, ds.y, 0)
    ds = Dataset(ring.X, ring.y, F)  # one copy of the rows for both
    w = spec.init("random", seed=1, scale=0.05).to(dev)
    fitter = BatchFitter(spec, dev)
    full = LocalSolveOp(spec, rows, dev, SolverOptions(iters=2))
    init = LocalSolveOp(spec, rows, dev, SolverOptions(iters=1, ls_max=0))
    ms = _time({"fit_eval": lambda: fitter.loss_grad(ds, w),
                "solve_9_slots": lambda: full.run(ring, rows, 0, w),
                "solve_1_slot": lambda: init.run(ring, rows, 0, w)})
    ev_full, ev_init = int(full.stats[0].item()), int(init.stats[0].item())
    nbytes = rows * spec.Fp * 2
    out = {"rows": rows, "row_bytes": nbytes, "ms": ms, "solve_evals": ev_full, "init_evals": ev_init,
           "rows_mode": bool(full._native.rows_mode), "grid": int(fitter._native.grid)}
    f0, f1, f2 = _mmm(ms["fit_eval"])
    a0, a1, a2 = _mmm(ms["solve_9_slots"])
    b0, b1, b2 = _mmm(ms["solve_1_slot"])
    print(f"rows {rows} x {spec.Fp} bf16 ({nbytes / 1e9:.2f} GB), fit grid {out['grid']} workgroups")
    print(f"fit one evaluation   ms min/med/max {f0:8.3f} {f1:8.3f} {f2:8.3f}   {nbytes / f1 / 1e9:6.3f} TB/s of rows")
    print(f"solve, 9 slots       ms min/med/max {a0:8.3f} {a1:8.3f} {a2:8.3f}   evaluations {ev_full}: "
          f"{a1 / ev_full:8.3f} ms per evaluation ({nbytes / (a1 / ev_full) / 1e9:6.3f} TB/s)")
    print(f"solve, 1 slot        ms min/med/max {b0:8.3f} {b1:8.3f} {b2:8.3f}   evaluations {ev_init}")
    if ev_full > ev_init:
        slope = (a1 - b1) / (ev_full - ev_init)
        out["slot_ms_slope"] = slope
        print(f"slope: {slope:8.3f} ms per further slot ({nbytes / slope / 1e9:6.3f} TB/s), statistics pass taken out")
    return out


def _fit_report(name, res, extra=None):
    ev = res.evals
    line = {"case": name, "seconds": res.seconds, "iters": res.iters, "evals": ev, "reason": res.reason,
            "objective": res.objective, "log_loss": res.log_loss, "pass_seconds": res.pass_seconds}
    line.update(extra or {})
    print(json.dumps(line))
    return line


def bench_truth(dev) -> dict:
    train, test = synth_finefood(90000, seed=0), synth_finefood(4877, seed=1)
    spec = ModelSpec(train.num_features, 6)
    fitter = BatchFitter(spec, dev)
    fitter.fit(train, w0=None)  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    on_dev = train.to(dev)
    torch.cuda.synchronize()
    h2d = time.perf_counter() - t0
    res = fitter.fit(on_dev)
    evs = list(fitter._native.eval_seconds)
    sc = Scorer(spec, res.w, dev).score(test.to(dev))
    return _fit_report("truth_90k", res, {"h2d_seconds": h2d, "eval_seconds_total": sum(evs),
                                          "share_in_evaluations": sum(evs) / res.seconds,
                                          "test_accuracy": sc.accuracy, "test_f1": sc.f1, "test_log_loss": sc.log_loss})


def bench_ceiling(dev, rows: int, F: int = 1024, K: int = 6) -> dict:
    spec = ModelSpec(F, K)
    t0 = time.perf_counter()
    train, W = planted(dev, rows, spec.Fp, K, seed=2)
    test, _ = planted(dev, 1 << 16, spec.Fp, K, seed=3, W=W)
    torch.cuda.synchronize()
    gen = time.perf_counter() - t0
    bayes = float((_logits(test.X, W).argmax(1).to(torch.int32) == test.y).float().mean())
    res = BatchFitter(spec, dev).fit(train)
    sc = Scorer(spec, res.w, dev).score(test)
    return _fit_report(f"ceiling_{rows}", res, {"rows": rows, "generate_seconds": gen, "test_accuracy": sc.accuracy,
                                                "test_f1": sc.f1, "planted_model_accuracy": bayes,
                                                "row_TB_per_s": rows * spec.Fp * 2 / res.pass_seconds / 1e12})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="eval,truth")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--ceiling_rows", type=int, default=1 << 24)
    ap.add_argument("--out", default=None, help="also write the results as JSON")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_fit: no GPU -- not measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    res = {}
    for what in a.what.split(","):
        if what == "eval":
            res[what] = bench_eval(dev, a.rows)
        elif what == "truth":
            res[what] = bench_truth(dev)
        elif what == "ceiling":
            res[what] = bench_ceiling(dev, a.ceiling_rows)
        else:
            ap.error(f"unknown measurement {what!r}")
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

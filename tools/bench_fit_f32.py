"""fp32-row fit (csrc/kernels/fit_f32.hip) on one GPU beside the bf16 fit on the same rows rounded:
one evaluation (``loss_grad``), its launches, and one scoring pass of each.

    python tools/bench_fit_f32.py [--rows 1048576] [--features 1024] [--classes 6] [--center] [--out FILE]

``--center`` times the centred mode of the fp32 family (``F32Fitter(center=True)``, the scorer with the rows' centre).

The two families are timed alternately in one session (medians of ``--repeats`` after warm-up calls,
device events around the whole call, host side included); bytes/s count one read of the rows,
4 B per value for fp32 and 2 B for bf16."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from psx.models.logreg import ModelSpec  # noqa: E402
from psx.ops.fit import BatchFitter  # noqa: E402
from psx.ops.fit_f32 import F32Fitter, F32Scorer  # noqa: E402
from psx.ops.lr import stream_handle  # noqa: E402
from psx.ops.score import Scorer  # noqa: E402
from psx.utils.data import Dataset  # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(fns, repeats, warmup):
    """Median milliseconds of every callable, the callables taking turns."""
    ms = [[] for _ in fns]
    for i in range(warmup + repeats):
        for k, fn in enumerate(fns):
            t = once(fn)
            if i >= warmup:
                ms[k].append(t)
    return [sorted(v)[len(v) // 2] for v in ms]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--center", action="store_true", help="the fp32 family's centred mode")
    ap.add_argument("--out", default=None, help="also write the results as JSON")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_fit_f32: no GPU -- not measured", file=sys.stderr)
        return 0
    dev = torch.device("cuda:0")
    rows, K = a.rows // 32 * 32, a.classes
    spec = ModelSpec(a.features, K)
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.zeros(rows, spec.Fp, dtype=torch.float32, device=dev)
    X[:, : spec.F] = torch.randn(rows, spec.F, generator=g, device=dev)
    y = torch.randint(0, K, (rows,), generator=g, device=dev).to(torch.int32)
    ds32, ds16 = Dataset(X, y, spec.F), Dataset(X.to(torch.bfloat16), y, spec.F)
    w = spec.init("random", seed=1, scale=0.05).to(dev)
    f32, f16 = F32Fitter(spec, dev, center=a.center), BatchFitter(spec, dev)
    f32.loss_grad(ds32, w)
    f16.loss_grad(ds16, w)
    center = f32.loss_grad_centred(ds32, w)[2][: spec.F] if a.center else None
    s32, s16 = F32Scorer(spec, ds32, dev, center=center), Scorer(spec, w, dev)
    b32, b16 = rows * spec.Fp * 4, rows * spec.Fp * 2
    ev32, ev16, sc32, sc16 = alternated(
        [lambda: f32.loss_grad(ds32, w), lambda: f16.loss_grad(ds16, w), lambda: s32.score(w), lambda: s16.score(ds16)],
        a.repeats, a.warmup)
    lm = f32._native.time_launches(w.data_ptr(), 5, stream_handle(dev))
    out = {"rows": rows, "F": spec.F, "Fp": spec.Fp, "K": K, "center": bool(a.center), "grid_f32": int(f32._native.grid),
           "grid_bf16": int(f16._native.grid), "eval_ms": {"fp32": ev32, "bf16": ev16},
           "score_ms": {"fp32": sc32, "bf16": sc16}, "launch_ms_fp32": {"lossgrad": lm[0], "reduce": lm[1]},
           "eval_TBps": {"fp32": b32 / ev32 / 1e9, "bf16": b16 / ev16 / 1e9},
           "score_TBps": {"fp32": b32 / sc32 / 1e9, "bf16": b16 / sc16 / 1e9},
           "lossgrad_launch_TBps_fp32": b32 / lm[0] / 1e9}
    print(f"rows {rows} x {spec.Fp} (F {spec.F}), K {K}{', centred' if a.center else ''}: fp32 {b32 / 1e9:.2f} GB (grid {out['grid_f32']}), "
          f"bf16 {b16 / 1e9:.2f} GB (grid {out['grid_bf16']})")
    for name, ms, tb in (("evaluation", out["eval_ms"], out["eval_TBps"]), ("score pass", out["score_ms"], out["score_TBps"])):
        print(f"{name:11s} fp32 {ms['fp32']:8.3f} ms {tb['fp32']:.3f} TB/s | bf16 {ms['bf16']:8.3f} ms {tb['bf16']:.3f} TB/s"
              f" | fp32 / bf16 bytes/s {tb['fp32'] / tb['bf16']:.2f}")
    print(f"fp32 launches: lossgrad {lm[0]:.3f} ms ({out['lossgrad_launch_TBps_fp32']:.3f} TB/s), reduce {lm[1]:.3f} ms")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Panel fit (csrc/kernels/panel_fit.hip) on one GPU: one evaluation and its launches, the
score pass, a full fit, the same loss + gradient in torch on the same device, and the
2,048-wide dense fit's evaluation (tools/bench_fit.py's ``fit_eval``) on the same bytes.

    python tools/bench_panel_fit.py [--rows 131072] [--features 8192] [--classes 6] [--out FILE]

An evaluation reads the rows twice: its bytes/s are counted as two reads."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from psx.models.logreg import ModelSpec  # noqa: E402
from psx.ops.fit import BatchFitter, FitOptions  # noqa: E402
from psx.ops.lr import stream_handle  # noqa: E402
from psx.ops.panel_fit import PanelDataset, PanelFitter, PanelScorer, PanelSpec  # noqa: E402
from psx.utils.data import Dataset  # noqa: E402


def timed(fn, repeats=7, warmup=2):
    """Median milliseconds of ``fn`` between device events."""
    ms = []
    for i in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def planted(dev, rows, F, Fp, K, chunk=1 << 14):
    """Rows ~ 0.05 N(0,1) in bf16, labels from a planted softmax model, built on the device in the padded container."""
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(K, F, generator=g, device=dev)
    X = torch.zeros(rows, Fp, dtype=torch.bfloat16, device=dev)
    y = torch.empty(rows, dtype=torch.int32, device=dev)
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        xb = (torch.randn(r1 - r0, F, generator=g, device=dev) * 0.05).to(torch.bfloat16)
        X[r0:r1, :F] = xb
        y[r0:r1] = torch.multinomial(torch.softmax(xb.float() @ W.t(), 1), 1, generator=g).view(-1).to(torch.int32)
    return X, y


def torch_loss_grad(X, y, Wt, b):
    """Mean cross entropy and its gradient with bf16 matmuls (fp32 accumulation) -- what a torch user would run."""
    z = (X @ Wt).float() + b
    lse = torch.logsumexp(z, 1)
    loss = (lse - z.gather(1, y.view(-1, 1)).view(-1)).mean()
    R = torch.softmax(z, 1)
    R[torch.arange(X.shape[0], device=X.device), y] -= 1.0
    return loss, (R.to(torch.bfloat16).t() @ X).float() / X.shape[0], R.mean(0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 17)
    ap.add_argument("--features", type=int, default=8192)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--max_iter", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the results as JSON")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_panel_fit: no GPU -- not measured", file=sys.stderr)
        return 0
    dev = torch.device("cuda:0")
    rows, K = a.rows // 32 * 32, a.classes
    spec = PanelSpec(a.features, K)
    X, y = planted(dev, rows, spec.F, spec.Fp, K)
    ds = PanelDataset(X, y, spec.F, None, rows)
    w = spec.init("random", seed=1, scale=0.05).to(dev)
    nbytes = rows * spec.Fp * 2
    live = (spec.F + 1023) // 1024 * 1024 * rows * 2  # the panels the kernels read
    f = PanelFitter(spec, dev, FitOptions(max_iter=a.max_iter, reg_param=1e-3))
    f.loss_grad(ds, w)
    out = {"rows": rows, "F": spec.F, "Fp": spec.Fp, "K": K, "row_bytes": nbytes, "grid": int(f._native.grid)}
    out["eval_ms"] = timed(lambda: f.loss_grad(ds, w))
    out["launch_ms"] = dict(zip(("fwd", "resid", "bwd", "reduce"),
                                f._native.time_launches(w.data_ptr(), 5, stream_handle(dev))))
    sc = PanelScorer(spec, ds, dev)
    out["score_ms"] = timed(lambda: sc.score(w, proba=True))
    res = f.fit(ds)
    out["fit"] = {"seconds": res.seconds, "iters": res.iters, "evals": res.evals, "reason": res.reason,
                  "pass_ms": res.pass_seconds * 1e3, "objective": res.objective}
    Wt, b, yl = spec.coef(w).t().to(torch.bfloat16).contiguous(), spec.intercept(w), y.long()
    out["torch_ms"] = timed(lambda: torch_loss_grad(X[:, : spec.F], yl, Wt, b))
    out["eval_TBps_two_reads"] = 2 * live / out["eval_ms"] / 1e9
    # the 2,048-wide dense evaluation on the same number of row bytes
    dspec = ModelSpec(2048, K)
    dds = Dataset(X.view(-1, 2048), y.repeat_interleave(spec.Fp // 2048), 2048)
    df = BatchFitter(dspec, dev)
    dw = dspec.init("random", seed=1, scale=0.05).to(dev)
    out["dense2048_ms"] = timed(lambda: df.loss_grad(dds, dw))
    out["dense2048_TBps"] = nbytes / out["dense2048_ms"] / 1e9
    out["ratio_to_dense2048"] = out["eval_TBps_two_reads"] / out["dense2048_TBps"]
    lm = out["launch_ms"]
    print(f"rows {rows} x {spec.Fp} bf16 (F {spec.F}, {nbytes / 1e9:.2f} GB), K {K}, grid {out['grid']} x "
          f"{(spec.F + 1023) // 1024} panels")
    print(f"one evaluation  {out['eval_ms']:8.3f} ms  {out['eval_TBps_two_reads']:.3f} TB/s counted as two reads "
          f"of the live panels; launches fwd {lm['fwd']:.3f} resid {lm['resid']:.3f} bwd {lm['bwd']:.3f} "
          f"reduce {lm['reduce']:.3f} ms")
    print(f"score pass      {out['score_ms']:8.3f} ms (with probabilities)")
    print(f"torch loss+grad {out['torch_ms']:8.3f} ms (bf16 matmuls): panel / torch {out['eval_ms'] / out['torch_ms']:.2f}")
    print(f"dense 2,048     {out['dense2048_ms']:8.3f} ms  {out['dense2048_TBps']:.3f} TB/s (one read); "
          f"panel bytes/s / dense bytes/s {out['ratio_to_dense2048']:.2f}")
    print(f"fit             {res.seconds:.3f} s, {res.iters} iterations, {res.evals} evaluations, reason {res.reason}, "
          f"median pass {res.pass_seconds * 1e3:.3f} ms")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())

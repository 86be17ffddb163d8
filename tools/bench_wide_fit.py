"""Measurements of the wide full-batch fit (psx/ops/wide_fit.py) on one GPU.

  eval     one evaluation (the loss + gradient of ``loss_grad``, and a fit's evaluation, whose
           reduction also forms the solver's fp64 dots) over --rows synthetic hashed rows
           (nnz ~ 48, F = 2^20), K = 6 and K = 1, split into row pass / column pass / reduction (device events around the
           three stages), beside wide_score_kernel on the same rows (the same gathers) and a
           torch baseline on the same device: CSR matmul forward, softmax / sigmoid,
           transposed-CSR matmul backward.  One process, one warm-up, --repeats repeats, the
           variants alternating inside every repeat; the column-length distribution is
           printed beside the times.
  chunk    the column pass at col_chunk 128 .. 4096.
  setup    seconds and device memory of loading the dataset (sorts, inverted index, items,
           statistics, workspace).
  fit      a full fit of the same rows: iterations, evaluations, seconds.
  --weights  (instead of --what) one evaluation with row weights, class weights and a
           held-out fold against the plain one by stage, the two alternating inside every
           repeat; the fold switch (the weights kernel plus the weighted statistics, device
           events around set_weights); and, with --cv FOLDS, the wall time of a
           FOLDS x 3-penalty cross_validate of 10 iterations a fit.

  --many   (instead of --what) many fits per read of the rows (csrc/kernels/wide_fit_many.hip): one raw
           evaluation of 1, slots / 2 and slots models (the round of loss_grad_many: all passes, the
           reductions, the copy of the result blocks and the wait) against that many plain weighted
           evaluations (device events around the three stages), alternating inside every repeat; and a
           5-fold x 4-penalty cross_validate of 10 iterations a fit, batched against sequential, alternating.

Usage: python tools/bench_wide_fit.py [--what eval,chunk,setup,fit | --weights [--cv 5] | --many] [--rows N] [--out FILE.json]
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

from psx import _native  # noqa: E402
from psx.models.wide import WideSpec  # noqa: E402
from psx.ops.fit import FitOptions, FitWeights, _Weights, cross_validate  # noqa: E402
from psx.ops.lr import stream_handle  # noqa: E402
from psx.ops.wide_fit import DEFAULT_COL_CHUNK, WideFitter  # noqa: E402
from psx.utils.data import synth_sparse  # noqa: E402

F = 1 << 20


def _med(v):
    s = sorted(v)
    return s[len(s) // 2]


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _data(dev, rows, K):
    return synth_sparse(rows, F, "binary" if K == 1 else "finefood", device=dev, seed=0)


def _columns(ds):
    cnt = torch.bincount(ds.idx.long())
    cnt = cnt[cnt > 0].double()
    return {"touched": int(cnt.numel()), "median": float(cnt.median()), "p99": float(torch.quantile(cnt, 0.99)),
            "max": int(cnt.max()), "nnz": ds.nnz}


def _stages(fitter, ds, w, repeats):
    """Median ms of the row pass, the column pass, the reduction of ``loss_grad`` (raw:
    gradient only) and the reduction of a fit's evaluation (with the 4 + 2 hist fp64
    dots over the solver's vectors)."""
    st = stream_handle(fitter.device)
    fitter.loss_grad(ds, w)  # loads the dataset, sets the trial weights, warms up
    raw, fit = [], []
    for _ in range(repeats):  # the two reductions alternate inside a repeat
        raw.append(fitter._native.stage_ms(True, st))
        fit.append(fitter._native.stage_ms(False, st))
    rows, cols, red = [_med([r[i] for r in raw]) for i in range(3)]
    return rows, cols, red, _med([r[2] for r in fit])


def bench_eval(dev, rows, K, repeats):
    spec = WideSpec(F, K)
    ds = _data(dev, rows, K)
    w = spec.init("random", seed=1, scale=0.05).to(dev)
    fitter = WideFitter(spec, dev)
    h, st = _native.hip(), stream_handle(dev)
    pred = torch.empty(rows, dtype=torch.int32, device=dev)
    nll = torch.empty(rows, dtype=torch.float32, device=dev)
    counts = torch.zeros(257, dtype=torch.int32, device=dev)

    def score():
        h.wide_score(spec.K, spec.KP, spec.F, ds.indptr.data_ptr(), ds.idx.data_ptr(), ds.val.data_ptr(),
                     ds.y.data_ptr(), rows, w.data_ptr(), stream=st, pred=pred.data_ptr(), nll=nll.data_ptr(),
                     conf=counts.data_ptr(), oor=counts.data_ptr() + 1024)

    rowsp, colsp, red, red_fit = _stages(fitter, ds, w, repeats)
    # the torch baseline works in the touched subspace too, on the fitter's own inverted index
    d = fitter._data
    A = torch.sparse_csr_tensor(d.indptr, d.col.long(), d.val.float(), size=(rows, d.U))
    At = torch.sparse_csr_tensor(d.colptr, d.crow.long(), d.cval.float(), size=(d.U, rows))
    Wd = w[: F * spec.KP].view(F, spec.KP)[d.uniq.long()][:, :K].contiguous()
    y = ds.y.long()

    def torch_eval():
        z = A @ Wd + w[F * spec.KP: F * spec.KP + K]
        if K == 1:
            r = torch.sigmoid(z) - (y > 0).float().view(-1, 1)
        else:
            r = torch.softmax(z, 1)
            r[torch.arange(rows, device=dev), y] -= 1.0
        return At @ r

    score()
    torch_eval()
    torch.cuda.synchronize()
    ms = {"wide_score": [], "torch": []}
    for _ in range(repeats):
        ms["wide_score"].append(_event_ms(score))
        ms["torch"].append(_event_ms(torch_eval))
    out = {"rows": rows, "K": K, "columns": _columns(ds), "col_chunk": fitter.col_chunk,
           "items": int(fitter._data.n_items), "long_items": int(fitter._data.long_items.numel()),
           "rows_ms": rowsp, "cols_ms": colsp, "reduce_raw_ms": red, "reduce_fit_ms": red_fit,
           "loss_grad_ms": rowsp + colsp + red, "fit_eval_ms": rowsp + colsp + red_fit,
           "wide_score_ms": _med(ms["wide_score"]), "torch_ms": _med(ms["torch"])}
    print(json.dumps(out))
    return out


def bench_chunk(dev, rows, K, repeats):
    spec = WideSpec(F, K)
    ds = _data(dev, rows, K)
    w = spec.init("random", seed=1, scale=0.05).to(dev)
    out = []
    for cc in (128, 256, 512, 1024, 2048, 4096):
        fitter = WideFitter(spec, dev, col_chunk=cc)
        r, c, d, df = _stages(fitter, ds, w, repeats)
        out.append({"K": K, "col_chunk": cc, "items": int(fitter._data.n_items),
                    "long_items": int(fitter._data.long_items.numel()), "rows_ms": r, "cols_ms": c,
                    "reduce_raw_ms": d, "reduce_fit_ms": df})
        print(json.dumps(out[-1]))
        del fitter
    return out


def bench_setup(dev, rows, K):
    spec = WideSpec(F, K)
    ds = _data(dev, rows, K)
    fitter = WideFitter(spec, dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t0 = time.perf_counter()
    d = fitter._load(ds)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    index = sum(t.numel() * t.element_size() for t in vars(d).values() if isinstance(t, torch.Tensor))
    # the native workspace: 9 + 2 hist vectors of U*KP + KP floats, R [N][KP], gitem [items][KP]
    work = 4 * spec.KP * ((9 + 2 * fitter.opts.hist) * (d.U + 1) + rows + d.n_items)
    out = {"rows": rows, "K": K, "set_data_seconds": dt, "dataset_bytes": ds.nnz * 6 + rows * 12,
           "torch_peak_bytes": torch.cuda.max_memory_allocated(dev) - base, "index_bytes": index,
           "workspace_bytes": work}
    print(json.dumps(out))
    return out


def bench_fit(dev, rows, K):
    spec = WideSpec(F, K)
    ds = _data(dev, rows, K)
    fitter = WideFitter(spec, dev, FitOptions(reg_param=1e-3))
    res = fitter.fit(ds)
    ev = list(fitter._native.eval_seconds)
    out = {"rows": rows, "K": K, "touched": int(res.features.numel()), "seconds": res.seconds, "iters": res.iters,
           "evals": res.evals, "reason": res.reason, "objective": res.objective, "log_loss": res.log_loss,
           "pass_seconds": res.pass_seconds, "eval_seconds_total": sum(ev)}
    print(json.dumps(out))
    return out


def bench_weights(dev, rows, K, repeats, cv_folds):
    spec = WideSpec(F, K)
    ds = _data(dev, rows, K)
    w = spec.init("random", seed=1, scale=0.05).to(dev)
    g = torch.Generator().manual_seed(0)
    wts = FitWeights(torch.rand(rows, generator=g) * 2, 0.5 + torch.rand(max(K, 2), generator=g),
                     torch.randint(0, 5, (rows,), generator=g).to(torch.uint8), 0)
    fitter = WideFitter(spec, dev)
    st = stream_handle(dev)
    fitter.loss_grad(ds, w, weights=wts)  # loads the dataset, copies the weight streams, warms up
    data, nat = fitter._data, fitter._native
    checked = [_Weights(spec, ds, FitWeights(wts.sample_weight, wts.class_weight, wts.fold, k)) for k in (0, 1)]
    plain, weighted, switch = [], [], []
    for i in range(repeats):
        nat.set_weights(stream=st)
        plain.append(nat.stage_ms(False, st))
        switch.append(_event_ms(lambda: fitter._apply_weights(data, checked[i % 2])))
        weighted.append(nat.stage_ms(False, st))
    med = lambda runs: [_med([r[i] for r in runs]) for i in range(3)]  # noqa: E731
    tot = sorted(sum(r) for r in plain)
    out = {"rows": rows, "K": K, "plain_ms": med(plain), "weighted_ms": med(weighted),
           "plain_eval_ms": _med(tot), "plain_eval_spread_ms": tot[-1] - tot[0],
           "weighted_eval_ms": _med([sum(r) for r in weighted]), "fold_switch_ms": _med(switch)}
    if cv_folds:
        cv = cross_validate(spec, ds, [1e-4, 1e-3, 1e-2], folds=cv_folds, device=dev, opts=FitOptions(max_iter=10))
        out.update(cv_folds=cv_folds, cv_seconds=cv.seconds, cv_means=cv.means)
    print(json.dumps(out))
    return out


def bench_many(dev, rows, K, repeats):
    spec = WideSpec(F, K)
    ds = _data(dev, rows, K)
    g = torch.Generator().manual_seed(0)
    shared = FitWeights(torch.rand(rows, generator=g) * 2, 0.5 + torch.rand(max(K, 2), generator=g),
                        torch.randint(0, 5, (rows,), generator=g).to(torch.uint8))
    fitter = WideFitter(spec, dev)
    st, nat = stream_handle(dev), fitter._native
    slots = fitter.many_capacity
    one = FitWeights(shared.sample_weight, shared.class_weight, shared.fold, 0)
    w = spec.init("random", seed=1, scale=0.05).to(dev)
    fitter.loss_grad(ds, w, weights=one)  # loads the dataset, applies the weights, warms up
    out = {"rows": rows, "K": K, "KP": spec.KP, "slots": slots, "eval": []}
    for M in sorted({1, max(1, slots // 2), slots}):
        ws = w.repeat(M, 1)
        holds = [m % 5 for m in range(M)]
        fitter.loss_grad_many(ds, ws, shared, holds)
        many, plain = [], []
        for _ in range(repeats):
            fitter.loss_grad_many(ds, ws, shared, holds)
            many.append(nat.many_round_seconds[0] * 1e3)
            plain.append(M * sum(nat.stage_ms(True, st)))
        out["eval"].append({"models": M, "many_ms": _med(many), "plain_ms": _med(plain),
                            "many_spread_ms": max(many) - min(many)})
        del ws
    regs, kw = [1e-4, 1e-3, 1e-2, 1e-1], dict(folds=5, device=dev, opts=FitOptions(max_iter=10))
    cross_validate(spec, ds, regs[:1], batch=5, **kw)  # warm-up of both paths' first touches
    seq, bat = [], []
    for _ in range(max(1, repeats // 2)):
        seq.append(cross_validate(spec, ds, regs, **kw))
        bat.append(cross_validate(spec, ds, regs, batch=20, **kw))
    out.update(cv_sequential_s=_med([c.seconds for c in seq]), cv_batched_s=_med([c.seconds for c in bat]),
               cv_best=(seq[0].best_reg_param, bat[0].best_reg_param),
               cv_loss_gap=max(abs(a - b) for a, b in zip(sum(seq[0].losses, []), sum(bat[0].losses, []))))
    print(json.dumps(out))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="eval,chunk,setup,fit")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the results as JSON")
    ap.add_argument("--weights", action="store_true", help="the weighted evaluation against the plain one")
    ap.add_argument("--cv", type=int, default=0, help="with --weights: folds of a timed cross_validate")
    ap.add_argument("--many", action="store_true", help="many fits per read of the rows against the plain evaluations")
    ap.add_argument("--classes", default="6,1", help="with --many: class counts to measure")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_wide_fit: no GPU -- not measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    print(f"default col_chunk {DEFAULT_COL_CHUNK}")
    res = {}
    if a.many:
        res["many"] = [bench_many(dev, a.rows, int(K), a.repeats) for K in a.classes.split(",")]
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return 0
    if a.weights:
        res["weights"] = [bench_weights(dev, a.rows, K, a.repeats, a.cv) for K in (6, 1)]
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return 0
    for what in a.what.split(","):
        if what == "eval":
            res[what] = [bench_eval(dev, a.rows, K, a.repeats) for K in (6, 1)]
        elif what == "chunk":
            res[what] = [bench_chunk(dev, a.rows, K, a.repeats) for K in (6, 1)]
        elif what == "setup":
            res[what] = [bench_setup(dev, a.rows, K) for K in (6, 1)]
        elif what == "fit":
            res[what] = [bench_fit(dev, a.rows, K) for K in (6, 1)]
        else:
            ap.error(f"unknown measurement {what!r}")
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

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

Usage: python tools/bench_wide_fit.py [--what eval,chunk,setup,fit] [--rows N] [--out FILE.json]
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
from psx.ops.fit import FitOptions  # noqa: E402
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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="eval,chunk,setup,fit")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the results as JSON")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_wide_fit: no GPU -- not measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    print(f"default col_chunk {DEFAULT_COL_CHUNK}")
    res = {}
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

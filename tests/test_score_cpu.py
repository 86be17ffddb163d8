"""Scoring on the CPU: the Scorer's PyTorch path against the float64 oracle, its
errors, checkpoints written by real (short) runs, and the predict command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _score_cases import dense_case, wide_case, with_bad_labels
from psx.models.logreg import ModelSpec
from psx.models.wide import WideSpec
from psx.ops.lr import SolverOptions
from psx.ops.score import Scorer, ScoreResult
from psx.runtime.config import PSConfig
from psx.runtime.engine import LocalEngine
from psx.utils.checkpoint import CKPT_NAME
from psx.utils.data import load_any, synth_finefood, synth_sparse
from psx.utils.metrics import metrics_from_confusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "golden", "sample_input_data.csv")


def _same(a: ScoreResult, b: ScoreResult):
    for name in ("pred", "proba", "nll", "confusion"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert torch.equal(x.cpu().view(torch.int32) if x.dtype == torch.float32 else x.cpu(),
                               y.cpu().view(torch.int32) if y.dtype == torch.float32 else y.cpu()), name
    assert (a.rows, a.rows_out_of_range, a.log_loss, a.f1, a.accuracy) == \
        (b.rows, b.rows_out_of_range, b.log_loss, b.f1, b.accuracy)


# ---- the CPU path against the oracle ---------------------------------------------
@pytest.mark.parametrize("make", [lambda: dense_case(300, 6, 97), lambda: wide_case(6, 17), lambda: wide_case(1, 17)],
                         ids=["dense", "wide", "sigmoid"])
def test_cpu_scorer_meets_the_oracle_bounds(make):
    case = make()
    sc = Scorer(case.spec, case.w, "cpu")
    res = sc.score(case.ds, proba=True)
    case.check(res, "cpu")
    # labels -1, K and 99 among valid ones: NaN exactly there, counted, left out of log_loss
    bad = with_bad_labels(case)
    rb = sc.score(bad.ds, proba=True)
    bad.check(rb, "cpu bad labels")
    assert rb.rows_out_of_range == (0 if case.spec.K == 1 else 3)
    # without labels: no loss, the same predictions and probabilities bit for bit
    rn = sc.score(case.ds, labels=False, proba=True)
    case.check(rn, "cpu no labels", labels=False)
    assert torch.equal(rn.pred, res.pred) and torch.equal(rn.proba.view(torch.int32), res.proba.view(torch.int32))
    assert torch.equal(sc.predict(case.ds), res.pred)
    assert torch.equal(sc.predict_proba(case.ds).view(torch.int32), res.proba.view(torch.int32))
    # chunked (the CPU matrix product rounds differently per batch shape: the bounds, not the bits)
    for chunk in (1, 33):
        rc = sc.score(case.ds, proba=True, chunk_rows=chunk)
        case.check(rc, f"cpu chunk {chunk}")
        assert torch.equal(rc.confusion, res.confusion)


@pytest.mark.parametrize("make,K", [(lambda: dense_case(300, 6, 33, zero_w=True), 6),
                                    (lambda: wide_case(6, 17, zero_w=True), 6),
                                    (lambda: wide_case(1, 17, zero_w=True), 1)], ids=["dense", "wide", "sigmoid"])
def test_cpu_zero_weights(make, K):
    case = make()
    res = Scorer(case.spec, case.w, "cpu").score(case.ds, proba=True)
    case.check(res, "cpu w=0")
    C = case.spec.eval_classes
    assert int(res.pred.abs().sum()) == 0  # the lowest class wins the tie; binary: z > 0 is false
    assert float((res.proba - 1.0 / C).abs().max()) <= 1e-6
    assert float((res.nll - np.log(C)).abs().max()) <= 2 * 2e-5 + 1e-6


def test_value_errors_name_both_numbers():
    d, w = dense_case(99, 2, 5), wide_case(3, 5)
    sd, sw = Scorer(d.spec, d.w, "cpu"), Scorer(w.spec, w.w, "cpu")
    with pytest.raises(ValueError, match=r"300.*99|99.*300"):  # width mismatch
        sd.score(dense_case(300, 2, 5).ds)
    wider = wide_case(3, 5, F=6000)
    with pytest.raises(ValueError, match=r"6000.*5000"):  # more features than the model
        sw.score(wider.ds)
    with pytest.raises(ValueError, match="SparseDataset"):  # wrong dataset kind
        sw.score(d.ds)
    with pytest.raises(ValueError, match="Dataset"):
        sd.score(w.ds)
    with pytest.raises(ValueError, match=str(d.spec.P)):
        Scorer(d.spec, torch.zeros(7), "cpu")
    one = ModelSpec(10, 1)  # the one-logit model is the wide family's
    with pytest.raises(ValueError, match="1 classes"):
        Scorer(one, torch.zeros(one.P), "cpu")

    class _KeyRangeRank:  # what a key-range engine exposes: no whole server model
        pass

    with pytest.raises(ValueError, match="slice"):
        Scorer.from_engine(_KeyRangeRank())


# ---- checkpoints of real runs --------------------------------------------------------
def _cfg(tmp, **kw):
    base = dict(num_workers=2, consistency_model=0, producer_time_per_event=0, stream_mode="per_iter",
                rows_per_iter=64, epochs=50, max_iters=3, min_buffer_size=64, max_buffer_size=256, init="random",
                checkpoint_dir=str(tmp), checkpoint_every=3)
    base.update(kw)
    return PSConfig(**base)


def _sparse(rows, labels, seed):
    return synth_sparse(rows, num_features=1500, labels=labels, nnz_mean=20, max_nnz=48, seed=seed, vocab=6000,
                        class_vocab=200, signal=0.3)


def _run(kind, tmp):
    if kind == "dense":
        train, test = synth_finefood(1500, num_features=128, seed=0), synth_finefood(200, num_features=128, seed=1)
        eng = LocalEngine(_cfg(tmp), "cpu", train=train, test=test)
    else:
        lab = "binary" if kind == "sigmoid" else "finefood"
        train, test = _sparse(800, lab, 0), _sparse(150, lab, 3)
        eng = LocalEngine(_cfg(tmp, sigmoid=kind == "sigmoid", solver=SolverOptions(zero_const=False)), "cpu",
                          train=train, test=test)
    out = eng.run()
    assert out["rounds"] == 3
    return eng, test


@pytest.mark.parametrize("kind", ["dense", "wide", "sigmoid"])
def test_from_checkpoint_round_trips(kind, tmp_path):
    eng, test = _run(kind, tmp_path)
    live = Scorer.from_engine(eng)
    assert live.spec == eng.spec and isinstance(live.spec, ModelSpec if kind == "dense" else WideSpec)
    assert live.spec.K == (1 if kind == "sigmoid" else 6)
    want = live.score(test, proba=True)
    assert want.rows == test.rows and 0.0 < want.log_loss < 10.0
    by_dir = Scorer.from_checkpoint(str(tmp_path), "cpu")
    by_file = Scorer.from_checkpoint(str(tmp_path / CKPT_NAME), "cpu")
    for sc in (by_dir, by_file):
        assert sc.spec == eng.spec and torch.equal(sc.w, eng.server.w)
        _same(sc.score(test, proba=True), want)
    # the same counts as the training-time evaluation of these weights
    conf = torch.zeros(256, dtype=torch.int32)
    if kind == "dense":
        eng.evalset.confusion_async(None, eng.server.w, conf)
    else:
        conf = eng.evalset.confusion_cpu(eng.server.w)
    C = eng.spec.eval_classes
    assert torch.equal(want.confusion, conf.view(16, 16)[:C, :C].long())


def test_from_checkpoint_reference_layout_only(tmp_path):
    eng, test = _run("dense", tmp_path)
    path = str(tmp_path / CKPT_NAME)
    st = torch.load(path, map_location="cpu", weights_only=True)
    assert "w_reference_layout" in st
    del st["w"]
    stripped = str(tmp_path / "stripped.ckpt")
    torch.save(st, stripped)
    sc = Scorer.from_checkpoint(stripped, "cpu")
    assert torch.equal(sc.w, eng.server.w)
    _same(sc.score(test, proba=True), Scorer.from_engine(eng).score(test, proba=True))


# ---- the command line --------------------------------------------------------------------
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "psx.apps.predict", *args], capture_output=True, text=True, env=env,
                          cwd=ROOT, timeout=300)


def test_cli_exit_codes():
    r = _cli("-h")
    assert r.returncode == 0 and "--checkpoint_dir" in r.stdout
    assert _cli("--checkpoint_dir", "x", "--data", "y", "stray").returncode == 2
    assert _cli("--no_such_flag").returncode == 2
    assert _cli("--data", "y").returncode == 2  # the checkpoint is required


def test_cli_on_the_mock_data(tmp_path):
    cfg = PSConfig(train_path=MOCK, test_path=MOCK, num_workers=2, consistency_model=0, producer_time_per_event=0,
                   max_iters=3, checkpoint_dir=str(tmp_path), checkpoint_every=3)
    LocalEngine(cfg, "cpu").run()
    ds = load_any(MOCK)
    res = Scorer.from_checkpoint(str(tmp_path), "cpu").score(ds, proba=True)
    out = str(tmp_path / "preds.csv")
    r = _cli("--checkpoint_dir", str(tmp_path), "--data", MOCK, "--out", out, "--proba", "--device", "cpu")
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["rows"] == ds.rows and line["rows_out_of_range"] == 0
    assert (line["model"], line["num_features"], line["num_classes"], line["device"]) == ("dense", 99, 2, "cpu")
    assert line["rows_per_s"] > 0
    f1, acc = metrics_from_confusion(line["confusion"])
    assert line["f1"] == f1 and line["accuracy"] == acc
    assert line["confusion"] == res.confusion.tolist() and line["log_loss"] == res.log_loss
    rows = open(out).read().splitlines()
    assert rows[0] == "row,pred,label,nll,p0,p1" and len(rows) == 1 + ds.rows
    got = np.array([[float(v) for v in ln.split(",")] for ln in rows[1:]])
    assert got[:, 0].tolist() == list(range(ds.rows))
    assert got[:, 1].tolist() == res.pred.tolist() and got[:, 2].tolist() == ds.y.tolist()
    # the printed precision: %.6g
    want = np.concatenate([res.nll.double().numpy()[:, None], res.proba.double().numpy()], 1)
    assert np.array_equal(got[:, 3:], np.array([[float("%.6g" % v) for v in row] for row in want]))
    # --ignore_labels: no metrics, no nll / label columns
    out2 = str(tmp_path / "preds2.csv")
    r = _cli("--checkpoint_dir", str(tmp_path), "--data", MOCK, "--out", out2, "--ignore_labels", "--device", "cpu",
             "--chunk_rows", "7")
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert not {"accuracy", "f1", "log_loss", "confusion"} & set(line) and line["rows"] == ds.rows
    rows = open(out2).read().splitlines()
    assert rows[0] == "row,pred" and len(rows) == 1 + ds.rows
    assert [int(ln.split(",")[1]) for ln in rows[1:]] == res.pred.tolist()

"""The score histogram and its ranking metrics on the CPU: the cap on unsure entries of every
case (from the oracle alone), the Scorer's PyTorch path against the float64 oracle of
_hist_cases.py, the metric functions on hand-made tables and against sklearn, a planted case,
the predict command line and the errors."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _hist_cases as H
from _hist_cases import hist_oracle, with_bad_labels
from psx.ops.score import Scorer
from psx.utils import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FIELDS = ("hist", "auc", "auc_resolution", "auc_macro", "auc_weighted", "ap", "ap_macro", "ece")


def _dense_ids(v):
    return "-".join(str(x) for x in v)


# ---- the condition on the inputs ---------------------------------------------------
@pytest.mark.parametrize("fkts", sorted(set(H.DENSE_TABLE + H.DENSE_GPU)), ids=_dense_ids)
def test_dense_unsure_cap(fkts):
    F, K, T, scale = fkts
    o = hist_oracle(H.dense(F, K, T, scale))
    print(f"dense {fkts}: unsure {100 * o.unsure_share:.2f} % of {o.entries}")
    assert o.unsure_share <= H.MAX_UNSURE


@pytest.mark.parametrize("kts", H.WIDE_GPU, ids=_dense_ids)
def test_wide_unsure_cap(kts):
    K, T, scale = kts
    o = hist_oracle(H.wide(K, T, scale))
    print(f"wide {kts}: unsure {100 * o.unsure_share:.2f} % of {o.entries}")
    assert o.unsure_share <= H.MAX_UNSURE


def test_zero_weight_cases_are_exact():
    for F, K, T in H.DENSE_ZERO:
        o = hist_oracle(H.dense(F, K, T, 1.0, True))
        assert o.unsure_share == 0 and torch.equal(o.lo, o.hi)
    for K, T in H.WIDE_ZERO:
        o = hist_oracle(H.wide(K, T, 1.0, True))
        assert o.unsure_share == 0 and torch.equal(o.lo, o.hi)


def test_both_end_bins_fill_at_scale_20():
    o = hist_oracle(H.dense(512, 8, 700, 20.0))
    assert int(o.lo[:, :, 0].sum()) > 0 and int(o.lo[:, :, H.NB - 1].sum()) > 0


# ---- the CPU path against the oracle -----------------------------------------------
CPU_CASES = {
    "dense-100-2-229": lambda: H.dense(100, 2, 229),
    "dense-300-5-33": lambda: H.dense(300, 5, 33),
    "dense-1024-6-229": lambda: H.dense(1024, 6, 229),
    "dense-2000-16-229": lambda: H.dense(2000, 16, 229),
    "dense-512-8-700-s20": lambda: H.dense(512, 8, 700, 20.0),
    "dense-300-5-2000-s100": lambda: H.dense(300, 5, 2000, 100.0),
    "dense-zero-6": lambda: H.dense(100, 6, 64, 1.0, True),
    "dense-zero-2": lambda: H.dense(100, 2, 64, 1.0, True),
    "wide-6": lambda: H.wide(6, 400),
    "wide-16": lambda: H.wide(16, 400),
    "wide-6-s30": lambda: H.wide(6, 400, 30.0),
    "sigmoid": lambda: H.wide(1, 400),
    "wide-zero": lambda: H.wide(6, 400, 1.0, True),
    "sigmoid-zero": lambda: H.wide(1, 400, 1.0, True),
}


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_cpu_table_between_the_oracle_bounds(name):
    case = CPU_CASES[name]()
    res = Scorer(case.spec, case.w, "cpu").score(case.ds, curves=True)
    o = hist_oracle(case)
    o.check(res.hist, f"cpu {name}")
    K = case.spec.K
    y = case.ds.y.long()
    for c in range(o.Ch):  # the side totals, spelled out
        assert int(res.hist[c, 1].sum()) == int((y > 0).sum() if K == 1 else (y == c).sum())
        assert int(res.hist[c].sum()) == int(y.numel() if K == 1 else ((y >= 0) & (y < K)).sum())
    assert res.auc.shape == (o.Ch,) and res.auc_resolution.shape == (o.Ch,) and res.ap.shape == (o.Ch,)


def test_cpu_zero_weights_fill_one_bin_per_class():
    for K, b in ((2, 256), (6, 256 + round(-16 * np.log(5)))):  # l = 0 and l = -log(K - 1), inside a bin
        case = H.dense(100, K, 64, 1.0, True)
        res = Scorer(case.spec, case.w, "cpu").score(case.ds, curves=True)
        assert int(res.hist[:, :, b].sum()) == 64 * K == int(res.hist.sum())
        assert np.allclose(res.auc, 0.5) and np.allclose(res.auc_resolution, 0.5)


@pytest.mark.parametrize("name", ["dense-300-5-33", "wide-6", "sigmoid"])
def test_cpu_chunks_add_up(name):
    case = CPU_CASES[name]()
    sc = Scorer(case.spec, case.w, "cpu")
    ref = sc.score(case.ds, curves=True)
    for chunk in (7, 64, case.ds.rows):
        got = sc.score(case.ds, curves=True, chunk_rows=chunk)
        assert torch.equal(got.hist, ref.hist), chunk
        assert np.array_equal(got.auc, ref.auc, equal_nan=True) and got.ece == ref.ece


@pytest.mark.parametrize("name", ["dense-300-5-33", "wide-6", "sigmoid"])
def test_cpu_bad_labels_enter_no_cell(name):
    base = CPU_CASES[name]()
    case = with_bad_labels(base)  # -1, K and 99 at rows 1, 3 and the last
    res = Scorer(case.spec, case.w, "cpu").score(case.ds, curves=True)
    o = hist_oracle(case)
    o.check(res.hist, f"cpu bad labels {name}")
    K, T = case.spec.K, case.ds.rows
    if K == 1:  # the binary model knows no label out of range: -1 is a negative, K and 99 positives
        assert int(res.hist.sum()) == T and res.rows_out_of_range == 0
    else:
        assert int(res.hist.sum()) == (T - 3) * K and res.rows_out_of_range == 3


def test_plain_score_has_none_in_every_new_field():
    case = H.dense(300, 5, 33)
    sc = Scorer(case.spec, case.w, "cpu")
    for kw in (dict(), dict(proba=True), dict(labels=False), dict(curves=False)):
        res = sc.score(case.ds, **kw)
        assert all(getattr(res, f) is None for f in NEW_FIELDS), kw
    with pytest.raises(ValueError, match="labels"):
        sc.score(case.ds, labels=False, curves=True)


def test_curves_leave_the_other_outputs_alone():
    case = H.dense(300, 5, 33)
    sc = Scorer(case.spec, case.w, "cpu")
    a, b = sc.score(case.ds, proba=True), sc.score(case.ds, proba=True, curves=True)
    for f in ("pred", "proba", "nll", "confusion"):
        x, y = getattr(a, f), getattr(b, f)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), f
    assert (a.log_loss, a.f1, a.accuracy, a.rows_out_of_range) == (b.log_loss, b.f1, b.accuracy, b.rows_out_of_range)


# ---- the metric functions on hand-made tables ------------------------------------------
def _table(Ch=1):
    return np.zeros((Ch, 2, H.NB), dtype=np.int64)


def test_separated_table():
    h = _table()
    h[0, 0, 10], h[0, 0, 200], h[0, 1, 201], h[0, 1, 500] = 5, 2, 3, 4
    auc, res = M.roc_auc(h)
    assert auc[0] == 1.0 and res[0] == 0.0
    assert M.average_precision(h)[0] == 1.0 and M.ks_statistic(h)[0] == 1.0
    fpr, tpr, thr = M.roc_curve(h, 0)
    assert len(fpr) == len(tpr) == len(thr) == H.NB + 1
    assert (fpr[0], tpr[0], fpr[-1], tpr[-1]) == (0.0, 0.0, 1.0, 1.0)
    assert np.all(np.diff(fpr) >= 0) and np.all(np.diff(tpr) >= 0) and np.all(np.diff(thr) < 0)
    prec, rec, _ = M.pr_curve(h, 0)
    assert prec[0] == 1.0 and rec[0] == 0.0 and rec[-1] == 1.0 and prec[-1] == 7 / 14
    h[0] = h[0, ::-1].copy()  # the sides swapped: every pair the wrong way round
    assert M.roc_auc(h)[0][0] == 0.0


def test_one_bin_table():
    h = _table()
    h[0, 0, 300], h[0, 1, 300] = 6, 2
    auc, res = M.roc_auc(h)
    assert auc[0] == 0.5 and res[0] == 0.5
    assert M.average_precision(h)[0] == 0.25 and M.ks_statistic(h)[0] == 0.0
    pred, obs, n = M.calibration(h, 0)
    assert pred.shape == obs.shape == n.shape == (1,)
    assert pred[0] == 1 / (1 + np.exp(-(300 - 256) / 16)) and obs[0] == 0.25 and n[0] == 8
    assert M.ece(h)[0] == abs(0.25 - pred[0])


def test_class_without_positives_is_left_out():
    h = _table(3)
    h[0, 0, 100], h[0, 1, 300] = 4, 4  # AUC 1
    h[1, 0, 100] = 8  # no positive rows
    h[2, 0, 200], h[2, 1, 200] = 6, 2  # AUC 0.5
    auc, res = M.roc_auc(h)
    assert auc[0] == 1.0 and np.isnan(auc[1]) and np.isnan(res[1]) and auc[2] == 0.5
    macro, weighted = M.auc_summary(h)
    assert macro == 0.75 and weighted == (4 * 1.0 + 2 * 0.5) / 6
    assert np.isnan(M.average_precision(h)[1]) and np.isnan(M.ks_statistic(h)[1])
    only_pos = _table()
    only_pos[0, 1, 7] = 3
    assert np.isnan(M.roc_auc(only_pos)[0][0]) and all(np.isnan(v) for v in M.auc_summary(only_pos))
    assert np.isnan(M.ece(_table())[0])


def test_calibrated_table_has_small_ece():
    centres = M.bin_centres()
    p = 1 / (1 + np.exp(-centres))
    h = _table()
    n = 10 ** 6
    h[0, 1] = np.round(n * p)
    h[0, 0] = n - h[0, 1]
    assert M.ece(h)[0] <= 1e-6  # the rounding of the counts
    h[0, 0], h[0, 1] = h[0, 1].copy(), h[0, 0].copy()
    assert M.ece(h)[0] > 0.1


def test_metrics_equal_sklearn_on_the_bin_centres():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    h = rng.integers(0, 4, (4, 2, H.NB)) * (rng.random((4, 2, H.NB)) < 0.3)
    h[:, 1, 300:] += rng.integers(0, 3, (4, 212))  # positives lean high
    centres = M.bin_centres()
    auc, ap = M.roc_auc(h)[0], M.average_precision(h)
    for c in range(4):
        s = np.concatenate([np.repeat(centres, h[c, 0]), np.repeat(centres, h[c, 1])])
        y = np.concatenate([np.zeros(h[c, 0].sum()), np.ones(h[c, 1].sum())])
        assert abs(auc[c] - sk.roc_auc_score(y, s)) <= 1e-12
        assert abs(ap[c] - sk.average_precision_score(y, s)) <= 1e-12
        fpr, tpr, _ = M.roc_curve(h, c)
        area = float((np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2).sum())
        assert abs(area - auc[c]) <= 1e-12  # the curve's area is the binned AUC


# ---- a planted case ----------------------------------------------------------------------
def test_planted_auc_within_its_bound():
    case = H.planted()
    res = Scorer(case.spec, case.w, "cpu").score(case.ds, curves=True)
    hist_oracle(case).check(res.hist, "cpu planted")
    exact = H.check_planted_auc(res, case, "cpu planted")
    sk = pytest.importorskip("sklearn.metrics")
    o = hist_oracle(case)
    y = case.ds.y.numpy()
    for c in range(o.Ch):  # the oracle's own pair count against sklearn
        assert abs(exact[c] - sk.roc_auc_score(y == c, o.l64[:, c].numpy())) <= 1e-12
    assert res.auc_macro == pytest.approx(float(np.mean(res.auc)), abs=1e-15)
    P = res.hist[:, 1].sum(1).numpy()
    assert res.auc_weighted == pytest.approx(float((res.auc * P).sum() / P.sum()), abs=1e-15)
    assert res.ap_macro == pytest.approx(float(np.mean(res.ap)), abs=1e-15)
    assert 0.0 <= res.ece < 0.1  # labels drawn from the model's own probabilities: calibrated


# ---- the command line ---------------------------------------------------------------------
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "psx.apps.predict", *args], capture_output=True, text=True, env=env,
                          cwd=ROOT, timeout=300)


def _checkpoint(kind, tmp):
    from psx.ops.lr import SolverOptions
    from psx.runtime.config import PSConfig
    from psx.runtime.engine import LocalEngine
    from psx.utils.data import synth_finefood, synth_sparse

    base = dict(num_workers=2, consistency_model=0, producer_time_per_event=0, stream_mode="per_iter",
                rows_per_iter=64, epochs=50, max_iters=3, min_buffer_size=64, max_buffer_size=256, init="random",
                checkpoint_dir=str(tmp), checkpoint_every=3)
    if kind == "dense":
        train, test = synth_finefood(1500, num_features=128, seed=0), synth_finefood(200, num_features=128, seed=1)
        eng = LocalEngine(PSConfig(**base), "cpu", train=train, test=test)
    else:
        def sp(rows, seed):
            return synth_sparse(rows, num_features=1500, labels="binary", nnz_mean=20, max_nnz=48, seed=seed,
                                vocab=6000, class_vocab=200, signal=0.3)

        train, test = sp(800, 0), sp(150, 3)
        eng = LocalEngine(PSConfig(**base, sigmoid=True, solver=SolverOptions(zero_const=False)), "cpu",
                          train=train, test=test)
    assert eng.run()["rounds"] == 3
    return test


def _write_data(kind, test, path):
    with open(path, "w") as f:
        if kind == "dense":
            for r in range(test.rows):
                f.write(",".join(repr(float(v)) for v in test.X[r, : test.num_features].float().tolist()))
                f.write(f",{int(test.y[r])}\n")
        else:
            for r in range(test.rows):
                a, b = int(test.indptr[r]), int(test.indptr[r + 1])
                # LIBSVM feature ids are 1-based
                feats = " ".join(f"{int(i) + 1}:{float(v)!r}" for i, v in zip(test.idx[a:b], test.val[a:b].float()))
                f.write(f"{int(test.y[r])} {feats}\n")


@pytest.mark.parametrize("kind", ["dense", "sigmoid"])
def test_cli_curves(kind, tmp_path):
    test = _checkpoint(kind, tmp_path)
    data = str(tmp_path / ("test.csv" if kind == "dense" else "test.libsvm"))
    _write_data(kind, test, data)
    common = ("--checkpoint_dir", str(tmp_path), "--data", data, "--device", "cpu")
    if kind == "dense":
        common += ("--header", "no")
    plain = _cli(*common)
    assert plain.returncode == 0, plain.stderr
    out = str(tmp_path / "curves.json")
    r = _cli(*common, "--curves", "--curves_out", out)
    assert r.returncode == 0, r.stderr
    lines, before = r.stdout.strip().splitlines(), plain.stdout.strip().splitlines()
    assert len(before) == 1 and len(lines) == 2
    a, b = json.loads(before[0]), json.loads(lines[0])
    a.pop("rows_per_s"), b.pop("rows_per_s")  # a timing
    assert a == b and list(json.loads(before[0])) == list(json.loads(lines[0]))  # the line of today, then the new one
    new = json.loads(lines[1])
    assert list(new) == ["auc_macro", "auc_weighted", "ap_macro", "ece", "auc", "auc_resolution"]
    from psx.utils.data import load_any, load_libsvm

    sc = Scorer.from_checkpoint(str(tmp_path), "cpu")
    ds = load_any(data, header="no") if kind == "dense" else load_libsvm(data, num_features=sc.spec.F)
    res = sc.score(ds, curves=True)
    Ch = 6 if kind == "dense" else 1
    assert tuple(res.hist.shape) == (Ch, 2, H.NB) and int(res.hist.sum()) == ds.rows * Ch
    assert new["auc_macro"] == res.auc_macro and new["ece"] == res.ece and new["ap_macro"] == res.ap_macro
    assert new["auc_weighted"] == res.auc_weighted and len(new["auc"]) == len(new["auc_resolution"]) == Ch
    assert [v for v in new["auc"] if v is not None] == [float(v) for v in res.auc if v == v]
    doc = json.load(open(out))
    assert doc["hist"] == res.hist.tolist() and doc["bins"] == H.NB and doc["auc"] == new["auc"]
    assert {"ap", "ks", "ece_per_class", "auc_resolution", "bins_per_unit_log_odds"} <= set(doc)
    # curves need labels
    r = _cli(*common, "--curves", "--ignore_labels")
    assert r.returncode == 2 and "labels" in r.stderr
    r = _cli(*common, "--curves_out", out, "--ignore_labels")
    assert r.returncode == 2

"""Full-batch fit: the float64 oracle (fit_reference), the CPU trainer, checkpoints,
the command line, validation and the error messages.  No GPU."""
import json
import os
import subprocess
import sys

import pytest
import torch

from _fit_cases import CONVERGED, check_validation, converged_oracle, fit_case, rows64, warm_start
from psx.models.logreg import ModelSpec
from psx.models.reference import fit_reference, local_solve_reference
from psx.models.wide import WideSpec
from psx.ops.fit import BatchFitter, FitOptions, loss_grad
from psx.ops.score import Scorer
from psx.utils.data import Dataset, load_any

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "golden", "sample_input_data.csv")


# ---- 1. the oracle generalises local_solve_reference ---------------------------------------
@pytest.mark.parametrize("N,F,K,constant", [(200, 12, 4, False), (150, 9, 3, True)])
def test_fit_reference_is_local_solve_reference_without_a_penalty(N, F, K, constant):
    spec, ds, const = fit_case(N, F, K, seed=3)
    X, y = rows64(spec, ds)
    if not constant:
        X[:, const] = torch.randn(N, dtype=torch.float64).bfloat16().double()
    w0 = warm_start(spec)
    c0, b0 = spec.coef(w0), spec.intercept(w0)
    loc = local_solve_reference(X, y, c0, b0, iters=2, ls_max=4)
    fit = fit_reference(X, y, c0, b0, reg_param=0.0, max_iter=2, ls_max=4)
    assert fit.iters == loc.accepted and fit.evals == loc.evals and fit.ls_fail == loc.ls_fail
    assert fit.objective == loc.loss and fit.history[-1] == loc.loss
    assert torch.equal(fit.coef.float(), loc.coef) and torch.equal(fit.intercept.float(), loc.intercept)
    assert bool((fit.std == 0).any()) == constant


# ---- 2. the oracle against sklearn ---------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CONVERGED)))
def test_fit_reference_matches_sklearn(i):
    lm = pytest.importorskip("sklearn.linear_model")
    spec, ds, const, ref = converged_oracle(i)
    X, y = rows64(spec, ds)
    N = X.shape[0]
    live = ref.std > 0
    assert not bool(live[const]) and int((~live).sum()) == 1
    sk = lm.LogisticRegression(C=1.0 / (N * 0.1), solver="lbfgs", tol=1e-12, max_iter=20000)
    sk.fit((X[:, live] / ref.std[live]).numpy(), y.numpy())
    sk_coef = torch.from_numpy(sk.coef_)
    sk_b = torch.from_numpy(sk.intercept_)
    beta = (ref.coef * ref.std)[:, live]
    top = float(sk_coef.abs().max())
    dc = float((beta - sk_coef).abs().max())
    db = float((ref.intercept - (sk_b - sk_b.mean())).abs().max())
    print(f"case {CONVERGED[i]}: max |beta - sk| {dc:.3e} intercepts {db:.3e} (bound {1e-3 * top:.3e}), "
          f"iters {ref.iters} evals {ref.evals} reason {ref.reason}")
    assert dc <= 1e-3 * top
    assert db <= 1e-3 * max(top, float(sk_b.abs().max()))
    assert bool((ref.coef[:, const] == 0).all())


# ---- 3. history and the centring rule ------------------------------------------------------
def test_history_descends_and_centring_follows_the_penalty():
    spec, ds, _ = fit_case(300, 10, 4, seed=5)
    X, y = rows64(spec, ds)
    for lam in (0.0, 0.05):
        r = fit_reference(X, y, num_classes=4, reg_param=lam, max_iter=25)
        assert len(r.history) == r.iters + 1 and r.history[-1] == r.objective
        assert all(b <= a for a, b in zip(r.history, r.history[1:]))
        assert r.reason in ("tol", "max_iter", "line_search")
    w0 = warm_start(spec, scale=0.3)
    c0, b0 = spec.coef(w0).double(), spec.intercept(w0).double()
    assert float(c0.mean(0).abs().max()) > 1e-3  # the start is not centred
    pen = fit_reference(X, y, c0, b0, reg_param=0.05, max_iter=0)
    assert pen.reason == "max_iter" and pen.iters == 0 and pen.evals == 1
    live = pen.std > 0
    assert torch.allclose(pen.coef[:, live], c0[:, live], rtol=1e-12, atol=0)  # left as given
    assert float(pen.intercept.sum().abs()) < 1e-12  # intercepts: always centred
    free = fit_reference(X, y, c0, b0, reg_param=0.0, max_iter=0)
    assert float(free.coef.sum(0).abs().max()) < 1e-12
    assert torch.allclose(free.coef[:, live], (c0 - c0.mean(0, keepdim=True))[:, live], rtol=1e-9, atol=1e-15)
    # a penalised optimum is centred by itself
    _, _, _, conv = converged_oracle(0)
    beta = conv.coef * conv.std
    assert float(beta.sum(0).abs().max()) <= 1e-6 * float(beta.abs().max())


# ---- 4. CPU trainer, checkpoint, command line ----------------------------------------------
def test_cpu_trainer_is_the_oracle_and_round_trips(tmp_path):
    spec, ds, _ = fit_case(300, 10, 4, seed=6)
    X, y = rows64(spec, ds)
    opts = FitOptions(max_iter=15, reg_param=0.02)
    res = BatchFitter(spec, "cpu", opts).fit(ds)
    ref = fit_reference(X, y, num_classes=4, reg_param=0.02, max_iter=15)
    assert torch.equal(res.w, spec.pack(ref.coef, ref.intercept))
    assert (res.objective, res.log_loss, res.history) == (ref.objective, ref.log_loss, ref.history)
    assert (res.iters, res.evals, res.reason) == (ref.iters, ref.evals, ref.reason)
    assert res.log_loss < res.objective and res.seconds > 0 and res.pass_seconds > 0
    res.save(str(tmp_path))
    sc = Scorer.from_checkpoint(str(tmp_path), "cpu")
    assert torch.equal(sc.w, res.w)
    a, b = sc.score(ds), Scorer(spec, res.w, "cpu").score(ds)
    assert (a.log_loss, a.accuracy, a.f1) == (b.log_loss, b.accuracy, b.f1)
    st = torch.load(os.path.join(str(tmp_path), "server.ckpt"), weights_only=True)
    assert {"model", "num_features", "num_classes", "w", "w_reference_layout", "format", "fit"} <= set(st)
    assert st["fit"]["reg_param"] == 0.02 and st["fit"]["reason"] == ref.reason and st["fit"]["iters"] == ref.iters
    # one evaluation on the CPU: the float64 gradient in device layout
    w = warm_start(spec)
    loss, g = loss_grad(spec, ds, w, "cpu")
    assert g.shape == (spec.P,) and loss > 0


def _cli(mod, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", mod, *args], capture_output=True, text=True, env=env, cwd=ROOT,
                          timeout=300)


def test_cli_fits_writes_a_checkpoint_and_predict_reads_it(tmp_path):
    r = _cli("psx.apps.fit", "-h")
    assert r.returncode == 0 and "--reg_param" in r.stdout
    assert _cli("psx.apps.fit", "--train", MOCK, "stray").returncode == 2
    assert _cli("psx.apps.fit", "--test", MOCK).returncode == 2  # --train is required
    out = str(tmp_path / "ck")
    r = _cli("psx.apps.fit", "--train", MOCK, "--test", MOCK, "--reg_param", "0.1", "--max_iter", "20",
             "--checkpoint_dir", out, "--device", "cpu")
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    ds = load_any(MOCK)
    assert (line["rows"], line["features"], line["classes"]) == (ds.rows, 99, 2)
    assert {"iterations", "evaluations", "reason", "objective", "train_log_loss", "test_accuracy", "test_f1",
            "test_log_loss", "fit_seconds"} <= set(line)
    ref = BatchFitter(ModelSpec(99, 2), "cpu", FitOptions(max_iter=20, reg_param=0.1)).fit(ds)
    assert (line["iterations"], line["evaluations"], line["reason"]) == (ref.iters, ref.evals, ref.reason)
    assert line["objective"] == ref.objective and line["train_log_loss"] == ref.log_loss
    sc = Scorer.from_checkpoint(out, "cpu").score(ds)
    assert (line["test_accuracy"], line["test_f1"], line["test_log_loss"]) == (sc.accuracy, sc.f1, sc.log_loss)
    assert sc.accuracy > 0.6
    p = _cli("psx.apps.predict", "--checkpoint_dir", out, "--data", MOCK, "--device", "cpu")
    assert p.returncode == 0, p.stderr
    pl = json.loads(p.stdout.strip().splitlines()[-1])
    assert pl["accuracy"] == sc.accuracy and pl["log_loss"] == sc.log_loss
    # warm start from the checkpoint, hold-out validation
    r = _cli("psx.apps.fit", "--train", MOCK, "--reg_param", "0.1", "--max_iter", "3", "--init_checkpoint", out,
             "--valid_frac", "0.2", "--seed", "1", "--device", "cpu")
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["rows"] + line["valid_rows"] == ds.rows and "valid_log_loss" in line


# ---- 5. validation ---------------------------------------------------------------------------
def test_validation_keeps_the_best_iterate_and_stops_early():
    check_validation("cpu")


# ---- 6. errors ---------------------------------------------------------------------------------
def test_errors_are_value_errors():
    spec, ds, _ = fit_case(40, 10, 4, seed=9)
    f = BatchFitter(spec, "cpu")
    y = ds.y.clone()
    y[3] = 4
    with pytest.raises(ValueError, match=r"labels span \[0, 4\].*\[0, 4\)"):
        f.fit(Dataset(ds.X, y, 10))
    y[3] = -1
    with pytest.raises(ValueError, match="labels span"):
        f.fit(Dataset(ds.X, y, 10))
    with pytest.raises(ValueError, match="1 rows: at least 2"):
        f.fit(Dataset(ds.X[:1], ds.y[:1], 10))
    with pytest.raises(ValueError, match="reg_param must be >= 0"):
        BatchFitter(spec, "cpu", FitOptions(reg_param=-0.1))
    with pytest.raises(ValueError, match="10 features wide.*the model 11"):
        BatchFitter(ModelSpec(11, 4), "cpu").fit(ds)
    with pytest.raises(ValueError, match="padded 128.*padded 256"):
        BatchFitter(ModelSpec(200, 4), "cpu").fit(Dataset(ds.X, ds.y, 200))
    with pytest.raises(ValueError, match="dense model"):
        BatchFitter(WideSpec(5000, 4), "cpu")
    with pytest.raises(ValueError, match="weights in device layout"):
        f.fit(ds, w0=torch.zeros(7))
    # fp32 rows are fitted as bf16
    r32 = f.fit(Dataset(ds.X.float(), ds.y, 10))
    r16 = f.fit(ds)
    assert torch.equal(r32.w, r16.w)

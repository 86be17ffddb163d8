"""Multi-process parameter server on CPU (gloo): the RCCL schedules' logic with
world_size > 1, plus the ServerAppRunner/WorkerAppRunner pair as real processes."""
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, kw, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from psx.parallel.dist import DistEngine, init_from_env
    from psx.runtime.config import PSConfig
    from psx.utils.data import synth_finefood

    torch.set_num_threads(2)  # several ranks (and test workers) share the host's CPUs
    r, w, dev = init_from_env(cpu=True)
    kw = dict(kw)
    data = kw.pop("_data", "dense")
    count = kw.pop("_count_collectives", False)
    calls = {"all_reduce": 0, "item": 0}
    if count:  # every all_reduce issued by the engine after the bootstrap
        real = dist.all_reduce

        def counting(*a, **k):
            calls["all_reduce"] += 1
            return real(*a, **k)

        dist.all_reduce = counting
    cfg = PSConfig(**kw)
    if data == "wide":
        from psx.utils.data import synth_sparse

        train = synth_sparse(1500, num_features=3000, nnz_mean=20, max_nnz=48, seed=0, vocab=12000, class_vocab=200)
        test = synth_sparse(200, num_features=3000, nnz_mean=20, max_nnz=48, seed=1, vocab=12000, class_vocab=200)
    else:
        train, test = synth_finefood(1500, num_features=128, seed=0), synth_finefood(200, num_features=128, seed=1)
    eng = DistEngine(cfg, r, w, dev, train=train, test=test)
    out = eng.run()
    if count:
        dist.all_reduce = real
        out["all_reduce_calls"] = calls["all_reduce"]
    if r == 0:
        out_q.put((out, eng.server.w.cpu().numpy().copy()))  # by value: no fd the exiting rank owns
    dist.barrier()
    dist.destroy_process_group()


def _run(world, kw):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, kw, q)) for r in range(world)]
    for p in procs:
        p.start()
    out, w = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return out, torch.from_numpy(w)


BASE = dict(consistency_model=0, producer_time_per_event=0, stream_mode="per_iter", rows_per_iter=64, epochs=100,
            max_iters=5, num_workers=3)


def test_bsp_schedules_agree():
    ws = {}
    for sched in ("allreduce", "reduce_bcast", "sharded"):
        out, w = _run(3, dict(BASE, bsp_schedule=sched))
        assert out["rounds"] == 5 and out["updates"] == 15
        assert out["server_rows"] == 5  # allreduce: the last round's deferred server row is flushed
        ws[sched] = w
    assert torch.allclose(ws["allreduce"], ws["reduce_bcast"], atol=1e-5)
    assert torch.allclose(ws["allreduce"], ws["sharded"], atol=1e-5)


@pytest.mark.parametrize("sched", ["allreduce", "reduce_bcast", "sharded"])
def test_bsp_runs_until_exhausted_without_host_sync(sched):
    """CLI mode (max_iters = 0): the ranks agree to stop through the StopVote word
    (lagged read, no per-round all_reduce + .item()).  1500 rows over 3 ranks at 64
    rows per round: the 8th and last ingest happens in round 6 (startup ingest +
    rounds 0..6; the allreduce schedule ingests the next round's rows while its
    collective is in flight, so one round earlier), the vote is cast at the top
    of the next round and the ranks stop LAG rounds later.  The allreduce schedule
    issues exactly one collective per round (the delta payload carries the vote)."""
    from psx.parallel.dist import StopVote

    kw = dict(BASE, bsp_schedule=sched, max_iters=0, epochs=1, _count_collectives=True)
    out, w = _run(3, kw)
    voted = 6 if sched == "allreduce" else 7
    assert out["rounds"] == voted + StopVote.LAG
    if sched == "allreduce":
        # startup readiness polls aside, one all_reduce per round
        assert out["all_reduce_calls"] - out["rounds"] <= 2, out


def test_bsp_dedicated_server():
    out, w = _run(3, dict(BASE, bsp_schedule="reduce_bcast", server_colocated=False))
    assert out["updates"] == 10  # 2 worker ranks x 5 rounds


@pytest.mark.parametrize("c", [-1, 2, 10])
def test_async_dedicated_server(c):
    """SSP / ASP across processes through the ONE native server loop
    (csrc/runtime/async_server.h) over the host shared-memory transport."""
    out, w = _run(3, dict(BASE, consistency_model=c, max_iters=6))
    assert out["updates"] == 12 and out.get("native_server") is True
    assert out["host_us_per_update"] > 0
    if c > 0:
        assert out["max_vc_gap"] <= c + 1


@pytest.mark.parametrize("c", [1, 3])
def test_ssp_worker_stops_early(c):
    """SSP(D): a worker that finishes early is retired, so the others keep being
    released (its frozen clock must not hold min_clock back forever)."""
    out, w = _run(4, dict(BASE, consistency_model=c, max_iters=10, inject_worker_stop={0: 2}))
    assert out["updates"] == 2 + 2 * 10


def test_app_runners_as_processes(tmp_path):
    mock = os.path.join(ROOT, "tests", "golden", "sample_input_data.csv")  # the reference's mock data set
    port = str(_free_port())
    env = dict(os.environ, PYTHONPATH=ROOT)
    srv = subprocess.Popen([sys.executable, "-m", "psx.apps.server_app_runner", "-training", mock, "-test", mock,
                            "-c", "0", "-p", "0", "--num_workers", "2", "--device", "cpu", "--max_iters", "4",
                            "--master_port", port, "-l"], cwd=tmp_path, env=env)
    wk = subprocess.run([sys.executable, "-m", "psx.apps.worker_app_runner", "-test", mock, "--num_workers", "2",
                         "--device", "cpu", "--master_port", port, "-min", "8", "-max", "64"], cwd=tmp_path, env=env,
                        timeout=240)
    assert wk.returncode == 0
    assert srv.wait(timeout=120) == 0
    wl = (tmp_path / "logs-worker.csv").read_text().splitlines()
    assert wl[0].endswith("numTuplesSeen") and len(wl) == 1 + 8
    assert len((tmp_path / "logs-server.csv").read_text().splitlines()) == 1 + 4


@pytest.mark.parametrize("args,code", [(["-h"], 0), (["stray"], 2), (["-c", "-2"], 2), (["--bogus"], 2)])
def test_cli_exit_codes(args, code):
    r = subprocess.run([sys.executable, "-m", "psx.apps.server_app_runner"] + args, cwd=ROOT, capture_output=True,
                       text=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == code, r.stderr
    if code in (0, 2) and args != ["-c", "-2"]:
        assert "-training" in (r.stdout + r.stderr)


def test_worker_cli_help():
    r = subprocess.run([sys.executable, "-m", "psx.apps.worker_app_runner", "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and "WorkerAppRunner" in r.stdout and "-bc" in r.stdout


def test_wide_bsp_schedules_agree():
    """Sparse-input model over the collective schedules (dense delta pushes)."""
    ws = {}
    for sched in ("allreduce", "sharded"):
        out, w = _run(3, dict(BASE, bsp_schedule=sched, _data="wide", max_buffer_size=256, min_buffer_size=64))
        assert out["rounds"] == 5 and out["updates"] == 15
        ws[sched] = w
    assert w.numel() == 3000 * 8 + 8
    assert torch.allclose(ws["allreduce"], ws["sharded"], atol=1e-5)


@pytest.mark.parametrize("sparse_push", [True, False])
def test_wide_async_push(sparse_push):
    out, w = _run(3, dict(BASE, consistency_model=-1, max_iters=6, _data="wide", max_buffer_size=256,
                          min_buffer_size=64, sparse_push=sparse_push))
    assert out["updates"] == 12 and torch.isfinite(w).all()


def test_wide_sparse_pull_matches_dense_pull():
    """One worker (deterministic order): pulling the logged deltas since the last
    pull gives the same model as pulling the dense weights every time."""
    kw = dict(BASE, consistency_model=-1, max_iters=8, _data="wide", max_buffer_size=256, min_buffer_size=64,
              num_workers=1)
    out_s, w_s = _run(2, dict(kw, sparse_pull=True))
    out_d, w_d = _run(2, dict(kw, sparse_pull=False))
    assert out_s["sparse_pulls"] >= 1 and out_d["sparse_pulls"] == 0  # (small test model: dense is often cheaper)
    assert torch.allclose(w_s, w_d, atol=1e-6, rtol=1e-5), (w_s - w_d).abs().max()


@pytest.mark.parametrize("c", [-1, 2])
def test_wide_sparse_pull_multi_worker(c):
    out, w = _run(3, dict(BASE, consistency_model=c, max_iters=6, _data="wide", max_buffer_size=256,
                          min_buffer_size=64))
    assert out["updates"] == 12 and torch.isfinite(w).all()
    assert out["sparse_pulls"] > 0


@pytest.mark.parametrize("c,bound", [(0, 1), (2, 3), (10, 11), (-1, None)])
def test_log_derived_vc_gap(tmp_path, c, bound):
    """The reference validates its consistency models from the logs
    (iteration-vs-time plots, README.md:299-321); automated here: with a
    straggler (worker 1 sleeps per iteration) the max in-flight vector-clock
    gap read back from logs-worker.csv stays within the model's bound
    (BSP <= 1 and SSP(D) <= D + 1 as logged -- SURVEY §4), and ASP runs ahead."""
    import pandas as pd

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from plot_logs import max_vc_gap

    kw = dict(BASE, consistency_model=c, max_iters=12, logging=True, log_dir=str(tmp_path),
              inject_worker_delay_ms={1: 250.0})  # a straggler even on a loaded host
    if c != 0:
        kw["server_colocated"] = False
    out, _ = _run(3, kw)
    w = pd.read_csv(tmp_path / "logs-worker.csv", sep=";")
    s = pd.read_csv(tmp_path / "logs-server.csv", sep=";")
    assert list(s.columns) == ["timestamp", "partition", "vectorClock", "loss", "fMeasure", "accuracy"]
    gap = max_vc_gap(w)
    if bound is not None:
        if gap > bound:
            print(w.sort_values("timestamp").to_string())
        assert gap <= bound, gap
    else:
        assert gap >= 3, gap  # eventual consistency: the fast worker is not held back


def _uid_rank(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from psx.parallel.comm import exchange_unique_id, make_comm

    dist.init_process_group("gloo", rank=rank, world_size=world)
    ids = [exchange_unique_id(rank, lambda: bytes(range(128))) for _ in range(2)]
    assert make_comm(rank, world, "cpu") is None  # CPU / gloo: torch.distributed collectives
    q.put((rank, ids))
    dist.barrier()
    dist.destroy_process_group()


def test_native_comm_unique_id_exchange():
    """Every rank receives rank 0's RCCL unique id through the c10d store (fresh key per communicator)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_uid_rank, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(3))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ids == [bytes(range(128))] * 2 for ids in got.values())


def test_empty_worker_shard_rejected_on_every_rank():
    """Fewer training rows than workers: a worker's round-robin shard would be empty
    and its rank's native loop would stop alone while the peers wait in the round's
    collectives.  Every rank holds the same data, so every rank raises
    at construction, before any collective."""
    import pytest

    from psx.parallel.dist import DistEngine
    from psx.runtime.config import PSConfig
    from psx.utils.data import synth_finefood

    cfg = PSConfig(num_workers=4, consistency_model=0, producer_time_per_event=0, stream_mode="per_iter",
                   rows_per_iter=8, max_iters=2, server_colocated=False)
    for rank in range(5):
        with pytest.raises(ValueError, match="non-empty round-robin shard"):
            DistEngine(cfg, rank, 5, "cpu", train=synth_finefood(3, seed=0), test=synth_finefood(16, seed=1))

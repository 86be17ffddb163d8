"""The wide-model kernels at every launch geometry (csrc/kernels/wide_kernels.hip).

The solve kernels pick their shape from the ring row width NZ and the padded class
count KP: NQ = ceil(NZ / 64) non-zeros per lane (template variants 1, 2, 4, 8),
RB = wide_rows_per_group(NZ, KP) rows per plan group (block 64 * RB, group EB =
RB * NZ, LDS hash TS, uint16 group slots) and a KP variant of every solve and
evaluation kernel.  ``TABLE`` holds one case per variant; a CPU test checks it
against the binding so a retuned LDS budget cannot silently drop a case.

Windows come from ``make_window``: tiny (cap = 2 RB + 5 rows) but with, by
construction, a full row, rows of 63 / 64 / 65 non-zeros, a one-entry row, empty
rows (the last row among them), a feature repeated three times in one row, a hot
feature in every non-empty row, feature ids 0 and F - 1 -- and a variant whose ids
all share one home slot of the group's LDS table.  The reference is the float64
oracle (``WideSolveOp(..., "cpu")`` -> ``local_solve_reference``) with the
tolerances of tests/test_wide.py ``_gpu_vs_cpu``; margins are held to the fp32
summation bound and confusion counts are exact.
"""
import ctypes
import math

import pytest
import torch

from psx import _native
from psx.models.wide import WideSpec, padded_classes
from psx.ops.lr import EvalScratch, SolverOptions, stream_handle
from psx.ops.sparse import IngestBatch, SparseDataset, SparseRing, WideEvalSet, WideSolveOp, wide_logits

# (NZ, K, KP, RB, NQ variant)
TABLE = [
    (8, 16, 16, 8, 1),
    (64, 2, 2, 8, 1),  # boundary: exactly one entry per lane
    (72, 3, 4, 8, 2),
    (128, 6, 8, 8, 2),  # bench.py --model sparse1m
    (128, 1, 1, 8, 2),  # bench.py --model sharded100m
    (256, 6, 8, 7, 4),
    (320, 1, 1, 6, 8),
    (512, 1, 1, 4, 8),
    (512, 6, 8, 3, 8),
    (512, 12, 16, 1, 8),
]
RB_OF = {(nz, k): rb for nz, k, _, rb, _ in TABLE}
F_SMALL = 50_000
F_STRIDED = 1 << 20  # the one-home-slot variant: ids are multiples of 4096
STRIDE = 4096


def _hip_or_skip():
    try:
        return _native.hip()
    except RuntimeError as e:  # extension not built
        pytest.skip(str(e))


def _cap(RB):
    return min(21, 2 * RB + 5)


def _nq_variant(NZ):
    nq = -(-NZ // 64)
    return next(v for v in (1, 2, 4, 8) if nq <= v)


# ---------------------------------------------------------------------------
# window generator
def make_window(F, K, NZ, rows, seed, stride=1):
    """``rows`` CSR rows of up to NZ entries (see the module docstring for what every
    window holds).  Returns (SparseDataset, meta); meta: hot / dup feature ids, row lengths."""
    assert rows >= 7 and NZ >= 8
    g = torch.Generator().manual_seed(1000 * seed + NZ + 7 * K)
    if stride > 1:
        pool = torch.arange(0, F, stride)
        hot, dup = int(pool[len(pool) // 2]), int(pool[len(pool) // 3])
    else:
        pool = None
        hot, dup = 12_345 % F, 23_456 % F
    lens = [NZ, 1, 0] + [n for n in (63, 64, 65) if n <= NZ and n != NZ]
    dup_len = 65 if 65 <= NZ else min(NZ, 5)  # the row that repeats `dup` three times
    if dup_len not in lens or dup_len == NZ:
        lens.append(dup_len)
    while len(lens) < rows - 1:
        lens.append(int(torch.randint(2, NZ + 1, (1,), generator=g)))
    assert len(lens) == rows - 1, (lens, rows)
    order = torch.randperm(rows - 1, generator=g).tolist()
    lens = [lens[i] for i in order] + [0]  # the window's last row is empty
    dup_row = next(i for i, n in enumerate(lens) if n == dup_len)
    full_row = next(i for i, n in enumerate(lens) if n == NZ)

    def others(n, banned):
        if n <= 0:
            return torch.zeros(0, dtype=torch.int64)
        if pool is None:
            c = torch.randperm(F - 2, generator=g) + 1  # 1 .. F - 2
        else:
            c = pool[torch.randperm(len(pool), generator=g)]
        c = c[~torch.isin(c, torch.tensor(sorted(banned)))]
        if len(c) < n:  # the strided pool is smaller than a long row: ids repeat (and are summed)
            c = c[torch.randint(0, len(c), (n,), generator=g)]
        return c[:n]

    idx, val, indptr = [], [], [0]
    for r, n in enumerate(lens):
        if n == 0:
            ids = torch.zeros(0, dtype=torch.int64)
        elif r == dup_row:
            rest = torch.cat([torch.tensor([hot, dup, dup]), others(n - 4, {hot, dup})])
            ids = torch.cat([rest[torch.randperm(n - 1, generator=g)], torch.tensor([dup])])  # one copy is the last entry
        elif r == full_row and pool is None:
            rest = torch.cat([torch.tensor([hot, 0, F - 1]), others(n - 3, {hot})])
            ids = rest[torch.randperm(n, generator=g)]
        else:
            rest = torch.cat([torch.tensor([hot]), others(n - 1, {hot})])
            ids = rest[torch.randperm(n, generator=g)]
        v = torch.randn(n, generator=g)
        v = torch.sign(v) * (v.abs() + 0.1) / math.sqrt(max(n, 1))
        idx.append(ids)
        val.append(v)
        indptr.append(indptr[-1] + n)
    y = torch.randint(0, max(K, 2), (rows,), generator=g).to(torch.int32)
    ds = SparseDataset(torch.tensor(indptr, dtype=torch.int64), torch.cat(idx).to(torch.int32),
                       torch.cat(val).to(torch.bfloat16), y, F)
    return ds, dict(hot=hot, dup=dup, lens=lens, dup_row=dup_row, full_row=full_row)


def _row(ds, r):
    a, b = int(ds.indptr[r]), int(ds.indptr[r + 1])
    return ds.idx[a:b].long(), ds.val[a:b]


@pytest.mark.parametrize("NZ,K,stride", [(nz, k, 1) for nz, k, *_ in TABLE] + [(512, 6, STRIDE), (128, 6, STRIDE),
                                                                              (8, 16, STRIDE)])
def test_window_generator_properties(NZ, K, stride):
    F = F_STRIDED if stride > 1 else F_SMALL
    rows = _cap(RB_OF[(NZ, K)])
    ds, meta = make_window(F, K, NZ, rows, seed=0, stride=stride)
    lens = (ds.indptr[1:] - ds.indptr[:-1]).tolist()
    assert ds.rows == rows and lens == meta["lens"] and max(lens) == NZ and ds.max_nnz == NZ
    for n in (1, NZ) + tuple(n for n in (63, 64, 65) if n <= NZ):
        assert n in lens, (n, lens)
    assert lens.count(0) >= 2 and lens[-1] == 0
    ids, _ = _row(ds, meta["dup_row"])
    assert int((ids == meta["dup"]).sum()) == 3 and int(ids[-1]) == meta["dup"]
    for r, n in enumerate(lens):
        if n:
            assert meta["hot"] in _row(ds, r)[0].tolist()
    assert int(ds.idx.min()) >= 0 and int(ds.idx.max()) < F and float(ds.val.float().abs().min()) > 0
    if stride > 1:
        assert bool((ds.idx.long() % stride == 0).all())
        assert bool((((ds.idx.long() * 2654435761) & 4095) == 0).all())  # wide_hash(f) & (TS - 1), TS <= 4096
    else:
        full = _row(ds, meta["full_row"])[0].tolist()
        assert 0 in full and F - 1 in full
    assert set(ds.y.tolist()) <= set(range(max(K, 2)))


def test_geometry_table_covers_every_variant():
    """TABLE against wide_rows_per_group: every NQ / RB / KP class keeps a case."""
    h = _hip_or_skip()
    seen = {"NQ": set(), "RB": set(), "KP": set()}
    for NZ, K, KP, RB, NQ in TABLE:
        assert padded_classes(K) == KP
        got = (int(h.wide_rows_per_group(NZ, KP)), _nq_variant(NZ), KP)
        assert got == (RB, NQ, KP), f"NZ {NZ} K {K}: the table says (RB, NQ, KP) = {(RB, NQ, KP)}, the kernels run {got}"
        op = WideSolveOp(WideSpec(F_SMALL, K), _cap(RB), NZ, "cpu", SolverOptions())
        assert op.geometry == got
        seen["NQ"].add(got[1])
        seen["RB"].add(got[0])
        seen["KP"].add(got[2])
    want = {"NQ": {1, 2, 4, 8}, "RB": {1, 3, 4, 6, 7, 8}, "KP": {1, 2, 4, 8, 16}}
    for name in want:
        assert want[name] <= seen[name], f"no case left for {name} in {sorted(want[name] - seen[name])}"


# ---------------------------------------------------------------------------
# the solve against the float64 oracle
def _opts(std=True, iters=2):
    return SolverOptions(standardize=std, zero_const=False, iters=iters)


_DATA = {}
_ORACLE = {}


def _case(NZ, K, seed=0, stride=1):
    """(spec, ds, meta, cap, CPU ring) of one geometry; built once."""
    key = (NZ, K, seed, stride)
    if key not in _DATA:
        F = F_STRIDED if stride > 1 else F_SMALL
        cap = _cap(RB_OF[(NZ, K)])
        ds, meta = make_window(F, K, NZ, cap, seed, stride)
        ring = SparseRing(cap, NZ, "cpu")
        ring.ingest_from(ds, 0, 1, cap, 0)
        _DATA[key] = (WideSpec(F, K), ds, meta, cap, ring)
    return _DATA[key]


def _w_old(spec, scale):
    return spec.init("random", seed=5, scale=scale)


def _window_ids(ds, cap, B, start):
    rows = [(start + i) % cap for i in range(B)]
    return torch.unique(torch.cat([_row(ds, r)[0] for r in rows] + [torch.zeros(0, dtype=torch.int64)]))


def _oracle(NZ, K, seed=0, stride=1, B=None, start=0, std=True, iters=2, scale=0.05):
    spec, ds, meta, cap, ring = _case(NZ, K, seed, stride)
    B = cap if B is None else B
    key = (NZ, K, seed, stride, B, start, std, iters, scale)
    if key not in _ORACLE:
        op = WideSolveOp(spec, cap, NZ, "cpu", _opts(std, iters), dense_delta=True)
        op.run(ring, B, start, _w_old(spec, scale))
        _ORACLE[key] = (op.delta.clone(), float(op.loss), op.stats.tolist())
    return _ORACLE[key]


def _gpu_ring(cuda, ds, cap, NZ):
    ring = SparseRing(cap, NZ, cuda)
    ring.ingest_from(ds.to(cuda), 0, 1, cap, 0)
    return ring


def _check_against_oracle(spec, ds, cap, B, start, op, oracle):
    """Everything test_wide.py _gpu_vs_cpu asserts (same tolerances) + the exact plan,
    untouched features and padded classes."""
    torch.cuda.synchronize()
    dc, lc, sc = oracle
    dg, lg, sg = op.delta.cpu(), float(op.loss), op.stats.cpu().tolist()
    scale = dc.abs().max().item()
    err = (dc - dg).abs().max().item()
    print(f"evals/accepted cpu {sc[:2]} gpu {sg[:2]}  loss cpu {lc:.9g} gpu {lg:.9g}  |d delta| {err:.3g} of {scale:.3g}")
    assert sc[0] == sg[0] and sc[1] == sg[1], (sc, sg)  # evaluations and accepted steps
    assert math.isclose(lc, lg, rel_tol=1e-4), (lc, lg)
    assert err <= 2e-3 * scale + 1e-6, (err, scale)
    assert op.barrier_errors() == 0
    # the plan: exactly the window's distinct features
    want = _window_ids(ds, cap, B, start)
    U = op.host_count()
    assert U == int(want.numel())
    assert torch.equal(torch.sort(op.uniq[:U].cpu().long()).values, want)
    # untouched features and padded classes: exactly zero
    KP, K, F = spec.KP, spec.K, spec.F
    dd = dg[: F * KP].view(F, KP)
    touched = torch.zeros(F, dtype=torch.bool)
    touched[want] = True
    assert dd[~touched].abs().max().item() == 0.0
    if KP > K:
        assert dd[:, K:].abs().max().item() == 0.0 and dg[F * KP + K:].abs().max().item() == 0.0
        for buf in (op.dloc, op.wloc):
            loc = buf[: KP + U * KP].view(U + 1, KP).cpu()
            assert loc[:, K:].abs().max().item() == 0.0
    return dg, lg, sg


def _gpu_vs_oracle(cuda, NZ, K, seed=0, stride=1, B=None, start=0, std=True, iters=2, scale=0.05, op=None, ring=None):
    spec, ds, meta, cap, _ = _case(NZ, K, seed, stride)
    B = cap if B is None else B
    oracle = _oracle(NZ, K, seed, stride, B, start, std, iters, scale)
    ring = _gpu_ring(cuda, ds, cap, NZ) if ring is None else ring
    if op is None:
        op = WideSolveOp(spec, cap, NZ, cuda, _opts(std, iters), dense_delta=True)
    w = _w_old(spec, scale).to(cuda)
    op.run(ring, B, start, w)
    res = _check_against_oracle(spec, ds, cap, B, start, op, oracle)
    return spec, ds, op, ring, w, res


@pytest.mark.gpu
@pytest.mark.parametrize("NZ,K,KP,RB,NQ", TABLE)
def test_gpu_solve_matches_oracle_per_geometry(cuda, NZ, K, KP, RB, NQ):
    spec, ds, op, *_ = _gpu_vs_oracle(cuda, NZ, K)
    assert op.geometry == (RB, NQ, KP)


@pytest.mark.gpu
@pytest.mark.parametrize("NZ,K", [(512, 6), (128, 6), (8, 16)])
def test_gpu_solve_one_home_slot(cuda, NZ, K):
    """Every id a multiple of 4096: one home slot of the group's LDS table (TS <= 4096),
    so the probe chains are as long as the group has features; the long rows repeat ids."""
    _gpu_vs_oracle(cuda, NZ, K, stride=STRIDE)


@pytest.mark.gpu
@pytest.mark.parametrize("NZ,K", [(512, 6), (512, 12)])  # RB 3 and RB 1
@pytest.mark.parametrize("std", [True, False])
def test_gpu_solve_standardize_on_off(cuda, NZ, K, std):
    _gpu_vs_oracle(cuda, NZ, K, std=std)


def _full_row_slot(NZ, K):
    return _case(NZ, K)[2]["full_row"]


@pytest.mark.gpu
@pytest.mark.parametrize("NZ,K", [(512, 6), (256, 6)])  # RB 3 and RB 7
def test_gpu_solve_window_shapes(cuda, NZ, K):
    """B around the group size (a last group of 1 .. RB rows), one row, the whole ring,
    and a window that wraps past the ring's end -- on one op and ring."""
    spec, ds, meta, cap, _ = _case(NZ, K)
    RB = RB_OF[(NZ, K)]
    ring = _gpu_ring(cuda, ds, cap, NZ)
    op = WideSolveOp(spec, cap, NZ, cuda, _opts(True), dense_delta=True)
    for B, start in ((RB - 1, 0), (RB, 1), (RB + 1, 2), (cap, 0), (RB + 2, cap - 3), (cap, cap - 1)):
        _gpu_vs_oracle(cuda, NZ, K, B=B, start=start, op=op, ring=ring)
    # one row (its variance is undefined: standardize off); the full row
    _gpu_vs_oracle(cuda, NZ, K, B=1, start=_full_row_slot(NZ, K), std=False)


@pytest.mark.gpu
@pytest.mark.parametrize("NZ,K", [(512, 6), (256, 6)])
def test_gpu_solve_back_to_back_equals_fresh(cuda, NZ, K):
    """The next solve's begin clears exactly the previous solve's table entries (hslot):
    a second solve on another window == a fresh op's solve of that window, bit for bit."""
    spec, ds, meta, cap, _ = _case(NZ, K)
    RB = RB_OF[(NZ, K)]
    ring = _gpu_ring(cuda, ds, cap, NZ)
    first, second = (cap, 0), (RB + 1, cap - 2)
    op = WideSolveOp(spec, cap, NZ, cuda, _opts(True), dense_delta=True)
    _gpu_vs_oracle(cuda, NZ, K, B=first[0], start=first[1], op=op, ring=ring)
    *_, (d2, l2, s2) = _gpu_vs_oracle(cuda, NZ, K, B=second[0], start=second[1], op=op, ring=ring)
    *_, (df, lf, sf) = _gpu_vs_oracle(cuda, NZ, K, B=second[0], start=second[1], ring=ring)
    nbad = int((d2 != df).sum())
    print(f"second vs fresh: {nbad} entries differ, max {(d2 - df).abs().max().item():.3g}; loss {l2!r} {lf!r}")
    assert torch.equal(d2, df) and l2 == lf and s2 == sf


def _raw_solve(cuda, spec, ring, w, opts, persist, windows):
    """The native solver as tests/test_gpu_keyrange.py drives it (persist: the one-launch
    solve).  Returns [(dense delta, loss, stats, barrier flag)] per window."""
    h = _native.hip()
    c = h.WideCfg()
    c.K, c.KP, c.F, c.cap, c.NZ = spec.K, spec.KP, spec.F, ring.cap, ring.NZ
    c.iters, c.hist, c.ls_max, c.nslots, c.mode, c.gd_lr, c.tol = (opts.iters, opts.hist, opts.ls_max, opts.nslots, 0,
                                                                  opts.gd_lr, opts.tol)
    c.standardize, c.center, c.zero_const = int(opts.standardize), int(opts.center), int(opts.zero_const)
    c.persist = int(persist)
    umax = min(spec.F, ring.cap * ring.NZ)
    pl = spec.KP + umax * spec.KP
    dloc, wloc = torch.zeros(pl, device=cuda), torch.zeros(pl, device=cuda)
    loss, stats = torch.zeros(1, device=cuda), torch.zeros(8, dtype=torch.int32, device=cuda)
    uniq = torch.zeros(umax, dtype=torch.int32, device=cuda)
    s = h.WideSolver(c, ring.idx.data_ptr(), ring.val.data_ptr(), ring.nnz.data_ptr(), ring.y.data_ptr(),
                     w.data_ptr(), dloc.data_ptr(), wloc.data_ptr(), loss.data_ptr(), stats.data_ptr(),
                     uniq.data_ptr(), 0, True)
    assert s.kernels_per_solve == 1 if persist else s.kernels_per_solve > 5
    out = []
    for B, start in windows:
        s.run(B, start, stream_handle(cuda))
        torch.cuda.synchronize()
        U = s.ucount_host
        dense = torch.zeros(spec.P)
        dense[spec.F * spec.KP:] = dloc[: spec.KP].cpu()
        dense[: spec.F * spec.KP].view(spec.F, spec.KP)[uniq[:U].long().cpu()] = \
            dloc[spec.KP: spec.KP + U * spec.KP].view(U, spec.KP).cpu()
        out.append((dense, loss.item(), stats[:4].tolist(), int(stats[4].item())))
    return out


FORMS = [(512, 6), (256, 6), (128, 1)]  # RB 3, RB 7, the benchmark's binary rows
# window seeds of the retry cases, picked on the CPU oracle alone: the first seed for
# which, with and without standardisation, (a) a line search of the float64 oracle
# retries and (b) the same oracle run in float32 stays within a quarter of the
# tolerances of the float64 one (a 30x model on 512-wide rows can be too ill-conditioned
# for ANY fp32 solve: profiles/r09/README.md has the gaps of the seeds passed over)
TAIL_SEED = {(512, 6): 2, (256, 6): 1, (128, 1): 0}


@pytest.mark.gpu
@pytest.mark.parametrize("NZ,K", FORMS)
def test_gpu_persistent_solve_equals_chain(cuda, NZ, K):
    """The one-launch persistent solve (512-thread blocks masked with wv < RB) == the launch
    chain (64 * RB threads): the comparison of test_persistent_wide_solve_equals_chain."""
    spec, ds, meta, cap, _ = _case(NZ, K)
    ring = _gpu_ring(cuda, ds, cap, NZ)
    windows = ((cap, 0), (RB_OF[(NZ, K)] + 1, cap - 2), (cap - 1, 3))
    for scale, iters in ((0.05, 2), (30.0, 4)):
        w = _w_old(spec, scale).to(cuda)
        outs = [_raw_solve(cuda, spec, ring, w, _opts(True, iters), p, windows) for p in (False, True)]
        for (da, la, sa, ea), (db, lb, sb, eb) in zip(*outs):
            sc = da.abs().max().item()
            print(f"scale {scale}: stats {sa} {sb} loss {la!r} {lb!r} |d| {(da - db).abs().max().item():.3g} of {sc:.3g}")
            assert ea == 0 and eb == 0 and sa == sb
            assert (da - db).abs().max().item() <= 1e-4 * sc + 1e-7
            assert abs(la - lb) <= 1e-5 * abs(la)


@pytest.mark.gpu
@pytest.mark.parametrize("NZ,K", FORMS)
@pytest.mark.parametrize("std", [True, False])
def test_gpu_tail_retry_slots_match_oracle(cuda, NZ, K, std):
    """Line searches that need retries run in the persistent tail launch (as in
    test_gpu_wide_retry_slots_in_tail: a large initial model, iters = 4)."""
    seed = TAIL_SEED[(NZ, K)]
    sc = _oracle(NZ, K, seed=seed, std=std, iters=4, scale=30.0)[2]
    assert sc[0] > 1 + sc[1], sc  # some line search needed a retry: the tail's slots run
    _gpu_vs_oracle(cuda, NZ, K, seed=seed, std=std, iters=4, scale=30.0)


# ---------------------------------------------------------------------------
# margins and evaluation against float64
EVAL_NZ = 512
EVAL_LENS = {1: [EVAL_NZ], 3: [0, 65, EVAL_NZ], 17: [0, 1, 15, 16, 17, 63, 64, 65, EVAL_NZ, 64, 0, 17, 1, 63, 16, 65, 15]}
EVAL_KS = [1, 2, 3, 6, 12, 16]
U24 = 2.0 ** -24


def _eval_set(K, T, seed, shared):
    """T test rows with the lengths of EVAL_LENS[T]; about half the ids of every row come
    from ``shared`` (a solved window's features, so an overlay has something to replace)."""
    g = torch.Generator().manual_seed(77 * seed + 1000 * K + T)
    idx, val, indptr = [], [], [0]
    for n in EVAL_LENS[T]:
        a = shared[torch.randperm(len(shared), generator=g)[: n // 2]]
        b = torch.randperm(F_SMALL, generator=g)[: n - len(a)]
        ids = torch.cat([a, b])[torch.randperm(n, generator=g)] if n else torch.zeros(0, dtype=torch.int64)
        v = torch.randn(n, generator=g)
        idx.append(ids)
        val.append(torch.sign(v) * (v.abs() + 0.1) / math.sqrt(max(n, 1)))
        indptr.append(indptr[-1] + n)
    y = torch.randint(0, max(K, 2), (T,), generator=g).to(torch.int32)
    return SparseDataset(torch.tensor(indptr, dtype=torch.int64), torch.cat(idx).to(torch.int32),
                         torch.cat(val).to(torch.bfloat16), y, F_SMALL)


def _eval_model(spec, seed=4):
    w = spec.init("random", seed=seed, scale=1.0)
    g = torch.Generator().manual_seed(seed + 99)
    w[spec.F * spec.KP: spec.F * spec.KP + spec.K] = torch.randn(spec.K, generator=g)
    return w


def _margins64(spec, ds, w, extra=None):
    """float64 margins [T, K] of the bf16 values as stored, and the fp32 recursive-sum bound
    (nnz + 8) 2^-24 (sum |v w| + |b|) per row and class (+ ``extra`` [F, KP], |b| rows: an
    additional absolute per-coefficient error, times 2^-24 sum |v| extra)."""
    K, KP, F = spec.K, spec.KP, spec.F
    W = w[: F * KP].view(F, KP)[:, :K].double()
    b = w[F * KP: F * KP + K].double()
    z = torch.zeros(ds.rows, K, dtype=torch.float64)
    bound = torch.zeros(ds.rows, K, dtype=torch.float64)
    for r in range(ds.rows):
        ids, v = _row(ds, r)
        t = v.double()[:, None] * W[ids]
        z[r] = t.sum(0) + b
        bound[r] = (len(ids) + 8) * U24 * (t.abs().sum(0) + b.abs())
        if extra is not None:
            E, eb = extra
            bound[r] += U24 * ((v.double().abs()[:, None] * E[ids]).sum(0) + eb)
    return z, bound


def _predict64(spec, z, bound):
    """float64 prediction and whether it is safe: the gap to the runner-up (|z| for the
    binary model) exceeds twice the bound (each compared margin carries its own error)."""
    if spec.K == 1:
        return (z[:, 0] > 0).long(), z[:, 0].abs() > 2 * bound[:, 0]
    top = z.topk(2, dim=1)
    gap = top.values[:, 0] - top.values[:, 1]
    return top.indices[:, 0], gap > 2 * bound.max(dim=1).values


def _confusion(spec, ds, pred):
    y = ds.y.long()
    if spec.K == 1:
        y = (y > 0).long()
    c = torch.zeros(256, dtype=torch.int64)
    c.index_add_(0, y.clamp(0, 15) * 16 + pred, torch.ones_like(y))
    return c


def _overlay_case(K):
    """The window whose solve the overlay evaluations use (NZ 72, the table's RB 8 / NQ 2 row)."""
    F, NZ, cap = F_SMALL, 72, 21
    key = ("ov", K)
    if key not in _DATA:
        ds, _ = make_window(F, K, NZ, cap, seed=3)
        _DATA[key] = (WideSpec(F, K), ds, NZ, cap)
    return _DATA[key]


@pytest.mark.parametrize("K", EVAL_KS)
def test_eval_inputs_are_decided(K):
    """The condition for exact confusion counts, on the inputs alone: no test row's float64
    decision is within twice the fp32 summation bound."""
    spec, win, _, _ = _overlay_case(K)
    w = _eval_model(spec)
    for T in EVAL_LENS:
        ds = _eval_set(K, T, 0, torch.unique(win.idx.long()))
        assert (ds.indptr[1:] - ds.indptr[:-1]).tolist() == EVAL_LENS[T]
        z, bound = _margins64(spec, ds, w)
        _, safe = _predict64(spec, z, bound)
        assert bool(safe.all()), (K, T, safe.tolist())


def _plain_counts(cuda, spec, ds, w, table=(0, 0), wloc=0):
    acc = torch.zeros(512, dtype=torch.int32, device=cuda)
    _native.hip().wide_eval(spec.K, spec.KP, spec.F, ds.indptr.data_ptr(), ds.idx.data_ptr(), ds.val.data_ptr(),
                            ds.y.data_ptr(), ds.rows, w.data_ptr(), table[0], table[1], wloc, acc.data_ptr(),
                            stream=stream_handle(cuda))
    torch.cuda.synchronize()
    assert int(acc[256:].abs().sum()) == 0
    return acc[:256].cpu().long()


def _slot_counts(addr):
    return torch.tensor((ctypes.c_int32 * 256).from_address(addr)[:], dtype=torch.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("K", EVAL_KS)
def test_gpu_logits_and_eval_per_kp(cuda, K):
    from psx.utils.logsink import _HostSlots

    spec, win, NZ, cap = _overlay_case(K)
    KP, F = spec.KP, spec.F
    w = _eval_model(spec)
    wg = w.to(cuda)
    # the overlay: a solve from w on the window (its own check is the solve tests')
    ring = _gpu_ring(cuda, win, cap, NZ)
    op = WideSolveOp(spec, cap, NZ, cuda, _opts(True), dense_delta=True)
    op.run(ring, cap, 0, wg)
    torch.cuda.synchronize()
    assert op.barrier_errors() == 0
    delta = op.delta.cpu()
    w_local = (w.double() + delta.double())
    # w_old + delta re-rounds the overlay's coefficients (delta = wloc - w_old in fp32):
    # up to 2^-24 |delta| per coefficient on top of the summation bound
    extra = (delta[: F * KP].view(F, KP)[:, : spec.K].double().abs(), delta[F * KP: F * KP + spec.K].double().abs())
    slots = _HostSlots(4, True)
    sb = _native.host.EVAL_SLOT_BYTES
    try:
        for T in EVAL_LENS:
            ds = _eval_set(K, T, 0, torch.unique(win.idx.long()))
            dg = ds.to(cuda)
            z64, bound = _margins64(spec, ds, w)
            zg = wide_logits(spec, dg, wg).cpu()
            err = (zg[:, : spec.K].double() - z64).abs()
            print(f"K {K} T {T}: worst margin error / bound {(err / bound).max().item():.3f}")
            assert bool((err <= bound).all()), (err / bound).max().item()
            if KP > spec.K:
                assert zg[:, spec.K:].abs().max().item() == 0.0  # zero padding contributes exactly 0
            pred, safe = _predict64(spec, z64, bound)
            assert bool(safe.all())
            plain = _plain_counts(cuda, spec, dg, wg)
            assert torch.equal(plain, _confusion(spec, ds, pred))
            # overlay: the local model = w_old + the op's own delta
            zl, bl = _margins64(spec, ds, w_local, extra)
            predl, safel = _predict64(spec, zl, bl)
            assert bool(safel.all()), (K, T, safel.tolist())
            over = _plain_counts(cuda, spec, dg, wg, op.table, op.wloc.data_ptr())
            assert torch.equal(over, _confusion(spec, ds, predl))
            # paired: both rows in one pass == the two single passes == the references
            ev, sc = WideEvalSet(spec, ds, cuda), EvalScratch(cuda)
            a = [slots.ptr + i * sb for i in range(4)]
            ev.eval_pair_to_slots(op, wg, None, wg, sc, a[0], 1, op.loss, a[1], 2)
            ev.eval_to_slot(op, wg, sc, a[2], 3, op.loss)
            ev.eval_to_slot(None, wg, sc, a[3], 4, None)
            torch.cuda.synchronize()
            got = [_slot_counts(p) for p in a]
            assert torch.equal(got[0], got[2]) and torch.equal(got[1], got[3])
            assert torch.equal(got[0], over) and torch.equal(got[1], plain)
            assert sc.acc.abs().sum().item() == 0
    finally:
        slots.free()


def _ingest_source(F=F_SMALL):
    lens = [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 600, 3, 0, 520, 8, 2, 512, 9, 1] * 3
    g = torch.Generator().manual_seed(11)
    idx = torch.randint(0, F, (sum(lens),), generator=g).to(torch.int32)
    val = torch.randn(sum(lens), generator=g).to(torch.bfloat16)
    indptr = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0)
    return SparseDataset(indptr, idx, val, torch.arange(len(lens), dtype=torch.int32), F)


def _rings_equal(rc, rg):
    assert torch.equal(rc.nnz, rg.nnz.cpu()) and torch.equal(rc.y, rg.y.cpu()) and int(rc.trunc) == int(rg.trunc)
    for s in range(rc.cap):
        k = int(rc.nnz[s])
        assert torch.equal(rc.idx[s, :k], rg.idx[s, :k].cpu())
        assert torch.equal(rc.val[s, :k].view(torch.int16), rg.val[s, :k].cpu().view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("NZ", [8, 512])
def test_gpu_ring_ingest_wide_and_narrow_rows(cuda, NZ):
    """sparse_ring_ingest and the batched ingest (IngestBatch): every third source row, a
    destination that wraps, source rows longer than NZ -- bit-equal to the CPU ring."""
    ds = _ingest_source()
    dg = ds.to(cuda)
    cap, n = 16, 14  # 14 rows into 16 slots from slot 11: the destination wraps
    rc, rg = SparseRing(cap, NZ, "cpu"), SparseRing(cap, NZ, cuda)
    rc.ingest_from(ds, 2, 3, n, 11)
    rg.ingest_from(dg, 2, 3, n, 11)
    torch.cuda.synchronize()
    assert int(rc.trunc) > 0
    _rings_equal(rc, rg)
    batch = IngestBatch()
    jobs = ((0, 3, n, 13), (1, 3, 12, 9))
    cpu, gpu = [], []
    for first, step, cnt, dst in jobs:
        c, q = SparseRing(cap, NZ, "cpu"), SparseRing(cap, NZ, cuda)
        c.ingest_from(ds, first, step, cnt, dst)
        q.batch = batch
        q.ingest_from(dg, first, step, cnt, dst)
        cpu.append(c)
        gpu.append(q)
    assert len(batch.jobs) == 2
    batch.flush(cuda)
    torch.cuda.synchronize()
    for c, q in zip(cpu, gpu):
        assert int(c.trunc) > 0
        _rings_equal(c, q)

"""The invariant chain of the full-batch fitters: a float64 checker of the optimiser
state (``x, d, g_c, g_t, beta_t, wfix, S, Y``) read back after ``begin`` and after
every accepted step (``read_state`` of the native fitters).  Every link is checked on
its own, on the device's own vectors, so the check depends neither on how sensitive a
trajectory is nor on how often a line search retries.

  1. gradient   g_c equals the float64 gradient of the objective at the device's x
                (beta = x, coef = x / sigma + wfix, bf16 rows as stored) under the
                derived bound of one evaluation (``eval_oracle`` of _fit_cases.py /
                _wide_fit_cases.py) carried to standardised space (bound / sigma), plus
                2^-23 (|g| + reg |beta|) for the L2 term and the final roundings.
  2. pairs      the accepted step is x_i = fl32(x_{i-1} + t d_{i-1}) for ONE scalar t;
                the pushed pair is S = fl32(t d_{i-1}) (S / d constant to 2^-22 where
                |d| > 2^-20 max|d|) and Y = g_c,i - g_c,i-1 exactly in fp32.  The slot is
                found by comparing S, Y with the previous snapshot: exactly one slot
                changes per push, a live slot is overwritten only when H pairs are live
                (and then the oldest), and no slot changes only where the controller
                declined the pair (s.y <= 1e-10 y.y): recomputed here in float64 from the
                state, with a factor 10 of room for the controller's own dots.
                The first step's Y is held to the float64 gradient of the start under
                the evaluation bound (the start's gradient is in no snapshot).
  3. direction  d equals -H g_c of the float64 two-loop recursion over the device's live
                pairs, oldest first as link 2 ordered them.  The tolerance is measured on
                the reference alone: the two-loop is recomputed 16 times with every
                element of the pairs and of g_c moved by a random relative +-2^-24, and
                the tolerance is 8 x the largest movement of d seen (inf-norm).  It must
                stay below 1e-3 max|d| -- a condition on the inputs.
  4. trial      beta_t = fl32(x + t d) (t = 1 after an accept, beta_t = x after begin);
                the padding elements of every vector are exactly zero; ``current()``
                equals the float64 finalisation of x to 2^-22 relative + K 2^-24 max|.|.

``Chain`` holds the order of the live pairs; ``DenseProblem`` / ``WideProblem`` give
the float64 objective in the layout of the fitter's vectors; ``emulate`` produces
snapshots of a float64 L-BFGS rounded to fp32 the way the device rounds (the
checker's self-tests in test_fit_chain_cpu.py run on them)."""
import torch

U22 = 2.0 ** -22
U23 = 2.0 ** -23
U24 = 2.0 ** -24
VECS = ("x", "d", "g_c", "g_t", "beta_t", "wfix")


class ChainError(AssertionError):
    def __init__(self, link, msg):
        super().__init__(f"link {link}: {msg}")
        self.link = link


def _fail(link, msg):
    raise ChainError(link, msg)


def two_loop(S, Y, g):
    """-H g of the textbook two-loop recursion; S, Y: lists of float64 vectors, oldest first."""
    if not S:
        return -g.clone()
    q = g.clone()
    alphas = []
    for s, y in zip(reversed(S), reversed(Y)):
        rho = 1.0 / float(s @ y)
        a = rho * float(s @ q)
        alphas.append((rho, a))
        q = q - a * y
    r = (float(S[-1] @ Y[-1]) / float(Y[-1] @ Y[-1])) * q
    for (s, y), (rho, a) in zip(zip(S, Y), reversed(alphas)):
        r = r + s * (a - rho * float(y @ r))
    return -r


def direction_tolerance(S, Y, g, seed=0, draws=16):
    """(d64, tol): tol = 8 x the largest inf-norm movement of the two-loop's d under
    random relative +-2^-24 perturbations of every element of S, Y and g (16 draws)."""
    d = two_loop(S, Y, g)
    gen = torch.Generator().manual_seed(977 + seed)

    def jig(v):
        sign = torch.randint(0, 2, v.shape, generator=gen).double() * 2 - 1
        return v * (1.0 + sign * U24)

    move = 0.0
    for _ in range(draws):
        dp = two_loop([jig(s) for s in S], [jig(y) for y in Y], jig(g))
        move = max(move, float((dp - d).abs().max()))
    return d, 8.0 * move


class Chain:
    """Feed it the snapshot after ``begin`` and then the one after every accepted step.

    A snapshot is a dict of CPU fp32 tensors ``x d g_c g_t beta_t wfix`` [nv] and
    ``S Y`` [H, nv] plus ``dir_reset`` (the fitter's counter).  ``problem`` gives
    ``n``, ``pad`` (bool [nv]: elements that must be zero), ``grad(x64, wfix64) ->
    (g64 [n], bound [n])`` and ``finalize(x64, wfix64) -> float64 current()``."""

    def __init__(self, problem, H, seed=0):
        self.p, self.H, self.seed = problem, H, seed
        self.prev = None
        self.live = []  # slots, oldest first
        self.steps = 0
        self.pushes = self.declined = self.wraps = 0
        self.dir_tol = []  # (tolerance / max|d|, error / tolerance) per step
        self.grad_ratio = 0.0

    # ---- pieces ---------------------------------------------------------------------
    def _padding(self, s):
        for k in VECS:
            if bool((s[k][self.p.pad] != 0).any()):
                _fail(4, f"padding of {k} is not zero")
        for k in ("S", "Y"):
            if bool((s[k][:, self.p.pad] != 0).any()):
                _fail(4, f"padding of {k} is not zero")

    def _gradient(self, s):
        n = self.p.n
        g64, bound = self.p.grad(s["x"][:n].double(), s["wfix"][:n].double())
        err = (s["g_c"][:n].double() - g64).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        self.grad_ratio = max(self.grad_ratio, ratio)
        if not bool((err <= bound).all()):
            i = int((err - bound).argmax())
            _fail(1, f"g_c[{i}] = {float(s['g_c'][i]):.9g}, float64 {float(g64[i]):.9g}, bound {float(bound[i]):.3e} "
                     f"(largest err/bound {ratio:.3g})")
        return g64

    def begin(self, s):
        self._padding(s)
        n = self.p.n
        for k in ("d", "g_c"):
            if bool((s[k] != 0).any()):
                _fail(4, f"{k} is not zero after begin")
        if bool((s["S"] != 0).any()) or bool((s["Y"] != 0).any()):
            _fail(2, "history not cleared by begin")
        if not torch.equal(s["beta_t"][:n], s["x"][:n]):
            _fail(4, "trial point differs from x after begin")
        self.g0 = self.p.grad(s["x"][:n].double(), s["wfix"][:n].double())
        self.prev, self.live, self.steps = s, [], 0

    def step(self, s, current=None):
        """One accepted (non-final) step: snapshot ``s`` against the previous one."""
        n, H, prev = self.p.n, self.H, self.prev
        self.steps += 1
        self._padding(s)
        if not torch.equal(s["wfix"], prev["wfix"]):
            _fail(4, "wfix changed during the fit")
        self._gradient(s)
        if not torch.equal(s["g_t"][:n], s["g_c"][:n]):
            _fail(1, "g_c is not the gradient of the accepted evaluation (g_t)")
        # ---- link 2 ----
        x0, x1 = prev["x"][:n].double(), s["x"][:n].double()
        first = self.steps == 1  # the first direction and the start's gradient are in no snapshot: g0 is float64's
        d0 = None if first else prev["d"][:n].double()
        changed = [j for j in range(H)
                   if not (torch.equal(s["S"][j], prev["S"][j]) and torch.equal(s["Y"][j], prev["Y"][j]))]
        if len(changed) > 1:
            _fail(2, f"{len(changed)} slots changed in one push: {changed}")
        y32 = None if first else s["g_c"][:n] - prev["g_c"][:n]
        if not changed:
            if not first:
                dx, y64 = x1 - x0, y32.double()
                sy, yy = float(dx @ y64), float(y64 @ y64)
                if sy > 1e-9 * (yy if yy > 0 else 1.0) and yy > 0:
                    _fail(2, f"no slot changed, but the pair is a keeper (s.y {sy:.3e}, y.y {yy:.3e})")
            self.declined += 1
        else:
            j = changed[0]
            Sj, Yj = s["S"][j][:n].double(), s["Y"][j][:n]
            if first:
                g0, b0 = self.g0
                ey = (Yj.double() - (s["g_c"][:n].double() - g0)).abs()
                if not bool((ey <= b0 + U23 * (g0.abs() + s["g_c"][:n].double().abs())).all()):
                    _fail(2, f"Y[{j}] != g_c,1 - g(x_0) within the bound of one evaluation")
            elif not torch.equal(Yj, y32):
                _fail(2, f"Y[{j}] != g_c,i - g_c,i-1 ({int((Yj != y32).sum())} elements differ)")
            if d0 is not None:
                big = d0.abs() > 2.0 ** -20 * float(d0.abs().max())
                k = int(d0.abs().argmax())
                t = float(Sj[k]) / float(d0[k])
                ratio = (Sj / d0)[big]
                if not bool(((ratio - t).abs() <= U22 * abs(t)).all()):
                    _fail(2, f"S[{j}] / d_(i-1) is not one scalar: t {t:.9g}, worst relative deviation "
                             f"{float(((ratio - t).abs() / abs(t)).max()):.3e}")
                if not bool(((Sj - t * d0).abs() <= U22 * (t * d0).abs() + 1e-45).all()):
                    _fail(2, f"S[{j}] != fl32(t d_(i-1))")
            # x_i = fl32(x_(i-1) + t d), S = fl32(t d): one rounding each
            if not bool(((x1 - (x0 + Sj)).abs() <= U23 * torch.maximum(x1.abs(), Sj.abs()) + 1e-45).all()):
                _fail(2, f"S[{j}] != x_i - x_(i-1) to one rounding of each")
            if j in self.live:
                if len(self.live) < H:
                    _fail(2, f"live slot {j} overwritten with only {len(self.live)} of {H} pairs live")
                if j != self.live[0]:
                    _fail(2, f"slot {j} overwritten, the oldest live pair is in slot {self.live[0]}")
                self.live.pop(0)
                self.wraps += 1
            elif len(self.live) >= H:
                _fail(2, "a free slot was written with H pairs live")
            self.live.append(j)
            self.pushes += 1
        if s["dir_reset"] > prev["dir_reset"]:
            self.live = []
        # ---- link 3 ----
        S64 = [s["S"][j][:n].double() for j in self.live]
        Y64 = [s["Y"][j][:n].double() for j in self.live]
        d64, tol = direction_tolerance(S64, Y64, s["g_c"][:n].double(), seed=self.seed + self.steps)
        dmax = float(d64.abs().max())
        err = float((s["d"][:n].double() - d64).abs().max())
        self.dir_tol.append((tol / dmax, err / tol if tol > 0 else 0.0))
        if not tol <= 1e-3 * dmax:
            _fail(3, f"input condition: the measured tolerance {tol:.3e} exceeds 1e-3 max|d| = {1e-3 * dmax:.3e}")
        if not err <= tol:
            _fail(3, f"d differs from the float64 two-loop over {len(self.live)} live pairs by {err:.3e} "
                     f"(tolerance {tol:.3e}, max|d| {dmax:.3e})")
        # ---- link 4 ----
        bt = (s["x"][:n].double() + s["d"][:n].double()).float()
        if not torch.equal(s["beta_t"][:n], bt):
            _fail(4, f"beta_t != fl32(x + 1.0 d) at {int((s['beta_t'][:n] != bt).sum())} elements")
        if current is not None:
            self.check_current(s, current)
        self.prev = s

    def check_current(self, s, current):
        n = self.p.n
        w64 = self.p.finalize(s["x"][:n].double(), s["wfix"][:n].double())
        top = float(w64.abs().max())
        err = (current.double() - w64).abs()
        if not bool((err <= U22 * w64.abs() + self.p.K * U24 * top).all()):
            i = int(err.argmax())
            _fail(4, f"current()[{i}] = {float(current[i]):.9g}, float64 finalisation {float(w64[i]):.9g}")

    def report(self):
        tol = max((a for a, _ in self.dir_tol), default=0.0)
        frac = max((b for _, b in self.dir_tol), default=0.0)
        return (f"steps {self.steps} pushes {self.pushes} declined {self.declined} wraps {self.wraps} "
                f"grad err/bound {self.grad_ratio:.3f} dir tol/max|d| {tol:.2e} dir err/tol {frac:.3f}")


# ---- the objective in the fitters' layouts -------------------------------------------------------
class DenseProblem:
    """Vectors of ``BatchFitter``: [K][Fp] coefficients then K intercepts (n), padded to nv."""

    def __init__(self, spec, ds, reg, center=None):
        from _fit_cases import eval_oracle
        from psx.models.reference import feature_std

        self._oracle = eval_oracle
        self.spec, self.ds, self.reg = spec, ds, float(reg)
        self.K, self.F, self.Fp = spec.K, spec.F, spec.Fp
        self.n = spec.K * spec.Fp + spec.K
        self.nv = (self.n + 63) // 64 * 64
        self.center = (reg == 0.0) if center is None else center
        self.sigma = feature_std(ds.X[: ds.rows, : spec.F].double())
        live = self.sigma > 0
        self.inv = torch.where(live, 1.0 / torch.where(live, self.sigma, torch.ones_like(self.sigma)),
                               torch.zeros_like(self.sigma))
        pad = torch.zeros(self.nv, dtype=torch.bool)
        pad[: spec.K * spec.Fp].view(spec.K, spec.Fp)[:, spec.F:] = True
        pad[self.n:] = True
        self.pad = pad

    def unpack(self, v):
        K, F, Fp = self.K, self.F, self.Fp
        return v[: K * Fp].view(K, Fp)[:, :F], v[K * Fp: K * Fp + K]

    def pack(self, c, b):
        v = torch.zeros(self.n, dtype=torch.float64)
        v[: self.K * self.Fp].view(self.K, self.Fp)[:, : self.F] = c
        v[self.K * self.Fp:] = b
        return v

    def coef_eff(self, x, wfix):
        c, b = self.unpack(x)
        wf, _ = self.unpack(wfix)
        return torch.where(self.sigma > 0, c * self.inv, wf), c, b

    def grad(self, x, wfix):
        ce, c, b = self.coef_eff(x, wfix)
        _, g, _, bg, _ = self._oracle(self.spec, self.ds, self.pack(ce, b))
        gc, gb = self.unpack(g)
        bc, bb = self.unpack(bg)
        g64 = self.pack(gc * self.inv + self.reg * c, gb)
        beta = self.pack(c, torch.zeros_like(b))
        return g64, self.pack(bc * self.inv, bb) + U23 * (g64.abs() + self.reg * beta.abs())

    def value(self, x, wfix):
        ce, c, b = self.coef_eff(x, wfix)
        return self._oracle(self.spec, self.ds, self.pack(ce, b))[0] + 0.5 * self.reg * float((c * c).sum())

    def finalize(self, x, wfix):
        ce, _, b = self.coef_eff(x, wfix)
        if self.center:
            ce = ce - ce.mean(0, keepdim=True)
        return self.pack(ce, b - b.mean())


class WideProblem:
    """Vectors of ``WideBatchFitter``: [U][KP] coefficients of the touched features
    then KP intercepts (n), padded to nv.  ``finalize`` returns the same compact
    layout (``current()`` scatters it through the sorted touched features)."""

    def __init__(self, spec, ds, reg, compact=False):
        """``compact``: the oracle works on a copy of the dataset whose feature ids are the
        ranks of the touched features (a model of U features): for an F too large to densify."""
        from _wide_fit_cases import csr64, eval_oracle, touched
        from psx.models.reference import feature_std
        from psx.models.wide import WideSpec
        from psx.ops.sparse import SparseDataset

        self._oracle = eval_oracle
        self.spec, self.ds, self.reg = spec, ds, float(reg)
        self.K, self.KP = spec.K, spec.KP
        self.f = touched(ds)
        self.U = int(self.f.numel())
        self.ospec, self.ods, self.of = spec, ds, self.f  # what the oracle sees
        if compact:
            rank = torch.searchsorted(self.f, ds.idx.long())
            self.ods = SparseDataset(ds.indptr, rank.to(torch.int32), ds.val, ds.y, self.U)
            self.ospec, self.of = WideSpec(self.U, spec.K), torch.arange(self.U)
        self.n = (self.U + 1) * spec.KP
        self.nv = (self.n + 63) // 64 * 64
        self.center = reg == 0.0
        self.sigma = feature_std(csr64(self.ods)[:, self.of])
        live = self.sigma > 0
        self.inv = torch.where(live, 1.0 / torch.where(live, self.sigma, torch.ones_like(self.sigma)),
                               torch.zeros_like(self.sigma))
        pad = torch.zeros(self.nv, dtype=torch.bool)
        pad[: self.n].view(self.U + 1, spec.KP)[:, spec.K:] = True
        pad[self.n:] = True
        self.pad = pad

    def unpack(self, v):  # -> [K, U], [K]
        m = v[: self.n].view(self.U + 1, self.KP)
        return m[: self.U, : self.K].t(), m[self.U, : self.K]

    def pack(self, c, b):
        v = torch.zeros(self.n, dtype=torch.float64)
        m = v.view(self.U + 1, self.KP)
        m[: self.U, : self.K] = c.t()
        m[self.U, : self.K] = b
        return v

    def coef_eff(self, x, wfix):
        c, b = self.unpack(x)
        wf, _ = self.unpack(wfix)
        return torch.where(self.sigma > 0, c * self.inv, wf), c, b

    def _full(self, c, b):
        s = self.ospec
        w = torch.zeros(s.P, dtype=torch.float64)
        w[: s.F * s.KP].view(s.F, s.KP)[self.of, : s.K] = c.t()
        w[s.F * s.KP: s.F * s.KP + s.K] = b
        return w

    def _compact(self, w):
        s = self.ospec
        return w[: s.F * s.KP].view(s.F, s.KP)[self.of, : s.K].t(), w[s.F * s.KP: s.F * s.KP + s.K]

    def grad(self, x, wfix):
        ce, c, b = self.coef_eff(x, wfix)
        _, g, _, bg, _ = self._oracle(self.ospec, self.ods, self._full(ce, b))
        gc, gb = self._compact(g)
        bc, bb = self._compact(bg)
        g64 = self.pack(gc * self.inv + self.reg * c, gb)
        beta = self.pack(c, torch.zeros_like(b))
        return g64, self.pack(bc * self.inv, bb) + U23 * (g64.abs() + self.reg * beta.abs())

    def value(self, x, wfix):
        ce, c, b = self.coef_eff(x, wfix)
        return self._oracle(self.ospec, self.ods, self._full(ce, b))[0] + 0.5 * self.reg * float((c * c).sum())

    def finalize(self, x, wfix):
        ce, _, b = self.coef_eff(x, wfix)
        if self.K > 1:
            if self.center:
                ce = ce - ce.mean(0, keepdim=True)
            b = b - b.mean()
        return self.pack(ce, b)

    def compact_current(self, w_full):
        """The compact layout of a full ``current()`` vector [F*KP + KP] (CPU)."""
        s = self.spec
        m = w_full[: s.F * s.KP].view(s.F, s.KP)[self.f]
        return torch.cat([m.reshape(-1), w_full[s.F * s.KP:]])


# ---- snapshots --------------------------------------------------------------------------------
def snapshot(nat, H, device, stream):
    """The native fitter's state as CPU tensors."""
    nv = int(nat.nv)
    t = {k: torch.empty(nv, dtype=torch.float32, device=device) for k in VECS}
    t["S"] = torch.empty(H, nv, dtype=torch.float32, device=device)
    t["Y"] = torch.empty(H, nv, dtype=torch.float32, device=device)
    nat.read_state(t["x"].data_ptr(), t["d"].data_ptr(), t["g_c"].data_ptr(), t["g_t"].data_ptr(),
                   t["beta_t"].data_ptr(), t["wfix"].data_ptr(), t["S"].data_ptr(), t["Y"].data_ptr(), stream)
    s = {k: v.cpu() for k, v in t.items()}
    s["dir_reset"] = int(nat.dir_reset)
    return s


def run_chain(nat, problem, H, steps, device, stream, w_out=None, current_of=None, seed=0):
    """Drive a begun native fitter ``steps`` accepted steps, checking every link after
    each; ``w_out`` (device) receives ``current()`` after the last step, mapped by
    ``current_of`` to the problem's layout.  -> the Chain (its report is printed by the caller)."""
    assert int(nat.nv) == problem.nv and int(nat.n) == problem.n
    ch = Chain(problem, H, seed=seed)
    ch.begin(snapshot(nat, H, device, stream))
    for i in range(steps):
        before = int(nat.accepted)
        ended = nat.run(1, stream)
        if ended or int(nat.accepted) != before + 1:
            break
        cur = None
        if w_out is not None:
            nat.current(w_out.data_ptr(), stream)
            cur = current_of(w_out.cpu())
        ch.step(snapshot(nat, H, device, stream), current=cur)
    return ch


def emulate(problem, x0, H, steps):
    """Snapshots of a float64 L-BFGS on ``problem`` rounded to fp32 where the device
    rounds: x, g_c, d, S, Y, beta_t; steps by Armijo backtracking from t = 1 (the first
    from 1/|g|); the ring is slot = push number mod H.  -> list of snapshots (begin first)."""
    n, nv = problem.n, problem.nv
    z = lambda: torch.zeros(nv, dtype=torch.float32)  # noqa: E731

    def put(v64):
        o = z()
        o[:n] = v64.float()
        return o

    wfix = z()
    x = put(x0)
    S, Y = torch.zeros(H, nv), torch.zeros(H, nv)
    snaps = [dict(x=x, d=z(), g_c=z(), g_t=z(), beta_t=x.clone(), wfix=wfix, S=S.clone(), Y=Y.clone(), dir_reset=0)]
    g = put(problem.grad(x[:n].double(), wfix[:n].double())[0])
    d = -g
    live, pushes = [], 0
    f = lambda v: problem.value(v[:n].double(), wfix[:n].double())  # noqa: E731
    t = 1.0 / float(g.double().norm())
    for _ in range(steps):
        f0, dg = f(x), float(g.double() @ d.double())
        while True:
            xn = put(x[:n].double() + t * d[:n].double())
            if f(xn) <= f0 + 1e-4 * t * dg:
                break
            t *= 0.5
        gn = put(problem.grad(xn[:n].double(), wfix[:n].double())[0])
        s32, y32 = put(t * d[:n].double()), gn - g
        j = pushes % H
        S[j], Y[j] = s32, y32
        if j in live:
            live.remove(j)
        live.append(j)
        pushes += 1
        x, g = xn, gn
        d = put(two_loop([S[k][:n].double() for k in live], [Y[k][:n].double() for k in live], g[:n].double()))
        bt = put(x[:n].double() + d[:n].double())
        snaps.append(dict(x=x, d=d, g_c=g, g_t=g.clone(), beta_t=bt, wfix=wfix, S=S.clone(), Y=Y.clone(), dir_reset=0))
        t = 1.0
    return snaps

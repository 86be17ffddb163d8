"""The solver controller's split form (solver_ctrl.h: ctrl_linesearch + ctrl_accept_ls /
ctrl_accept_terminal) against ctrl_step on identical randomised evaluation sequences.

The line search of the split form sees only (f, g.d); an accept in the last
iteration takes the entry that needs no dots, and `step` is then fed garbage in
every other dot to show it does not read them.  Every exposed field is compared
after every evaluation."""
import math
import random

import pytest

from psx._native import host

FIELDS = ("phase", "action", "action_slot", "iter", "m", "head", "push_slot", "nacc", "ls_fail", "evals", "ls_i",
          "zoom", "dir_reset", "t", "t_acc", "f_c", "f_init", "dg0", "gg_c", "gamma", "cg", "lo_t", "lo_f", "lo_d",
          "hi_t", "hi_f", "hi_d", "cs", "cy", "Sg", "Yg")


def _cfg(hist, iters, ls_max, nslots):
    c = host.SolverCfg()
    c.K, c.F, c.Fp, c.P, c.cap = 2, 4, 128, 10, 32
    c.iters, c.hist, c.ls_max, c.nslots = iters, hist, ls_max, nslots
    c.mode, c.center, c.zero_const, c.gd_lr, c.tol = 0, 1, 1, 1.0, 1e-6
    return c


def _state(c):
    out = {k: getattr(c, k) for k in FIELDS}
    # SY / YY: the whole arrays.  Only the entries of stored pairs are ever written; the
    # binding zeroes a new controller, so the rest compares equal too
    out["SY"], out["YY"] = list(c.SY), list(c.YY)
    return out


def _same(a, b):
    def eq(x, y):
        if isinstance(x, list):
            return len(x) == len(y) and all(eq(p, q) for p, q in zip(x, y))
        if isinstance(x, float):
            return x == y or (math.isnan(x) and math.isnan(y))
        return x == y

    return [k for k in a if not eq(a[k], b[k])]


def _run(rng, hist, iters, ls_max, nslots, seen):
    cfg = _cfg(hist, iters, ls_max, nslots)
    a, b = host.SolverCtrl(), host.SolverCtrl()
    nd = 3 + 2 * hist
    for slot in range(nslots):
        if a.phase == host.kPhDone:
            break
        # an objective value around the current one (mostly a decrease), sometimes not finite;
        # a slope of either sign; the gradient's other dots at random
        f = 1.0 if slot == 0 else a.f_c * rng.choice([0.5, 0.9, 0.999, 0.9999999, 1.0, 1.1, 3.0])
        kind = rng.random()
        if slot > 0 and kind < 0.08:
            f = rng.choice([float("nan"), float("inf"), 1e301])
        td = rng.choice([-1.0, -0.5, -0.01, 0.01, 0.4, 2.0]) * abs(a.dg0 if slot > 0 else 1.0) * rng.random()
        dots = [rng.uniform(0.1, 2.0), td, rng.uniform(-1.0, 1.0)] + [rng.uniform(-1.0, 1.0) for _ in range(2 * hist)]
        if slot == 0:  # evaluation 0 is the same entry in both forms
            a.step(cfg, f, dots, slot)
            b.step(cfg, f, dots, slot)
        else:
            was_zoom = b.zoom
            v = b.linesearch(cfg, f, td, slot)
            seen.add(("verdict", v))
            if was_zoom:
                seen.add("zoom")
            if v == host.kLsTrial and not was_zoom and not b.zoom and b.t > a.t and math.isfinite(f):
                seen.add("extension")
            if not math.isfinite(f) or abs(f) >= 1e300:
                seen.add("nonfinite")
            if slot + 1 >= nslots and v in (host.kLsSettle, host.kLsDone):
                seen.add("out_of_slots")
            adots = dots
            if v in (host.kLsAccept, host.kLsSettle):
                if b.accept_is_terminal(cfg):
                    b.accept_terminal(f, slot)
                    seen.add("terminal")
                    # step must not read any dot but g.d on this path
                    adots = [float("nan"), td, float("nan")] + [rng.choice([float("nan"), 1e300, -7.0])
                                                                  for _ in range(2 * hist)]
                else:
                    b.accept(cfg, f, dots, slot, v)
                    seen.add("continue")
            a.step(cfg, f, adots, slot)
        diff = _same(_state(a), _state(b))
        assert not diff, (hist, iters, ls_max, nslots, slot, diff)
    assert a.evals == b.evals <= nslots


@pytest.mark.parametrize("hist", [1, 10])
def test_split_controller_equals_step(hist):
    rng = random.Random(1234 + hist)
    seen = set()
    for iters in (1, 2, 3):
        for ls_max in (1, 2, 3, 4):
            full = 1 + iters * ls_max
            for nslots in {full, max(2, full - 1), max(2, full - 2)}:
                for _ in range(150):
                    _run(rng, hist, iters, ls_max, nslots, seen)
    want = {"zoom", "extension", "nonfinite", "out_of_slots", "terminal", "continue", ("verdict", host.kLsTrial),
            ("verdict", host.kLsAccept), ("verdict", host.kLsSettle), ("verdict", host.kLsDone)}
    assert want <= seen, want - seen


RESULT_FIELDS = ("iter", "nacc", "evals", "ls_fail", "action_slot", "t_acc", "f_c", "f_init")


@pytest.mark.parametrize("hist", [1, 10])
def test_out_of_slots_accept_by_the_terminal_entry(hist):
    """A caller that cannot continue may also take accept_terminal for an accept in the last
    slot of an EARLIER iteration (nslots below 1 + iters * ls_max; solver_ctrl.h,
    ctrl_accept_terminal_p).  There the two states differ: step still books the pair and the
    next direction (m, head, push_slot, gamma, dg0, dir_reset; action kActAccept after a
    Wolfe accept), which nothing can use.  What a solve reports must be equal all the same,
    and the split form must have ended."""
    rng = random.Random(99 + hist)
    hit = {host.kLsAccept: 0, host.kLsSettle: 0}
    for iters, ls_max, nslots in ((2, 2, 2), (3, 2, 3), (3, 3, 4), (3, 4, 3), (2, 4, 4)):
        cfg = _cfg(hist, iters, ls_max, nslots)
        for _ in range(300):
            a, b = host.SolverCtrl(), host.SolverCtrl()
            for slot in range(nslots):
                if a.phase == host.kPhDone:
                    break
                f = 1.0 if slot == 0 else a.f_c * rng.choice([0.5, 0.9, 0.999, 1.0, 1.1])
                td = rng.choice([-1.0, -0.5, -0.01, 0.01, 0.4, 2.0]) * abs(a.dg0 if slot > 0 else 1.0) * rng.random()
                dots = [rng.uniform(0.1, 2.0), td, rng.uniform(-1.0, 1.0)] + [rng.uniform(-1.0, 1.0)
                                                                              for _ in range(2 * hist)]
                a.step(cfg, f, dots, slot)
                if slot == 0:
                    b.step(cfg, f, dots, slot)
                    continue
                v = b.linesearch(cfg, f, td, slot)
                if v in (host.kLsAccept, host.kLsSettle):
                    if slot + 1 >= nslots and not b.accept_is_terminal(cfg):
                        b.accept_terminal(f, slot)
                        hit[v] += 1
                        assert b.phase == host.kPhDone and b.action == host.kActAcceptDone
                        sa, sb = _state(a), _state(b)
                        diff = [k for k in RESULT_FIELDS if sa[k] != sb[k]]
                        assert not diff, (iters, ls_max, nslots, slot, v, diff)
                        break
                    b.accept(cfg, f, dots, slot, v)
    assert hit[host.kLsAccept] > 0 and hit[host.kLsSettle] > 0, hit


def test_terminal_accept_state():
    """The dot-free accept leaves an ended solve: the accepted step, the trial's f, kActAcceptDone."""
    cfg = _cfg(10, 1, 4, 5)
    c = host.SolverCtrl()
    c.step(cfg, 1.0, [4.0, -4.0, 4.0] + [0.0] * 20, 0)
    assert c.action == host.kActInit and c.t == 0.5
    assert c.linesearch(cfg, 0.5, -0.1, 1) == host.kLsAccept
    assert c.accept_is_terminal(cfg)
    c.accept_terminal(0.5, 1)
    assert (c.phase, c.action, c.action_slot, c.iter, c.nacc, c.evals) == (host.kPhDone, host.kActAcceptDone, 1, 1, 1, 2)
    assert c.t_acc == 0.5 and c.f_c == 0.5

"""first_step / step_t / min_step / max_step in the fused dopri5 solves (csrc/dopri5.hip, cde_dopri_adj.h), against the
oracle's restatement of torchdiffeq's rules (oracle/odeint.py: _Dopri5.integrate):

  * every attempt's step size is clamped to [min_step, max_step] before it is planned and after the step-size update;
  * an attempt that would pass the next step time is clipped onto it, a jump time strictly inside takes over, and the
    step-time index moves on only when an accepted attempt was clipped onto a step time;
  * an attempt longer than max_step is rejected, one no longer than min_step accepted, whatever its error ratio;
  * first_step replaces Hairer's initial step (forward: once; backward: at the start of every output interval).

Forward: the attempt table read off the status blocks (tests/dopri5_forward_attempts.py), every plan re-derived here with
those rules, then replayed through the float64 oracle.  Backward: the kernels' own attempt trace.  The bars are the ones of
test_gpu_13_adaptive_forward_attempts.py and test_gpu_02_adaptive_backward.py: error ratios within 0.02 r + 0.01 (two-layer
relu fields: 97 % of the attempts), the oracle's decisions wherever |r - 1| > 0.03 -- after the forced accept / reject --,
controller arithmetic to 1e-12, trajectories 1e-4 / 2e-5 (float32) and 1e-7 / 1e-8 (float64), gradients rtol 1e-3 and
atol 1e-4 max|g|.  A case proves a rule only if the rule fires: every case must show, in the KERNEL's table, an accepted
attempt clipped onto a step time, an attempt planned at exactly max_step and one no longer than min_step."""
import bisect
import math
import warnings

import pytest
import torch

import dopri5_forward_attempts as dfa
from gpu_common import (_front, oracle_cde, oracle_interp, LinearField, _TwoLayerField, _TricksFunc, make_series, DEV, _close,
                        _oracle_solver_log)
from oracle import odeint as oracle_ode

pytestmark = pytest.mark.gpu

T_OUT = [0., 2.6, 7.]
# the four options together: on a Hermite-cubic control, and on a linear one with jump_t on its knots
CUBIC = dict(first_step=0.1, min_step=0.15, max_step=0.45, step_t=[0.7, 1.9, 2.6, 3.3, 5.0, 9.0])
LINEAR = dict(first_step=0.3, min_step=0.05, max_step=0.35, step_t=[0.5, 1.5, 2.25, 4.75])


# the two-layer field of these tests takes shorter steps: bounds that bite there (forward; backward over a shorter span,
# the float64 oracle's replay of a two-layer backward being slow)
MLP = dict(first_step=0.1, min_step=0.08, max_step=0.25, step_t=[0.7, 1.9, 2.6, 3.3, 5.0, 9.0])
MLP_BACK = dict(first_step=0.02, min_step=0.008, max_step=0.02, step_t=[0.1, 0.25, 0.45, 0.55])
T_SHORT = [0., 0.3, 0.6]


def _case(H, C, tanh, degree, *, B=37, width=None, dtype=torch.float32, variant="auto", tuning=None, opts=None, seed=7,
          t_out=T_OUT):
    opts = opts or (CUBIC if degree == 3 else LINEAR)
    return dict(t_out=t_out, H=H, C=C, tanh=tanh, degree=degree, B=B, L=8, width=width, dtype=dtype, variant=variant, tuning=tuning or {},
                opts=opts, jumps=degree == 1, seed=seed, tol=(1e-4, 1e-6))


# one case per consumer of the forward controller (which kernel a case runs: `dopri5_advance`, csrc/dopri5.hip).  The
# pending error sums are readable in all of them: the forms in which a workgroup's waves share a tile run a single tile.
FORWARD = {
    "generic_f64": _case(20, 5, True, 3, dtype=torch.float64),
    # min_step above what the solve needs in places: attempts whose error ratio is above 1 are accepted all the same
    "generic_f64_large_min_step": _case(20, 5, True, 3, dtype=torch.float64, opts=dict(CUBIC, min_step=0.3)),
    "mfma_split_one_tile": _case(32, 8, True, 3, B=13),
    "mfma_128_by_option": _case(32, 8, True, 3, B=130, tuning=dict(k4_no_split=1)),
    "wide_64x8": _case(64, 8, True, 3),
    "two_layer_one_wave_per_tile": _case(32, 8, True, 3, width=128, tuning=dict(k4m_no_split=1), opts=MLP),
    "two_layer_split_one_tile": _case(32, 8, True, 3, B=13, width=128, opts=MLP),
    "wide_40x6_linear_jumps_and_steps": _case(40, 6, False, 1),
}


def _make_field(cfg, dtype):
    if cfg["width"] is None:
        return LinearField(cfg["H"], cfg["C"], dtype, scale=0.3, tanh=cfg["tanh"], seed=7)
    return _TwoLayerField(cfg["H"], cfg["C"], cfg["width"], dtype, seed=3)


def _problem(native, cfg):
    B, L, C, H, dtype = cfg["B"], cfg["L"], cfg["C"], cfg["H"], cfg["dtype"]
    x = make_series(B, L, C, dtype, seed=cfg["seed"])
    coeffs = oracle_interp.hermite_bdiff_coeffs(x) if cfg["degree"] == 3 else x
    Xo = (oracle_interp.CubicPath if cfg["degree"] == 3 else oracle_interp.LinearPath)(coeffs.double())
    X = None
    if native is not None:
        X = (native.CubicSpline if cfg["degree"] == 3 else native.LinearInterpolation)(coeffs.to(DEV))
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(cfg["seed"]), dtype=torch.float64).to(dtype)
    return X, Xo, z0, torch.tensor(cfg["t_out"], dtype=dtype), (Xo.grid_points.double() if cfg["jumps"] else None)


def _solve_forward(native, monkeypatch, cfg, chunk=1):
    X, Xo, z0, t_out, jump_t = _problem(native, cfg)
    options = dict(cfg["opts"])
    if cfg["jumps"]:
        options["jump_t"] = X.grid_points
    func = _make_field(cfg, cfg["dtype"]).to(DEV)
    with native.tuning(**cfg["tuning"]):
        got = dfa.run(native, monkeypatch, _front(), X, func, z0.to(DEV), t_out.to(DEV), read_sums=True,
                      mlp=cfg["width"] is not None, tanh=cfg["tanh"], variant=cfg["variant"], chunk=chunk,
                      path="dopri5_forward" if cfg["width"] is None else "mlp_dopri5_forward", options=options,
                      rtol=cfg["tol"][0], atol=cfg["tol"][1])
    return Xo, z0, t_out, jump_t, got


# ------------------------------------------------------------------ torchdiffeq's rules, restated
def _clamp(dt, lo, hi):
    if not math.isfinite(dt):
        dt = lo
    return min(max(dt, lo), hi)


def _kept(times, t_first):
    """The times a solve keeps (>= its start, sorted) and the index it starts at."""
    kept = sorted(v for v in times if v >= t_first)
    return kept, (min(bisect.bisect(kept, t_first), len(kept) - 1) if kept else 0)


def _plan(t0, dt, steps, i_step, jumps, i_jump):
    """(t1, dt, on_step, on_jump) of an attempt of clamped size dt from t0."""
    t1, on_step, on_jump = t0 + dt, False, False
    if steps and t0 < steps[i_step] < t0 + dt:
        on_step, t1 = True, steps[i_step]
        dt = t1 - t0
    if jumps and t0 < jumps[i_jump] < t0 + dt:
        on_jump, on_step, t1 = True, False, jumps[i_jump]
        dt = t1 - t0
    return t1, dt, on_step, on_jump


def _decide(ratio, dt, lo, hi):
    accept = ratio <= 1
    if dt > hi:
        accept = False
    if dt <= lo:
        accept = True
    return accept


def _check_forward_controller(att, t_out, jump_t, opts):
    """Every plan and decision of the forward solve from the status blocks, with the new rules; returns how often each fired."""
    st, rows, n = att.statuses, att.rows, len(att)
    lo, hi = opts.get("min_step", 0.0), opts.get("max_step", math.inf)
    assert [s.phase for s in st] == [1, 2] + [3] * n + [4]
    tt = t_out.double().tolist()
    steps, i_step = _kept(opts.get("step_t", []), tt[0])
    jumps, i_jump = _kept([] if jump_t is None else jump_t.tolist(), tt[0])
    if "first_step" in opts:
        assert st[2].dt == _clamp(opts["first_step"], lo, hi)                      # exactly
    fired = dict(step_clips=0, at_max=0, at_min=0, forced_accepts=0, forced_rejects=0, jump_clips=0)
    i_out = 1
    for j in range(n):
        plan, done = st[2 + j], st[3 + j]
        t0, t1, on_jump, accepted, _ = rows[j].tolist()
        where = "attempt %d of %d" % (j, n)
        assert plan.i_out == i_out and plan.i_jump == i_jump, where
        assert plan.dt == _clamp(plan.dt, lo, hi), (where, plan.dt)                # clamped before it is planned
        want_t1, dt, on_step, want_jump = _plan(t0, plan.dt, steps, i_step, jumps, i_jump)
        assert t1 == want_t1 and plan.dt_try == dt and bool(on_jump) == want_jump, (where, t1, want_t1)    # bit for bit
        assert t1 > t0, where
        ratio = att.ratio(j)
        accept = _decide(ratio, dt, lo, hi)
        assert bool(accepted) == accept, (where, ratio, dt)
        assert done.n_accept + done.n_reject == j + 1 and done.t_lo == t0 and done.t_hi == (t1 if accept else t0), where
        fired["at_max"] += dt == hi
        fired["at_min"] += dt <= lo
        fired["forced_accepts"] += accept and ratio > 1
        fired["forced_rejects"] += (not accept) and ratio <= 1
        if accept:
            while i_out < len(tt) and not (tt[i_out] > t1):
                i_out += 1
            fired["step_clips"] += on_step
            fired["jump_clips"] += want_jump
            if on_step and i_step != len(steps) - 1:
                i_step += 1
            if want_jump and i_jump != len(jumps) - 1:
                i_jump += 1
        assert done.i_out == i_out, where
        want = _clamp(plan.dt_try * dfa.next_factor(ratio), lo, hi)
        assert abs(done.dt - want) <= 1e-12 * want, (where, done.dt, want)
    assert i_out == len(tt) and st[-1].n_accept + st[-1].n_reject == n
    assert (att.stats["n_accept"], att.stats["n_reject"]) == (st[-1].n_accept, st[-1].n_reject)
    assert att.stats["launches"] == n + 3
    # the trace keeps its meaning: the third value is "clipped onto a JUMP time"
    assert torch.equal(att.stats["steps"], rows[rows[:, 3] != 0][:, :3])
    return fired


def _assert_fired(fired, where):
    assert fired["step_clips"] >= 1, "%s: no accepted attempt was clipped onto a step time %r" % (where, fired)
    assert fired["at_max"] >= 1, "%s: no attempt was planned at exactly max_step %r" % (where, fired)
    assert fired["at_min"] >= 1, "%s: no attempt with dt <= min_step %r" % (where, fired)


@pytest.mark.parametrize("name", sorted(FORWARD))
def test_forward_attempts_follow_the_step_options(native, monkeypatch, name):
    cfg = FORWARD[name]
    opts = cfg["opts"]
    lo, hi = opts["min_step"], opts["max_step"]
    Xo, z0, t_out, jump_t, att = _solve_forward(native, monkeypatch, cfg)
    fired = _check_forward_controller(att, t_out, jump_t, opts)
    print("%s: %d attempts, %r" % (name, len(att), fired))
    _assert_fired(fired, name)
    if cfg["jumps"]:
        assert fired["jump_clips"] >= 1
    # ---- the float64 oracle re-makes every attempt from its own state
    field = oracle_ode._Field(oracle_cde.ControlledField(Xo, _make_field(cfg, torch.float64)))
    solver = oracle_ode._Dopri5(field, z0.double(), cfg["tol"][0], cfg["tol"][1], oracle_ode._rms, replay_attempts=att.replay())
    with torch.no_grad():
        ref = solver.integrate(t_out.double()).permute(1, 0, 2)
    assert len(solver.ratios) == len(att)
    inside = []
    for j, r in enumerate(solver.ratios):
        mine = att.ratio(j)
        inside.append(abs(mine - r) <= 0.02 * r + 0.01)
        if abs(r - 1) > 0.03:
            dt = att.statuses[2 + j].dt_try
            assert bool(att.rows[j, 3]) == _decide(r, dt, lo, hi), "attempt %d: oracle ratio %.5g, kernel %.5g" % (j, r, mine)
    if cfg["width"] is not None:
        assert sum(inside) >= 0.97 * len(inside), "%d of %d error ratios match the oracle's" % (sum(inside), len(inside))
    else:
        assert all(inside), "error ratio of attempt %d leaves the band" % inside.index(False)
    if cfg["dtype"] == torch.float64:
        _close(att.out, ref, 1e-7, 1e-8)
    else:
        _close(att.out, ref, 1e-4, 2e-5)
    if name == "generic_f64_large_min_step":
        assert fired["forced_accepts"] >= 1, "no forced accept of an attempt whose ratio is above 1: %r" % fired
    if cfg["dtype"] == torch.float64:
        # float64: the oracle's own controller, free-running with the options, takes the same accepted and rejected sequence
        free = oracle_ode._Dopri5(field, z0.double(), cfg["tol"][0], cfg["tol"][1], oracle_ode._rms, **opts)
        with torch.no_grad():
            free_out = free.integrate(t_out.double()).permute(1, 0, 2)
        assert (free.n_accept, free.n_reject) == (att.stats["n_accept"], att.stats["n_reject"])
        theirs = torch.tensor(free.accepted, dtype=torch.float64)
        mine = att.rows[att.rows[:, 3] != 0][:, :3]
        assert torch.equal(mine[:, 2], theirs[:, 2])
        _close(mine[:, :2], theirs[:, :2], 1e-9, 1e-12)
        _close(att.out, free_out, 1e-7, 1e-8)


def test_forward_solve_with_step_options_does_not_depend_on_the_launch_window(native, monkeypatch):
    """The carried state of the options (step-time index, whether the pending attempt was clipped) ping-pongs with the launch
    parity: windows of 1, 7 and 48 launches give the same bits and the same attempts."""
    cfg = FORWARD["wide_40x6_linear_jumps_and_steps"]
    res = {}
    for chunk in (1, 7, 48):
        got = _solve_forward(native, monkeypatch, cfg, chunk=chunk)[-1]
        out, stats = (got.out, got.stats) if chunk == 1 else got
        res[chunk] = (out, stats["n_accept"], stats["n_reject"], stats["steps"])
        assert stats["launches"] % chunk == 0 and stats["launches"] >= stats["n_accept"] + stats["n_reject"] + 3
    for chunk in (7, 48):
        assert res[chunk][1:3] == res[1][1:3]
        assert torch.equal(res[chunk][3], res[1][3])
        assert torch.equal(res[chunk][0], res[1][0])


# ------------------------------------------------------------------ backward
def _reversed_times(times):
    """torchdiffeq's view of step_t in a reversed-time solve: `-torch.as_tensor(step_t).flip(0)` -- a list of Python floats
    becomes a float32 tensor on the way."""
    return (-torch.as_tensor(times)).flip(0).double().tolist() if len(times) else []


ADJ_OTHER = dict(first_step=0.2, min_step=0.1, max_step=0.5, step_t=[1.1, 3.3, 4.2, 6.5])
BACKWARD = {
    "k4a_tanh_cubic": _case(20, 5, True, 3),
    "k4a_identity_linear_jumps": _case(32, 8, False, 1),
    "k4a_explicit_adjoint_options": dict(_case(20, 5, True, 3), adj=ADJ_OTHER),
    # (its step time 3.4, not CUBIC's 3.3: from 3.3 -- as float32, which is how a reversed solve reads a list -- two forced
    #  steps of min_step end at 2.99999995, which the kernel's float32 stage times round ONTO the knot at 3 and torchdiffeq's
    #  "just before t1" then puts on the other side of it than the float64 oracle's; the two error estimates of that one
    #  attempt then belong to different pieces of the control -- 0.030 against 168 -- with or without the control block)
    "k4a_control_block": dict(_case(32, 8, False, 3, opts=dict(CUBIC, step_t=[0.7, 1.9, 2.6, 3.4, 5.0, 9.0])), control=True),
    "k4am_relu_8_channels": _case(32, 8, True, 3, B=19, width=128, opts=MLP_BACK, t_out=T_SHORT),
    "k4am_relu_16_channels": _case(8, 14, True, 1, B=19, width=64, opts=MLP_BACK, t_out=T_SHORT),
}


def _check_backward_attempts(attempts, s0, opts, jump_s):
    """One output interval's attempt trace (t0, t1, on_jump, accepted, ratio) in reversed time against the rules.  The trace
    holds no step sizes: a planned size is known exactly where it is first_step or a bound of the clamp, else to the
    1e-6 of the update rule's check in test_gpu_02 (one float32 ratio through a float64 pow)."""
    lo, hi = opts.get("min_step", 0.0), opts.get("max_step", math.inf)
    steps, i_step = _kept(_reversed_times(opts.get("step_t", [])), s0)
    jumps, i_jump = _kept([] if jump_s is None else jump_s, s0)
    fired = dict(step_clips=0, at_max=0, at_min=0, forced_accepts=0, forced_rejects=0, jump_clips=0)
    dt_plan = _clamp(opts["first_step"], lo, hi) if "first_step" in opts else None
    assert attempts[0, 0] == s0
    for n, (t0, t1, on_jump, accepted, ratio) in enumerate(attempts.tolist()):
        where = "attempt %d of %d" % (n, len(attempts))
        dt = t1 - t0
        exact = dt_plan is not None and (n == 0 or dt_plan in (lo, hi))
        on_step = False
        if dt_plan is not None:
            want_t1, want_dt, on_step, want_jump = _plan(t0, dt_plan, steps, i_step, jumps, i_jump)
            if on_step or want_jump:
                assert t1 == want_t1 and bool(on_jump) == want_jump, (where, t1, want_t1)        # clips: bit for bit
            elif exact:
                assert t1 == want_t1 and on_jump == 0, (where, t1, want_t1)
            else:
                assert abs(dt - want_dt) <= 1e-6 * want_dt + 1e-12 and on_jump == 0, (where, dt, want_dt)
            if not (on_step or want_jump):
                assert lo * (1 - 1e-12) <= dt <= hi * (1 + 1e-12), (where, dt)
        # (the trace holds t0 and t1, not the planned size: t1 - t0 of an attempt planned at a bound is a rounding off it)
        short = dt <= lo or t1 == t0 + lo
        accept = _decide(ratio, min(dt, hi) if dt <= hi * (1 + 1e-12) else dt, lo, hi) or short
        assert bool(accepted) == accept, (where, ratio, dt)
        fired["at_max"] += t1 == t0 + hi
        fired["at_min"] += short
        fired["forced_accepts"] += accept and ratio > 1
        if accept:
            fired["step_clips"] += on_step
            fired["jump_clips"] += bool(on_jump)
            if on_step and i_step != len(steps) - 1:
                i_step += 1
            if on_jump and i_jump != len(jumps) - 1:
                i_jump += 1
        factor = 10.0 if ratio == 0 else min(10.0, max(0.9 / ratio ** 0.2, 1.0 if ratio < 1 else 0.2))
        dt_plan = _clamp(dt * factor, lo, hi)
    return fired


@pytest.mark.parametrize("name", sorted(BACKWARD))
def test_backward_attempts_follow_the_step_options(native, name):
    """Every backward attempt against the rules (from the kernels' own trace), then replayed through the float64 oracle for
    error ratios, decisions and all gradients."""
    cfg = BACKWARD[name]
    front = _front()
    mlp, control = cfg["width"] is not None, cfg.get("control", False)
    B, H, kw = cfg["B"], cfg["H"], dict(rtol=cfg["tol"][0], atol=cfg["tol"][1])
    x = make_series(B, cfg["L"], cfg["C"], seed=cfg["seed"])
    base = oracle_interp.hermite_bdiff_coeffs(x) if cfg["degree"] == 3 else x
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(cfg["seed"]))
    t_out = torch.tensor(cfg["t_out"])
    lw = torch.rand(B, 3, H, generator=torch.Generator().manual_seed(3)) + 0.5
    func = _make_field(cfg, torch.float32).to(DEV)
    coeffs = base.to(DEV).requires_grad_(control)
    X = (native.CubicSpline if cfg["degree"] == 3 else native.LinearInterpolation)(coeffs)
    zd = z0.to(DEV).requires_grad_(True)
    options = dict(cfg["opts"])
    if cfg["jumps"]:
        options["jump_t"] = X.grid_points
    call = dict(options=options)
    if "adj" in cfg:
        call["adjoint_options"] = dict(cfg["adj"])
    if control:
        call["adjoint_params"] = tuple(func.parameters()) + (coeffs,)
    backward_opts = cfg.get("adj", cfg["opts"])             # adjoint_options=None: the forward options are the backward's
    front.record_dopri5_steps = True
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = native.cdeint(X, func, zd, t_out.to(DEV), **call, **kw)
        assert not any("step-wise" in str(w.message) for w in caught)
        path = front.last_dispatch()[0].path
        assert path == ("mlp_dopri5_adjoint" if mlp else "dopri5_adjoint"), path
        fwd = dict(front.last_dopri5_stats)
        (out * lw.to(DEV)).sum().backward()
        bwd = dict(front.last_dopri5_adjoint_stats)
    finally:
        front.record_dopri5_steps = False
    assert len(bwd["attempts"]) == 2
    jump_s = sorted(-v for v in X.grid_points.tolist()) if (cfg["jumps"] and "adj" not in cfg) else None
    total = dict(step_clips=0, at_max=0, at_min=0, forced_accepts=0, forced_rejects=0, jump_clips=0)
    lo, hi = backward_opts["min_step"], backward_opts["max_step"]
    for attempts, s0 in zip(bwd["attempts"], (-float(t_out[2]), -float(t_out[1]))):
        first = _clamp(backward_opts["first_step"], lo, hi)
        t1 = float(attempts[0, 1])
        assert t1 == s0 + first or float(attempts[0, 2]) == 1 or t1 in _reversed_times(backward_opts["step_t"]), (t1, s0, first)
        fired = _check_backward_attempts(attempts, s0, backward_opts, jump_s)
        for key in total:
            total[key] += fired[key]
    print("%s: %r" % (name, total))
    _assert_fired(total, name)

    f64 = _make_field(cfg, torch.float64)
    c64 = base.double().clone().requires_grad_(control)
    Xo = (oracle_interp.CubicPath if cfg["degree"] == 3 else oracle_interp.LinearPath)(c64)
    zo = z0.double().requires_grad_(True)
    extra = dict(adjoint_params=tuple(f64.parameters()) + (c64,)) if control else {}
    with _oracle_solver_log() as solvers:
        ref = oracle_cde.cdeint(Xo, f64, zo, t_out.double(), adjoint=True, method="dopri5",
                                options=dict(replay_steps=fwd["steps"]),
                                adjoint_options=dict(replay_attempts=[a.clone() for a in bwd["attempts"]]), **extra, **kw)
        (ref * lw.double()).sum().backward()
    assert len(solvers) == 3
    for attempts, solver in zip(bwd["attempts"], solvers[1:]):
        mine, theirs = attempts[:, 4], torch.tensor(solver.ratios, dtype=torch.float64)
        assert len(mine) == len(theirs) > 0
        inside = (mine - theirs).abs() <= 0.02 * theirs + 0.01
        if mlp:
            assert inside.double().mean() >= 0.97, "only %.1f %% of the error ratios match the oracle's" % (100 * inside.double().mean())
        else:
            assert inside.all(), "error ratio of attempt %d: kernel %.5g, oracle %.5g" % (
                int((~inside).nonzero()[0]), mine[~inside][0], theirs[~inside][0])
        for n in torch.nonzero(inside & ((theirs - 1).abs() > 0.03)).flatten().tolist():
            t0, t1 = float(attempts[n, 0]), float(attempts[n, 1])
            want = _decide(float(theirs[n]), min(t1 - t0, hi) if t1 - t0 <= hi * (1 + 1e-12) else t1 - t0, lo, hi) or t1 == t0 + lo
            assert bool(attempts[n, 3]) == want, (n, float(theirs[n]), t1 - t0)
    _close(out, ref, 1e-4, 2e-5)
    pairs = [(zd.grad, zo.grad)] + [(p.grad, q.grad) for p, q in zip(func.parameters(), f64.parameters())]
    if control:
        pairs.append((coeffs.grad, c64.grad))
    for got, want in pairs:
        assert got is not None
        _close(got, want, 1e-3, 1e-4 * want.abs().max().item())


# ------------------------------------------------------------------ step-wise, and the refusals that stay
def test_stepwise_path_takes_the_step_options(native):
    """A field no kernel recognises, all four options: forward and gradients against the float64 oracle, at the bars of
    test_stepwise_path_arbitrary_func_vs_oracle (two tolerance-level adaptive solutions: 1e-3 / 1e-4, gradients 1e-2 / 1e-3)."""
    B, L, C, H, dtype = 6, 6, 3, 8, torch.float64
    x = make_series(B, L, C, dtype, seed=17)
    coeffs = oracle_interp.hermite_bdiff_coeffs(x)
    z0 = torch.randn(B, H, dtype=dtype, generator=torch.Generator().manual_seed(17))
    kw = dict(adjoint=True, rtol=1e-5, atol=1e-7, options=dict(first_step=0.05, min_step=0.01, max_step=0.4, step_t=[0.9, 2.5, 4.1]))
    fo = _TricksFunc(C, H, dtype)
    zo = z0.clone().requires_grad_(True)
    Xo = oracle_interp.CubicPath(coeffs)
    ref = oracle_cde.cdeint(Xo, fo, zo, Xo.interval, **kw)
    ref[:, -1].pow(2).sum().backward()
    fd = _TricksFunc(C, H, dtype).to(DEV)
    X = native.CubicSpline(coeffs.to(DEV))
    zd = z0.to(DEV).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = native.cdeint(X, fd, zd, X.interval, **kw)
    assert _front().last_dispatch()[0].path == "stepwise"
    out[:, -1].pow(2).sum().backward()
    _close(out, ref, 1e-3, 1e-4)
    _close(zd.grad, zo.grad, 1e-2, 1e-3)
    for pd, po in zip(fd.parameters(), fo.parameters()):
        _close(pd.grad, po.grad, 1e-2, 1e-3 * max(1.0, po.grad.abs().max().item()))


def test_refusals_that_stay(native):
    from torchcde_amd import distributed
    front = _front()
    cfg = FORWARD["mfma_split_one_tile"]
    X, _, z0, t_out, _ = _problem(native, cfg)
    func = _make_field(cfg, torch.float32).to(DEV)
    with distributed.shared_step_control(cfg["B"], reduce=lambda sums: None):
        for key, value in CUBIC.items():
            with pytest.raises(NotImplementedError, match="shared_step_control"):
                with torch.no_grad():
                    native.cdeint(X, func, z0.to(DEV), t_out.to(DEV), options={key: value})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.no_grad():
            native.cdeint(X, func, z0.to(DEV), t_out.to(DEV), options=dict(max_num_steps=10 ** 6, max_step=0.5))
    assert front.last_dispatch()[0].path == "stepwise"

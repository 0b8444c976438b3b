"""The adaptive FORWARD solve (csrc/dopri5.hip) pinned to torchdiffeq attempt by attempt, on every kernel form.

The backward kernels trace every attempt; the forward kernels trace accepted steps only, so rejected attempts, the step-size
update, the clipping onto jump times and Hairer's first step were compared with nothing.  They are all in the controller's
status block: with one launch per look at it (tests/dopri5_forward_attempts.py) the blocks are the complete attempt list,
and the float64 oracle (oracle/odeint.py: _Dopri5 with `replay_attempts`) re-makes every attempt from ITS OWN state at t0,
so a kernel's error estimate, decision, step-size update and dense output are each compared with torchdiffeq's.

Which kernel a case runs follows from the launcher, `dopri5_advance` (csrc/dopri5.hip:1141-1242); every case names the lines.
Bars (none of them measured on the kernels):
  * error ratio per attempt: |r_kernel - r_oracle| <= 0.02 r_oracle + 0.01, the band of the backward tests
    (test_gpu_02_adaptive_backward.py); all attempts, except two-layer relu fields: 97 % of them (relu kinks, as there);
  * decisions: accepted == (r_oracle <= 1) wherever |r_oracle - 1| > 0.03;
  * controller arithmetic: exact, the step-size update to 1e-12 (one `pow` and one division in float64);
  * Hairer's first step: 1e-3; trajectories: rtol 1e-4 / atol 2e-5 in float32, 1e-7 / 1e-8 in float64 (the replay bars).
"""
import bisect
import math
import time

import pytest
import torch

import dopri5_forward_attempts as dfa
from gpu_common import (_front, oracle_cde, oracle_interp, LinearField, _TwoLayerField, make_series, DEV, _close)
from test_gpu_10_softplus_field import _SoftplusField

pytestmark = pytest.mark.gpu

_T3, _T3J, _T3S, _T4 = [0., 2.6, 7.], [0., 3.5, 7.], [0., 2.6, 5.], [0., 2.6, 2.6001, 7.]


def _case(H, C, tanh, degree, jumps=False, *, sums, B=37, L=8, t_out=_T3, width=None, field="affine", dtype=torch.float32,
          variant="auto", tuning=None, tol=(1e-4, 1e-6), long=False):
    return dict(H=H, C=C, tanh=tanh, degree=degree, jumps=jumps, sums=sums, B=B, L=L, t_out=t_out, width=width, field=field,
                dtype=dtype, variant=variant, tuning=tuning or {}, tol=tol, long=long)


# `sums`: the pending error sums are readable (the kernel's grid is dopri_grid(form, n), dopri5.hip:1094-1096).  The forms in
# which the eight waves of a workgroup share one tile (:1214-1219 two-layer, :1236-1239 one-layer) launch a workgroup per
# tile; their ratio is recovered from the step-size update -- unless the batch is one tile (the long controls: B = 5).
_LONG = dict(B=5, L=9001, t_out=[8990., 8995.5, 9000.], long=True)
CASES = {
    # ---- one-layer, generic kernel (:1180-1188; float64 always, float32 under variant="generic": dopri_use_mfma :1069-1072)
    "generic_f32": _case(20, 5, True, 3, variant="generic", sums=True),
    "generic_f64": _case(20, 5, True, 3, dtype=torch.float64, tol=(1e-5, 1e-7), sums=True),
    # ---- one-layer, 32 x 8 MFMA, the eight waves of a workgroup share a tile: up to 256 tiles (:1236, :1238-1239)
    "mfma_split_identity_cubic": _case(32, 8, False, 3, sums=False),
    "mfma_split_tanh_linear_crossing_kinks": _case(20, 5, True, 1, sums=False),           # no jump_t: steps cross the knots
    "mfma_split_dense_two_outputs_in_a_step": _case(32, 8, False, 3, t_out=_T4, sums=False),
    # ---- one-layer, 32 x 8 MFMA, 128-series workgroups (:1240): by option, and by itself beyond 256 tiles
    "mfma_128_by_option": _case(32, 8, True, 3, B=130, tuning=dict(k4_no_split=1), sums=True),
    "mfma_128_at_4100": _case(32, 8, True, 3, B=4100, L=6, t_out=_T3S, sums=True),        # 257 tiles, 33 workgroups
    # ---- one-layer, wide kernel (:1190-1199): 8 waves x 2 blocks up to 8 channels, 4 x 4 beyond (:1197)
    "wide_64x8_tanh_cubic": _case(64, 8, True, 3, sums=True),
    "wide_40x6_identity_linear_jumps": _case(40, 6, False, 1, True, sums=True),
    "wide_32x16_identity_cubic_interval": _case(32, 16, False, 3, t_out=None, sums=True),
    "wide_12x11_tanh_linear_jumps": _case(12, 11, True, 1, True, t_out=_T3J, sums=True),
    "wide_dense_two_outputs_in_a_step": _case(64, 8, True, 3, t_out=_T4, sums=True),
    # the tile loop of a workgroup (dopri_wide_grid :1077-1080): 257 tiles over 256 workgroups, 513 over 512
    "wide_64x8_tile_loop_4100": _case(64, 8, True, 3, B=4100, L=6, t_out=_T3S, sums=True),
    "wide_12x11_tile_loop_8200": _case(12, 11, False, 1, True, B=8200, L=6, t_out=_T3S, sums=True),
    # ---- two-layer field (:1202-1224): shared tiles (:1218) / one wave per tile (:1220); 16-channel tiles and the upper
    # half of the output layer (:1222)
    "two_layer_split": _case(32, 8, True, 3, B=130, width=128, field="relu", sums=False),
    "two_layer_one_wave_per_tile": _case(32, 8, True, 3, B=130, width=128, field="relu", tuning=dict(k4m_no_split=1),
                                         sums=True),
    "two_layer_16_channels_linear_jumps": _case(16, 14, True, 1, True, t_out=_T3J, width=64, field="relu", sums=False),
    "two_layer_upper_half_32x14": _case(32, 14, True, 1, t_out=None, width=128, field="relu", sums=False),
    "two_layer_softplus": _case(32, 8, True, 3, B=130, width=128, field="softplus", tuning=dict(k4m_no_split=1), sums=True),
    # ---- controls longer than the LDS knot buffers (:366-367; the knots then come from global memory, :429-431), jump_t on
    # all 9001 knots: the controller skips the 8990 before t[0] (c.pad, :122-129)
    "long_mfma_32x8": _case(32, 8, True, 1, True, sums=True, **_LONG),
    "long_wide_48x6": _case(48, 6, True, 1, True, sums=True, **_LONG),
    "long_two_layer_16x6x64": _case(16, 6, True, 1, True, width=64, field="relu", sums=True, **_LONG),
}
_PATHS = {"affine": "dopri5_forward", "relu": "mlp_dopri5_forward", "softplus": "mlp_dopri5_forward"}


def _field(cfg, dtype):
    H, C = cfg["H"], cfg["C"]
    if cfg["field"] == "affine":
        return LinearField(H, C, dtype, scale=0.3, tanh=cfg["tanh"], seed=7)
    return (_SoftplusField if cfg["field"] == "softplus" else _TwoLayerField)(H, C, cfg["width"], dtype, seed=3)


def _problem(native, name):
    """The case's inputs: the control both sides see (the SAME coefficients: the oracle's path takes them as float64), z0,
    output times, jump times."""
    cfg = CASES[name]
    B, L, C, H, dtype = cfg["B"], cfg["L"], cfg["C"], cfg["H"], cfg["dtype"]
    seed = len(name)
    if cfg["long"]:                       # the construction of test_long_controls_beyond_the_lds_knot_buffers
        x = (torch.randn(B, L, C, generator=torch.Generator().manual_seed(9)) * 0.02).cumsum(-2)
    else:
        x = make_series(B, L, C, dtype, seed=seed)
    coeffs = oracle_interp.hermite_bdiff_coeffs(x) if cfg["degree"] == 3 else x
    X = (native.CubicSpline if cfg["degree"] == 3 else native.LinearInterpolation)(coeffs.to(DEV))
    Xo = (oracle_interp.CubicPath if cfg["degree"] == 3 else oracle_interp.LinearPath)(coeffs.double())
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)
    t_out = Xo.interval.to(dtype) if cfg["t_out"] is None else torch.tensor(cfg["t_out"], dtype=dtype)
    jump_t = Xo.grid_points.double() if cfg["jumps"] else None
    return cfg, X, Xo, z0, t_out, jump_t


def _solve(native, monkeypatch, name, chunk=1):
    cfg, X, Xo, z0, t_out, jump_t = _problem(native, name)
    call = dict(rtol=cfg["tol"][0], atol=cfg["tol"][1])
    if cfg["jumps"]:
        call["options"] = dict(jump_t=X.grid_points)
    func = _field(cfg, cfg["dtype"]).to(DEV)
    with native.tuning(**cfg["tuning"]):
        got = dfa.run(native, monkeypatch, _front(), X, func, z0.to(DEV), t_out.to(DEV), read_sums=cfg["sums"],
                      mlp=cfg["field"] != "affine", tanh=cfg["tanh"], variant=cfg["variant"], chunk=chunk,
                      path=_PATHS[cfg["field"]], **call)
    return cfg, Xo, z0, t_out, jump_t, got


def _check_controller(cfg, att, t_out, jump_t):
    """Assertion 3: everything the controller does between two attempts, from the status blocks alone."""
    st, rows, n = att.statuses, att.rows, len(att)
    assert [s.phase for s in st] == [1, 2] + [3] * n + [4]
    tt = t_out.double().tolist()
    t_first = tt[0]
    kept, i_jump, pad = [], 0, 0
    if jump_t is not None:                                   # torchdiffeq: the jump times >= t[0], sorted; bisect from t[0]
        allj = sorted(jump_t.tolist())
        pad = sum(1 for v in allj if v < t_first)
        kept = allj[pad:]
        i_jump = min(bisect.bisect(kept, t_first), len(kept) - 1)
    assert all(s.pad == pad for s in st)
    i_out = 1
    for j in range(n):
        plan, done = st[2 + j], st[3 + j]
        t0, t1, on_jump, accepted, factor = rows[j].tolist()
        where = "attempt %d of %d" % (j, n)
        # ---- the plan: from the current t_hi, one dt long unless the next kept jump time lies strictly inside
        assert plan.i_out == i_out and plan.i_jump == i_jump, where
        dt = plan.dt
        clip = bool(kept) and t0 < kept[i_jump] < t0 + dt
        if clip:
            assert t1 == kept[i_jump] and on_jump == 1 and plan.dt_try == t1 - t0, where      # bit for bit
        else:
            assert t1 == t0 + dt and on_jump == 0 and plan.dt_try == dt, where
        assert t1 > t0, where
        # ---- the decision and what it moves
        assert accepted in (0.0, 1.0) and done.n_accept + done.n_reject == j + 1, where
        assert done.t_lo == t0 and done.t_hi == (t1 if accepted else t0), where
        if accepted:
            while i_out < len(tt) and not (tt[i_out] > t1):
                i_out += 1
            if on_jump and i_jump != len(kept) - 1:
                i_jump += 1
        assert done.i_out == i_out, where
        # ---- the step-size update (torchdiffeq: safety 0.9, ifactor 10, dfactor 0.2 -- or 1 below ratio 1 --, exponent 1/5)
        if att.sums is not None:
            ratio = att.ratio(j)
            assert bool(accepted) == (ratio <= 1), (where, ratio)                  # in the state's dtype
            want = plan.dt_try * dfa.next_factor(ratio)
            assert abs(done.dt - want) <= 1e-12 * want, (where, done.dt, want)
        else:
            if accepted:
                assert 1 - 1e-12 <= factor <= dfa.IFACTOR * (1 + 1e-12), (where, factor)
            else:
                assert dfa.DFACTOR * (1 - 1e-12) <= factor < dfa.SAFETY, (where, factor)
    assert i_out == len(tt) and st[-1].i_out == len(tt)
    assert st[-1].n_accept + st[-1].n_reject == n
    last = rows[rows[:, 3] != 0][-1]
    assert last[1] >= tt[-1] and (rows[rows[:, 3] != 0][:-1, 1] < tt[-1]).all()
    # ---- the trace of accepted steps and the statistics of the call
    assert (att.stats["n_accept"], att.stats["n_reject"]) == (st[-1].n_accept, st[-1].n_reject)
    assert att.stats["launches"] == n + 3
    assert torch.equal(att.stats["steps"], rows[rows[:, 3] != 0][:, :3])


def _check_first_step(att, solver):
    """Assertion 4 (1e-3 against the oracle), and where the sums are readable Hairer's rule on the kernel's own sums
    (dopri5.hip:130-156; float32 `powf` and a division the compiler may form as a reciprocal: 1e-5)."""
    st = att.statuses
    first = float(solver.first_dt)
    assert abs(st[2].dt - first) <= 1e-3 * first, (st[2].dt, first)
    if att.sums is not None:
        T = att.dtype
        cast = lambda v: torch.tensor(v, dtype=torch.float64).to(T)                     # noqa: E731
        d0, d1 = cast(math.sqrt(att.sums[0][0] / att.n_elems)), cast(math.sqrt(att.sums[0][1] / att.n_elems))
        h0 = cast(1e-6) if (d0 < 1e-5 or d1 < 1e-5) else cast(0.01) * d0 / d1
        assert abs(st[1].h0 - float(h0)) <= 1e-5 * float(h0), (st[1].h0, float(h0))
        assert st[2].h0 == st[1].h0
        d2 = cast(math.sqrt(att.sums[1][0] / att.n_elems)) / cast(st[1].h0)
        h1 = (cast(0.01) / torch.max(d1, d2)) ** 0.2
        want = float(torch.min(100 * cast(st[1].h0), h1))
        assert abs(st[2].dt - want) <= 1e-5 * want, (st[2].dt, want)


def _check_ratios(name, cfg, att, solver):
    """Assertions 1 and 2.  Returns the worst deviation as a fraction of the band."""
    theirs = solver.ratios
    assert len(theirs) == len(att)
    devs = []
    for j, r in enumerate(theirs):
        band = 0.02 * r + 0.01
        lo, hi = att.ratio_bounds(j)
        if att.sums is not None:
            mine = att.ratio(j)
            # (the exact ratio and the one the step-size update implies are the same number)
            assert lo * (1 - 1e-9) - 1e-300 <= mine <= hi * (1 + 1e-9), (j, mine, lo, hi)
            lo = hi = mine
        devs.append(max(lo - r, r - hi, 0.0) / band)
        if abs(r - 1) > 0.03:
            assert bool(att.rows[j, 3]) == (r <= 1), "attempt %d: oracle ratio %.5g, the kernel %s it (ratio in [%.5g, %.5g])" % (
                j, r, "accepted" if att.rows[j, 3] else "rejected", lo, hi)
    devs = torch.tensor(devs)
    inside = (devs <= 1).double().mean().item()
    worst = int(devs.argmax())
    print("%s: %d attempts (%d accepted / %d rejected), worst ratio deviation %.3f of the band (attempt %d, oracle %.5g), "
          "%.1f %% inside" % (name, len(att), att.stats["n_accept"], att.stats["n_reject"], devs.max(), worst, theirs[worst],
                              100 * inside))
    if cfg["field"] == "relu":
        assert inside >= 0.97, "only %.1f %% of the attempts' error ratios match the oracle's" % (100 * inside)
    else:
        assert devs.max() <= 1, "error ratio of attempt %d: oracle %.5g, kernel in [%s]" % (
            worst, theirs[worst], ", ".join("%.5g" % v for v in att.ratio_bounds(worst)))
    return float(devs.max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_attempts_are_torchdiffeqs(native, monkeypatch, name):
    """Every attempt of the forward solve -- rejected ones included -- against the float64 oracle re-making it from its own
    state: error ratio, decision, step-size update, clipping onto jump times, output bookkeeping, Hairer's first step, the
    accepted-step trace, and the trajectory at every output time (those inside steps through the dense output)."""
    from oracle import odeint as oracle_ode
    started = time.time()
    cfg, Xo, z0, t_out, jump_t, att = _solve(native, monkeypatch, name)
    solved = time.time()
    _check_controller(cfg, att, t_out, jump_t)
    if "dense" in name:                                     # one accepted step emits two outputs
        assert max(b.i_out - a.i_out for a, b in zip(att.statuses[2:], att.statuses[3:])) >= 2
    if cfg["long"]:
        assert att.statuses[0].pad == 8990
    f64 = _field(cfg, torch.float64)
    field = oracle_ode._Field(oracle_cde.ControlledField(Xo, f64))
    solver = oracle_ode._Dopri5(field, z0.double(), cfg["tol"][0], cfg["tol"][1], oracle_ode._rms,
                                replay_attempts=att.replay())
    with torch.no_grad():
        ref = solver.integrate(t_out.double()).permute(1, 0, 2)
    assert (solver.n_accept, solver.n_reject) == (att.stats["n_accept"], att.stats["n_reject"])
    _check_ratios(name, cfg, att, solver)
    _check_first_step(att, solver)
    if cfg["dtype"] == torch.float64:
        _close(att.out, ref, 1e-7, 1e-8)
    else:
        _close(att.out, ref, 1e-4, 2e-5)
    print("%s: native solve %.2f s, checks and oracle %.2f s" % (name, solved - started, time.time() - solved))


@pytest.mark.parametrize("name", ["generic_f32", "mfma_128_by_option", "wide_12x11_tanh_linear_jumps",
                                  "two_layer_16_channels_linear_jumps"])
def test_forward_solve_does_not_depend_on_the_launch_window(native, monkeypatch, name):
    """cde_dopri5_advance's launch window (`first_launch`, `n_launches`: the parity of the two controller blocks, the image
    built by the first window only, idle launches after the end) at 1, 7 and the front end's 48 launches per window: the
    same bits, the same attempts."""
    res = {}
    for chunk in (1, 7, 48):
        got = _solve(native, monkeypatch, name, chunk=chunk)[-1]
        out, stats = (got.out, got.stats) if chunk == 1 else got
        res[chunk] = (out, stats["n_accept"], stats["n_reject"], stats["steps"])
        assert stats["launches"] % chunk == 0 and stats["launches"] >= stats["n_accept"] + stats["n_reject"] + 3
    for chunk in (7, 48):
        assert res[chunk][1:3] == res[1][1:3], (chunk, res[chunk][1:3], res[1][1:3])
        assert torch.equal(res[chunk][3], res[1][3])
        assert torch.equal(res[chunk][0], res[1][0])

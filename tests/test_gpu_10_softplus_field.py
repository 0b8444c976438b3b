"""The two-layer vector field with a softplus hidden layer, f(z) = act(W2 softplus(W1 z + b1) + b2), on every fused path the
relu field has (fields.py recognises it, the kernels take the hidden activation in bits 4-7 of `act`).  Shapes, references
and bars are those of the relu field's tests (test_gpu_06_rk4.py, test_gpu_02_adaptive_backward.py)."""
import sys
import warnings

import pytest
import torch

from gpu_common import (_front, _expect_dispatch, oracle_cde, oracle_interp, _TwoLayerField, make_series, DEV, _close,
                        _oracle_solver_log)

pytestmark = pytest.mark.gpu


class _SoftplusField(_TwoLayerField):
    def forward(self, t, z):
        y = self.linear2(torch.nn.functional.softplus(self.linear1(z)))
        if self.final_tanh:
            y = y.tanh()
        return y.view(*z.shape[:-1], self.H, self.C)


def _paths(native, coeffs, degree):
    path64 = (oracle_interp.CubicPath if degree == 3 else oracle_interp.LinearPath)(coeffs.double())
    path32 = (oracle_interp.CubicPath if degree == 3 else oracle_interp.LinearPath)(coeffs)
    X = (native.CubicSpline if degree == 3 else native.LinearInterpolation)(coeffs.to(DEV))
    return path64, path32, X


_RK4_REFERENCE = {}


def _rk4_reference(H, C, width, degree, final_tanh):
    """float64 and CPU-float32 oracle solutions of one shape, computed once and shared (never modified)."""
    key = (H, C, width, degree, final_tanh)
    if key not in _RK4_REFERENCE:
        B, L, seed = 203, 24, 71
        x = make_series(B, L, C, torch.float32, seed=seed)
        coeffs = oracle_interp.hermite_bdiff_coeffs(x) if degree == 3 else x
        gen = torch.Generator().manual_seed(seed + 1)
        z0 = torch.randn(B, H, generator=gen)
        t_out = torch.tensor([0., 7.5, 23.])
        lw = torch.rand(B, 3, H, generator=gen) + 0.5
        res = {}
        for dtype in (torch.float64, torch.float32):
            f = _SoftplusField(H, C, width, dtype, seed=5, final_tanh=final_tanh)
            path = (oracle_interp.CubicPath if degree == 3 else oracle_interp.LinearPath)(coeffs.to(dtype))
            zc = z0.to(dtype).clone().requires_grad_(True)
            out = oracle_cde.cdeint(path, f, zc, t_out.to(dtype), adjoint=True, method="rk4", options=dict(step_size=1.0))
            (out * lw.to(dtype)).sum().backward()
            res[dtype] = dict(out=out.detach(), z=zc.grad, params={n: p.grad for n, p in f.named_parameters()})
        _RK4_REFERENCE[key] = (coeffs, z0, t_out, lw, res)
    return _RK4_REFERENCE[key]


@pytest.mark.parametrize("H,C,width,degree,final_tanh,chunk_bytes,one_wave", [
    (32, 8, 128, 3, True, None, False), (32, 8, 128, 3, True, None, True),       # (second: k2m_no_split / k3m_no_split)
    (12, 16, 64, 1, False, 1, False),                                              # 16 x 16 tiles, one sweep launch per step
    (20, 9, 52, 1, False, None, False),                                            # the upper half, width no multiple of 16
    (8, 3, 100, 3, False, None, False)])
def test_softplus_field_rk4_forward_and_adjoint_fused(native, H, C, width, degree, final_tanh, chunk_bytes, one_wave):
    """K2m + K3m with the softplus hidden layer against the float64 oracle: trajectories, dL/dz0 and all four parameter
    gradients with the bars of test_two_layer_field_adjoint_fused (trajectories rtol 1e-4, atol max(5e-6, 4x the CPU-float32
    error); gradients rtol 1e-3 of the largest entry, or 4x the CPU-float32 error), and against the step-wise path running
    the user's module (close, not bitwise equal: two code paths ran)."""
    from torchcde_amd import fields
    cdeint_mod = sys.modules["torchcde_amd.cdeint"]
    coeffs, z0, t_out, lw, res = _rk4_reference(H, C, width, degree, final_tanh)
    ref, cpu32 = res[torch.float64], res[torch.float32]

    def bar(want, c32):
        return max(1e-3 * want.abs().max().item(), 4 * (c32.double() - want).abs().max().item())

    dfunc = _SoftplusField(H, C, width, seed=5, final_tanh=final_tanh).to(DEV)
    X = _paths(native, coeffs, degree)[2]
    found, _ = fields.probe(dfunc, t_out[0].to(DEV), z0.to(DEV))
    assert found is not None and found.kind == "mlp2" and found.hidden_act == 1
    z = z0.to(DEV).requires_grad_(True)
    budget = cdeint_mod._MlpPlan.scratch_budget
    options = dict(k2m_no_split=1, k3m_no_split=1) if one_wave else {}
    try:
        if chunk_bytes is not None:
            cdeint_mod._MlpPlan.scratch_budget = chunk_bytes
        with native.tuning(**options):
            out = native.cdeint(X, dfunc, z, t_out.to(DEV), method="rk4", options=dict(step_size=1.0))
            _expect_dispatch("two_layer_rk4", out)
            (out * lw.to(DEV)).sum().backward()
    finally:
        cdeint_mod._MlpPlan.scratch_budget = budget
    worst = (out.detach().double().cpu() - ref["out"]).abs().max().item()
    print("trajectory: max abs error %.3g (CPU float32: %.3g)" % (worst, (cpu32["out"].double() - ref["out"]).abs().max().item()))
    _close(out, ref["out"], 1e-4, max(5e-6, 4 * (cpu32["out"].double() - ref["out"]).abs().max().item()))
    _close(z.grad, ref["z"], 1e-3, bar(ref["z"], cpu32["z"]))
    for name, p in dfunc.named_parameters():
        assert p.grad is not None and p.grad.shape == ref["params"][name].shape, name
        _close(p.grad, ref["params"][name], 1e-3, bar(ref["params"][name], cpu32["params"][name]))
    with torch.no_grad():
        stepwise = native.cdeint(X, dfunc, z0.to(DEV), t_out.to(DEV), method="rk4", options=dict(step_size=1.0),
                                 variant="generic")
    _close(out, stepwise, 1e-4, 5e-6)
    assert not torch.equal(out.detach(), stepwise)


def test_softplus_field_both_branches_of_the_hidden_layer(native):
    """Pre-activations above torch's threshold of 20 (softplus(x) = x) and below -15 (softplus(x) = exp(x) to float32
    precision): `linear1` scaled by 12, so both sets are hit at the initial state already (asserted in float64 on the CPU)."""
    H, C, width, B, L = 32, 8, 128, 203, 24
    x = make_series(B, L, C, torch.float32, seed=61)
    coeffs = oracle_interp.hermite_bdiff_coeffs(x)
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(62))
    t_out = torch.tensor([0., 7.5, 23.])

    def field(dtype):
        f = _SoftplusField(H, C, width, dtype, seed=3, final_tanh=True)
        with torch.no_grad():
            f.linear1.weight.mul_(12.0)
            f.linear1.bias.mul_(12.0)
        return f

    f64 = field(torch.float64)
    with torch.no_grad():
        pre = f64.linear1(z0.double())
        assert (pre > 20).any() and (pre < -15).any()
        path64, path32, X = _paths(native, coeffs, 3)
        ref = oracle_cde.cdeint(path64, f64, z0.double(), t_out.double(), adjoint=False, method="rk4", options=dict(step_size=1.0))
        cpu32 = oracle_cde.cdeint(path32, field(torch.float32), z0, t_out, adjoint=False, method="rk4", options=dict(step_size=1.0))
        out = native.cdeint(X, field(torch.float32).to(DEV), z0.to(DEV), t_out.to(DEV), method="rk4", options=dict(step_size=1.0))
    assert _front().last_dispatch()[0].path == "mlp_rk4_forward"          # fused, not step-wise
    _close(out, ref, 1e-4, max(5e-6, 4 * (cpu32.double() - ref).abs().max().item()))


@pytest.mark.parametrize("control_grad", [False, True])
def test_softplus_field_backprop_mode_fused_against_autograd_through_the_oracle(native, control_grad):
    """adjoint=False under rk4 (K2m storing its stages, K3m's sweep as reverse mode), once with the coefficient tensor
    requiring a gradient; against autograd through the float64 oracle, bars as for the relu field."""
    H, C, width, B, L, seed = 32, 8, 128, 203, 12, 71
    x = make_series(B, L, C, torch.float32, seed=seed)
    base = oracle_interp.hermite_bdiff_coeffs(x)
    gen = torch.Generator().manual_seed(seed + 1)
    z0 = torch.randn(B, H, generator=gen)
    t_out = torch.tensor([0., 2.0, 4.5, 11.])
    lw = torch.rand(B, 4, H, generator=gen) + 0.5
    kw = dict(method="rk4", options=dict(step_size=1.0), adjoint=False)
    res = {}
    for dtype in (torch.float64, torch.float32):
        f = _SoftplusField(H, C, width, dtype, seed=5, final_tanh=True)
        co = base.to(dtype).clone().requires_grad_(control_grad)
        zc = z0.to(dtype).clone().requires_grad_(True)
        out = oracle_cde.cdeint(oracle_interp.CubicPath(co), f, zc, t_out.to(dtype), **kw)
        (out * lw.to(dtype)).sum().backward()
        res[dtype] = [out.detach(), zc.grad, co.grad] + [p.grad for p in f.parameters()]

    def bar(want, cpu32):
        return max(1e-3 * want.abs().max().item(), 4 * (cpu32.double() - want).abs().max().item())

    dfunc = _SoftplusField(H, C, width, seed=5, final_tanh=True).to(DEV)
    cd = base.to(DEV).clone().requires_grad_(control_grad)
    z = z0.to(DEV).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # in particular: no step-wise warning
        out = native.cdeint(native.CubicSpline(cd), dfunc, z, t_out.to(DEV), **kw)
    if control_grad:
        _expect_dispatch("two_layer_rk4_backprop_control", out)
    else:
        _expect_dispatch("two_layer_rk4_backprop", out)
    (out * lw.to(DEV)).sum().backward()
    got = [out.detach(), z.grad, cd.grad] + [p.grad for p in dfunc.parameters()]
    _close(got[0], res[torch.float64][0], 1e-4, 5e-6)
    for g_, want, cpu32 in zip(got[1:], res[torch.float64][1:], res[torch.float32][1:]):
        if want is None:
            assert g_ is None
            continue
        _close(g_, want, 1e-3, bar(want, cpu32))


@pytest.mark.parametrize("case,form", [("example_model", "split"), ("example_model", "one_wave_per_tile"),
                                       ("multi_out_jumps", "split")])
def test_softplus_field_default_call_runs_fused_with_torchdiffeqs_decisions(native, case, form):
    """cdeint(X, func, z0, times) -- dopri5 + adjoint -- with the softplus field: forward K4, backward K4am, every backward
    attempt re-made by the float64 oracle; the criteria of test_two_layer_default_call_runs_fused_with_torchdiffeqs_decisions
    (>= 97 % of the error ratios within 2 % + 0.01, decisions equal where clear, first step within 1e-3 / 2e-2, trajectories
    1e-4 / 2e-5, gradients 2e-3).  The field is smooth, so no attempt has a kink to blame for leaving the band.
    Observed share inside the band: not recorded yet -- the test prints it per interval (run with -s)."""
    front = _front()
    cfg = {"example_model": dict(B=70, L=7, C=8, H=32, width=128, degree=3, t_out=None, jumps=False),
           "multi_out_jumps": dict(B=150, L=9, C=4, H=16, width=64, degree=1, t_out=[0., 3.5, 8.], jumps=True)}[case]
    B, L, C, H, kw = cfg["B"], cfg["L"], cfg["C"], cfg["H"], dict(rtol=1e-4, atol=1e-6)
    seed = len(case)
    x = make_series(B, L, C, seed=seed)
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(seed))
    t_out = None if cfg["t_out"] is None else torch.tensor(cfg["t_out"])
    n_t = 2 if t_out is None else t_out.numel()
    lw = torch.rand(B, n_t, H, generator=torch.Generator().manual_seed(3)) + 0.5
    func = _SoftplusField(H, C, cfg["width"], seed=3, final_tanh=True).to(DEV)
    X = (native.CubicSpline(native.hermite_cubic_coefficients_with_backward_differences(x.to(DEV))) if cfg["degree"] == 3
         else native.LinearInterpolation(native.linear_interpolation_coeffs(x.to(DEV))))
    zd = z0.to(DEV).requires_grad_(True)
    times = X.interval if t_out is None else t_out.to(DEV)
    opts = dict(options=dict(jump_t=X.grid_points)) if cfg["jumps"] else {}
    options = dict(k4am_no_small_reduce=1, k4am_no_split=1, k4m_no_split=1) if form == "one_wave_per_tile" else {}
    front.record_dopri5_steps = True
    try:
        with native.tuning(**options):
            out = native.cdeint(X, func, zd, times, **opts, **kw)
            _expect_dispatch("two_layer_dopri5", out)
            fwd = dict(front.last_dopri5_stats)
            (out * lw.to(DEV)).sum().backward()
            bwd = dict(front.last_dopri5_adjoint_stats)
    finally:
        front.record_dopri5_steps = False
    assert len(bwd["attempts"]) == n_t - 1 and bwd["n_accept"] > 0

    f64 = _SoftplusField(H, C, cfg["width"], torch.float64, seed=3, final_tanh=True)
    Xo = (oracle_interp.CubicPath(oracle_interp.hermite_bdiff_coeffs(x.double())) if cfg["degree"] == 3
          else oracle_interp.LinearPath(x.double()))
    zo = z0.double().requires_grad_(True)
    adj_opts = dict(replay_attempts=[a.clone() for a in bwd["attempts"]])
    with _oracle_solver_log() as solvers:
        ref = oracle_cde.cdeint(Xo, f64, zo, Xo.interval if t_out is None else t_out.double(), adjoint=True, method="dopri5",
                                options=dict(replay_steps=fwd["steps"]), adjoint_options=adj_opts, **kw)
        (ref * lw.double()).sum().backward()
    assert len(solvers) == n_t
    for attempts, solver in zip(bwd["attempts"], solvers[1:]):
        mine, theirs = attempts[:, 4], torch.tensor(solver.ratios, dtype=torch.float64)
        accepted = attempts[:, 3] != 0
        inside = (mine - theirs).abs() <= 0.02 * theirs + 0.01
        print("%s/%s: %d of %d attempts inside the band, %d rejected" % (case, form, int(inside.sum()), len(inside),
                                                                          int((~accepted).sum())))
        assert inside.double().mean() >= 0.97, "only %.1f %% of the attempts' error ratios match the oracle's" % (
            100 * inside.double().mean())
        clear = inside & ((theirs - 1).abs() > 0.03)
        assert torch.equal(accepted[clear], (theirs <= 1)[clear])
        assert torch.equal(accepted, mine <= 1)
        first = float(attempts[0, 1] - attempts[0, 0])
        assert abs(first - float(solver.first_dt)) <= (1e-3 if solver is solvers[1] else 2e-2) * float(solver.first_dt)
    _close(out, ref, 1e-4, 2e-5)
    _close(zd.grad, zo.grad, 2e-3, 1e-3 * zo.grad.abs().max().item())
    for (name, got), want in zip(func.named_parameters(), f64.parameters()):
        assert got.grad is not None, name
        _close(got.grad, want.grad, 2e-3, 2e-3 * want.grad.abs().max().item())

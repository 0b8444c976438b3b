"""cdeint(..., backend="torchsde", method="reversible_heun") on the GPU: the fused kernels (csrc/revheun.hip) and the step-wise
solve against the float64 restatement of the recurrences (tests/revheun_reference.py) and autograd through it.

Tolerances.  Trajectories: this file uses the second convention of tests/gpu_common.py for every shape -- rtol 1e-4 with
atol 1e-5, and the kernel's error at most 4x the error of the CPU float32 restatement, measured here (the method is only
neutrally stable: on the CPU, float32 already sits at 1.3x the plain 1e-4 / 1e-6 bar at the first shape).  Gradients: rtol
1e-3 of the largest entry (float32), 1e-8 (float64)."""
import functools

import pytest
import torch

from gpu_common import DEV, _TricksFunc, _close, _front
from helpers import LinearField, TwoLayerField, make_series
from oracle import interp as oracle_interp
import revheun_reference as ref

pytestmark = pytest.mark.gpu

SDE = dict(backend="torchsde", method="reversible_heun")
ENDS = "ends"
CASES = [
    (37, 12, 8, 32, 3, 1.0, ENDS),
    (33, 9, 3, 6, 3, 0.7, (0.0, 1.4, 2.5, 8.0)),     # steps cross knots, last step clipped, outputs on and between grid points
    (70, 24, 5, 20, 1, 0.5, ENDS),
    (1, 5, 1, 1, 1, 1.0, ENDS),
    (261, 6, 8, 32, 3, 1.0, (0.0, 2.0, 5.0)),        # more than one workgroup
]


def _times(L, times):
    return torch.tensor([0.0, float(L - 1)] if times == ENDS else list(times))


def _oracle_path(x, degree):
    return oracle_interp.CubicPath(oracle_interp.hermite_bdiff_coeffs(x)) if degree == 3 else oracle_interp.LinearPath(x)


def _native_path(native, x, degree):
    if degree == 3:
        return native.CubicSpline(native.hermite_cubic_coefficients_with_backward_differences(x.to(DEV)))
    return native.LinearInterpolation(native.linear_interpolation_coeffs(x.to(DEV)))


def _inputs(B, L, C, H, n_out):
    x = make_series(B, L, C, seed=7 + B)
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(8))
    lw = torch.rand(B, n_out, H, generator=torch.Generator().manual_seed(9)) + 0.5
    return x, z0, lw


@functools.lru_cache(maxsize=None)
def _reference(case, tanh):
    """float64 restatement with autograd gradients, and the float32 restatement's trajectory (computed once per case)."""
    B, L, C, H, degree, dt, times = case
    t = _times(L, times)
    x, z0, lw = _inputs(B, L, C, H, t.numel())
    f64 = LinearField(H, C, torch.float64, scale=0.3, tanh=tanh, seed=3)
    zo = z0.double().requires_grad_(True)
    out = ref.solve(_oracle_path(x.double(), degree), f64, zo, t.double(), dt)
    (out * lw.double()).sum().backward()
    with torch.no_grad():
        out32 = ref.solve(_oracle_path(x, degree), LinearField(H, C, scale=0.3, tanh=tanh, seed=3), z0, t, dt)
    return out.detach(), zo.grad, f64.linear.weight.grad, f64.linear.bias.grad, out32


def _fused(native, case, tanh, **kw):
    B, L, C, H, degree, dt, times = case
    t = _times(L, times)
    x, z0, lw = _inputs(B, L, C, H, t.numel())
    func = LinearField(H, C, scale=0.3, tanh=tanh, seed=3).to(DEV)
    X = _native_path(native, x, degree)
    z = z0.to(DEV).requires_grad_(True)
    out = native.cdeint(X, func, z, t.to(DEV), dt=dt, **{**SDE, **kw})
    assert _front().last_dispatch()[0].path == "reversible_heun"
    (out * lw.to(DEV)).sum().backward()
    return out.detach(), z.grad, func.linear.weight.grad, func.linear.bias.grad


def _trajectory_bar(got, want, cpu32, what=""):
    err = (got.double().cpu() - want).abs().max().item()
    floor = (cpu32.double() - want).abs().max().item()
    print("%s max |error|: kernel %.3g, CPU float32 restatement %.3g" % (what, err, floor))
    _close(got, want, 1e-4, 1e-5)
    assert err <= 4 * floor, "kernel error %.3g, CPU float32 error %.3g" % (err, floor)


@pytest.mark.parametrize("tanh", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_fused_reversible_heun_against_the_restatement(native, case, tanh):
    """RHf / RHa against the float64 recurrences and autograd through them, identity and tanh fields; a second identical call
    is bitwise equal in outputs and gradients (fixed-order reduction of the parameter gradients)."""
    want, gz, gw, gb, cpu32 = _reference(case, tanh)
    out, z_grad, w_grad, b_grad = _fused(native, case, tanh)
    assert out.shape == want.shape
    _trajectory_bar(out, want, cpu32, str(case))
    for got, exact in ((z_grad, gz), (w_grad, gw), (b_grad, gb)):
        print("gradient error / largest entry: %.3g" % ((got.double().cpu() - exact).abs().max() / exact.abs().max()).item())
        _close(got, exact, 1e-3, 1e-3 * exact.abs().max().item())
    again = _fused(native, case, tanh)
    for a, b in zip(again, (out, z_grad, w_grad, b_grad)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("tanh", [False, True])
def test_adjoint_false_and_the_spelled_out_adjoint_method_take_the_same_sweep(native, tanh):
    """adjoint=False asks for the gradient of the discrete solve, which is what the reconstructing sweep returns: bitwise the
    adjoint=True results.  So does adjoint_method="adjoint_reversible_heun" against leaving it away."""
    case = CASES[1]
    base = _fused(native, case, tanh)
    for kw in (dict(adjoint=False), dict(adjoint_method="adjoint_reversible_heun"),
               dict(adjoint_method="adjoint_reversible_heun", adaptive=False, adjoint_adaptive=False, options=None,
                    adjoint_options={}, rtol=1e-2, atol=1e-2)):
        for a, b in zip(_fused(native, case, tanh, **kw), base):
            assert torch.equal(a, b), kw


def test_fused_forward_without_gradients_and_a_parameter_subset(native):
    """no_grad: the same forward kernel, the same bits, no autograd node; adjoint_params naming the bias alone leaves the
    weight without a gradient; float64 output times on the float32 solve."""
    case = CASES[1]
    B, L, C, H, degree, dt, times = case
    t = _times(L, times)
    x, z0, lw = _inputs(B, L, C, H, t.numel())
    base = _fused(native, case, True)
    func = LinearField(H, C, scale=0.3, tanh=True, seed=3).to(DEV)
    X = _native_path(native, x, degree)
    with torch.no_grad():
        plain = native.cdeint(X, func, z0.to(DEV), t.to(DEV), dt=dt, **SDE)
    assert _front().last_dispatch()[0].path == "reversible_heun" and not plain.requires_grad
    assert torch.equal(plain, base[0])
    z = z0.to(DEV).requires_grad_(True)
    out = native.cdeint(X, func, z, t.to(DEV), dt=dt, adjoint_params=(func.linear.bias,), **SDE)
    assert _front().last_dispatch()[0].path == "reversible_heun"
    (out * lw.to(DEV)).sum().backward()
    assert func.linear.weight.grad is None
    assert torch.equal(func.linear.bias.grad, base[3]) and torch.equal(z.grad, base[1])
    with torch.no_grad():
        wide_t = native.cdeint(X, func, z0.to(DEV), t.double().to(DEV), dt=dt, **SDE)
    assert _front().last_dispatch()[0].path == "reversible_heun"
    _close(wide_t, plain, 1e-5, 1e-6)
    with pytest.raises(NotImplementedError, match="times"):
        native.cdeint(X, func, z0.to(DEV), t.to(DEV).requires_grad_(True), dt=dt, **SDE)


# ------------------------------------------------------------------------------------------------ step-wise coverage
def _stepwise_case(native, func64, func, dtype, B=19, L=7, C=3, H=6, degree=3, dt=0.7, times=(0.0, 1.4, 2.5, 6.0)):
    t = torch.tensor(times)
    x, z0, lw = _inputs(B, L, C, H, t.numel())
    zo = z0.double().requires_grad_(True)
    want = ref.solve(_oracle_path(x.double(), degree), func64, zo, t.double(), dt)
    (want * lw.double()).sum().backward()
    with torch.no_grad():
        cpu32 = ref.solve(_oracle_path(x, degree), func, z0, t, dt) if dtype == torch.float32 else None
    dev_func = func.to(DEV)
    X = _native_path(native, x.to(dtype), degree)
    z = z0.to(dtype).to(DEV).requires_grad_(True)
    out = native.cdeint(X, dev_func, z, t.to(dtype).to(DEV), dt=dt, **SDE)
    choice = _front().last_dispatch()[0]
    assert choice.path == "reversible_heun_stepwise" and choice.reason
    (out * lw.to(dtype).to(DEV)).sum().backward()
    return out.detach(), z.grad, want.detach(), zo.grad, cpu32


def _module_grads_close(dev_func, func64, rtol):
    for (name, p), q in zip(dev_func.named_parameters(), func64.parameters()):
        _close(p.grad, q.grad, rtol, rtol * q.grad.abs().max().item())


def test_stepwise_two_layer_field(native):
    f64 = TwoLayerField(6, 3, 16, torch.float64, seed=4)
    f32 = TwoLayerField(6, 3, 16, seed=4)
    out, gz, want, want_gz, cpu32 = _stepwise_case(native, f64, f32, torch.float32)
    _trajectory_bar(out, want, cpu32, "two-layer field")
    _close(gz, want_gz, 1e-3, 1e-3 * want_gz.abs().max().item())
    _module_grads_close(f32, f64, 1e-3)


def test_stepwise_unrecognised_module(native):
    f64, f32 = _TricksFunc(3, 6, torch.float64), _TricksFunc(3, 6, torch.float32)
    with torch.no_grad():
        f32.variable.copy_(f64.variable)           # (torch.rand draws different numbers for the two dtypes)
    out, gz, want, want_gz, cpu32 = _stepwise_case(native, f64, f32, torch.float32)
    _trajectory_bar(out, want, cpu32, "unrecognised module")
    _close(gz, want_gz, 1e-3, 1e-3 * want_gz.abs().max().item())
    _module_grads_close(f32, f64, 1e-3)


def test_stepwise_float64_affine_field(native):
    f64 = LinearField(6, 3, torch.float64, scale=0.3, tanh=True, seed=3)
    dev = LinearField(6, 3, torch.float64, scale=0.3, tanh=True, seed=3)
    out, gz, want, want_gz, _ = _stepwise_case(native, f64, dev, torch.float64)
    assert out.dtype == torch.float64
    _close(out, want, 1e-9, 1e-11)
    _close(gz, want_gz, 1e-8, 1e-8 * want_gz.abs().max().item())
    _module_grads_close(dev, f64, 1e-8)


@pytest.mark.parametrize("adjoint", [True, False])
def test_stepwise_control_gradient(native, adjoint):
    """A coefficient tensor that requires a gradient -- named in adjoint_params, or reached by autograd under adjoint=False --
    runs step-wise and gets a gradient within 1e-3 of the restatement's."""
    B, L, C, H, dt = 19, 7, 3, 6, 0.7
    t = torch.tensor([0.0, 1.4, 2.5, 6.0])
    x, z0, lw = _inputs(B, L, C, H, t.numel())
    co = oracle_interp.hermite_bdiff_coeffs(x.double()).requires_grad_(True)
    f64 = LinearField(H, C, torch.float64, scale=0.3, tanh=True, seed=3)
    want = ref.solve(oracle_interp.CubicPath(co), f64, z0.double(), t.double(), dt)
    (want * lw.double()).sum().backward()
    func = LinearField(H, C, scale=0.3, tanh=True, seed=3).to(DEV)
    coeffs = native.hermite_cubic_coefficients_with_backward_differences(x.to(DEV)).requires_grad_(True)
    X = native.CubicSpline(coeffs)
    kw = dict(adjoint_params=tuple(func.parameters()) + (coeffs,)) if adjoint else dict(adjoint=False)
    out = native.cdeint(X, func, z0.to(DEV), t.to(DEV), dt=dt, **SDE, **kw)
    assert _front().last_dispatch()[0].path == "reversible_heun_stepwise"
    (out * lw.to(DEV)).sum().backward()
    _close(out, want, 1e-4, 1e-5)
    _close(coeffs.grad, co.grad, 1e-3, 1e-3 * co.grad.abs().max().item())
    _close(func.linear.weight.grad, f64.linear.weight.grad, 1e-3, 1e-3 * f64.linear.weight.grad.abs().max().item())


# ------------------------------------------------------------------------------------------------ the reference's two tests
def test_reference_backend_test_with_the_torchsde_spelling(native):
    """reference test/test_cdeint.py:49-63 (`test_backend`): the torchsde spelling of the midpoint solve is the torchdiffeq
    request with the same step -- bitwise, for the reference's plain function and for the fused affine field with gradients."""
    x = torch.randn(1, 10, 2, generator=torch.Generator().manual_seed(5))
    z0 = torch.randn(1, 3, generator=torch.Generator().manual_seed(6))
    X = native.CubicSpline(native.natural_cubic_coeffs(x.to(DEV)))

    def func(t, z):
        return -z.unsqueeze(-1).expand(1, 3, 2)

    ode = native.cdeint(X=X, func=func, z0=z0.to(DEV), t=X.interval, backend="torchdiffeq", method="midpoint",
                        options=dict(step_size=1.0), adjoint=False)
    sde = native.cdeint(X=X, func=func, z0=z0.to(DEV), t=X.interval, backend="torchsde", method="midpoint", dt=1.0, adjoint=False)
    assert _front().last_dispatch()[0].path == "stepwise"
    assert sde.shape == (1, 2, 3) and torch.equal(ode, sde)
    results = []
    for kw in (dict(backend="torchdiffeq", method="midpoint", options=dict(step_size=1.0)),
               dict(backend="torchsde", method="midpoint", dt=1.0)):
        f = LinearField(3, 2, scale=0.5, seed=1).to(DEV)
        z = z0.to(DEV).requires_grad_(True)
        out = native.cdeint(X, f, z, X.interval, **kw)
        assert _front().last_dispatch()[0].path == "fixed_grid"
        out[:, -1].sum().backward()
        results.append((out.detach(), z.grad, f.linear.weight.grad, f.linear.bias.grad))
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_reference_shape_test_torchsde_row(native):
    """reference test/test_cdeint.py:6-46 (`test_shape`), the ('torchsde', 'midpoint', {"dt": 1.0}) row: natural cubic control,
    the sigmoid module, off-grid float64 output times, tolerances passed along; the shape of the result.  And the same call
    with method="reversible_heun"."""
    gen = torch.Generator().manual_seed(12)
    for points, channels, hidden, batch, n_times in ((17, 2, 4, 2, 5), (5, 1, 1, 1, 2)):
        values = torch.rand(batch, points, channels, generator=gen)
        spline = native.CubicSpline(native.natural_cubic_coeffs(values.to(DEV)))
        f = _TricksFunc(channels, hidden, torch.float32).to(DEV)
        z0 = torch.rand(batch, hidden, generator=gen).to(DEV)
        start, end = spline.interval
        out_times = torch.rand(n_times, dtype=torch.float64, generator=gen).sort().values * (end.cpu() - start.cpu()) + start.cpu()
        out = native.cdeint(spline, f, z0, out_times, backend="torchsde", method="midpoint", rtol=1e-1, atol=1e-1, dt=1.0)
        assert out.shape == (batch, n_times, hidden)
        out = native.cdeint(spline, f, z0, out_times, backend="torchsde", method="reversible_heun", rtol=1e-1, atol=1e-1, dt=1.0)
        assert out.shape == (batch, n_times, hidden) and _front().last_dispatch()[0].path == "reversible_heun_stepwise"

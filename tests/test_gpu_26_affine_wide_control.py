"""The one-layer vector field Linear(H, H C) (+ tanh) on controls of 17 to 64 channels under rk4 on the GPU: the tiled forward
(K2c) and continuous-adjoint sweep (K3c, csrc/rk4_affine_tiled.hip) behind CDE_VARIANT_AUTO against the float64 oracle and
against variant="generic", the VALU kernels these calls ran on before.

Shapes (H, C, degree, tanh, scale): the full envelope; the first channel count beyond the old tiles with H not a multiple of 4
(scalar loads, CP = 20, linear control); C not a multiple of 4; pre-activations of order 1 (so the slope 1 - t^2 matters); one
hidden unit.  B = 35 (two full 16-series tiles and a ragged one), L = 10, t = [0, 3.5, 9] (two reverse segments, an output time
off the grid), step_size = 1 unless stated.

Bars, as tests/test_gpu_19_wide_control.py.  Trajectories: rtol 1e-4 with atol max(5e-6, 4 x the error of the oracle run in
float32 on the CPU).  Gradients: rtol 1e-3 with atol max(1e-3 max|want|, 4 x the CPU float32 oracle's error), against the
float64 oracle's adjoint=True run.
"""
import functools
import importlib

import pytest
import torch

from gpu_common import oracle_cde, oracle_interp, make_series, DEV, _close
from helpers import LinearField

pytestmark = pytest.mark.gpu

# (H, C, degree, tanh, scale): scale None is 0.4 / sqrt(C)
CASES = [(32, 64, 3, True, None), (5, 17, 1, False, None), (32, 21, 3, False, None), (16, 36, 1, True, 0.5),
         (1, 64, 3, False, None)]
IDS = ["H%d_C%d_deg%d_%s" % (c[:3] + ("tanh" if c[3] else "id",)) for c in CASES]
B_FULL, L, T_OUT, STEP = 35, 10, (0., 3.5, 9.), 1.0
NAMES = ("weight", "bias")


def _front():
    return importlib.import_module("torchcde_amd.cdeint")


def _make(case, dtype=torch.float32):
    H, C, _, tanh, scale = case
    return LinearField(H, C, dtype, scale=0.4 / C ** 0.5 if scale is None else scale, tanh=tanh, seed=5)


@functools.lru_cache(maxsize=None)
def _reference(case, B, step=STEP, t_out=T_OUT, length=L, oracle=True):
    """Inputs of one case and the oracle's adjoint=True runs in float64 and in float32 on the CPU (computed once, shared)."""
    H, C, degree, _, _ = case
    seed = 700 + 7 * H + C
    x = make_series(B, length, C, torch.float32, seed=seed)
    coeffs = oracle_interp.hermite_bdiff_coeffs(x) if degree == 3 else x
    gen = torch.Generator().manual_seed(seed + 1)
    z0 = torch.randn(B, H, generator=gen)
    t = torch.tensor(t_out)
    lw = torch.rand(B, len(t_out), H, generator=gen) + 0.5
    runs = {}
    for dtype in (torch.float64, torch.float32) if oracle else ():
        func = _make(case, dtype)
        path = (oracle_interp.CubicPath if degree == 3 else oracle_interp.LinearPath)(coeffs.to(dtype))
        z = z0.to(dtype).clone().requires_grad_(True)
        out = oracle_cde.cdeint(path, func, z, t.to(dtype), adjoint=True, method="rk4", options=dict(step_size=step))
        (out * lw.to(dtype)).sum().backward()
        runs[dtype] = dict(out=out.detach(), z=z.grad, weight=func.linear.weight.grad, bias=func.linear.bias.grad)
    return dict(case=case, coeffs=coeffs, z0=z0, t_out=t, lw=lw, degree=degree, step=step, f64=runs.get(torch.float64),
                f32=runs.get(torch.float32))


def _native_inputs(native, ref):
    X = (native.CubicSpline if ref["degree"] == 3 else native.LinearInterpolation)(ref["coeffs"].to(DEV))
    return X, _make(ref["case"]).to(DEV), ref["t_out"].to(DEV)


def _bar(want, cpu32):
    return max(1e-3 * want.abs().max().item(), 4 * (cpu32.double() - want).abs().max().item())


def _out_atol(ref):
    return max(5e-6, 4 * (ref["f32"]["out"].double() - ref["f64"]["out"]).abs().max().item())


def _gradients(z, func):
    return dict(z=z.grad, weight=func.linear.weight.grad, bias=func.linear.bias.grad)


def _check_gradients(ref, out, got, label, names=("z",) + NAMES):
    want, cpu32 = ref["f64"], ref["f32"]
    report = ["%s out: max err %.3g (bar: rtol 1e-4, atol %.3g), max|z| %.3g" % (
        label, (out.detach().double().cpu() - want["out"]).abs().max().item(), _out_atol(ref), want["out"].abs().max().item())]
    for name in names:
        err = (got[name].detach().double().cpu() - want[name]).abs().max().item()
        report.append("%s %s: max err %.3g, bar %.3g, max|want| %.3g, cpu32 err %.3g" % (
            label, name, err, _bar(want[name], cpu32[name]), want[name].abs().max().item(),
            (cpu32[name].double() - want[name]).abs().max().item()))
    print("\n".join(report))
    _close(out, want["out"], 1e-4, _out_atol(ref))
    for name in names:
        assert got[name].shape == want[name].shape, name
        _close(got[name], want[name], 1e-3, _bar(want[name], cpu32[name]))


def _train(native, ref, variant="auto", t_out=None, step=None, **kw):
    X, func, t = _native_inputs(native, ref)
    z = ref["z0"].to(DEV).requires_grad_(True)
    out = native.cdeint(X, func, z, t if t_out is None else t_out, method="rk4",
                        options=dict(step_size=ref["step"] if step is None else step), variant=variant, **kw)
    verdict = _front().last_dispatch()
    (out * ref["lw"].to(DEV)).sum().backward()
    return out, z, func, verdict


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_affine_wide_control_forward_tiled(native, case):
    """K2c against the float64 oracle and against the VALU kernels on the same inputs; the dispatch record names the kernels."""
    ref = _reference(case, B_FULL)
    X, func, t_out = _native_inputs(native, ref)
    z0 = ref["z0"].to(DEV)
    with torch.no_grad():
        auto = native.cdeint(X, func, z0, t_out, method="rk4", options=dict(step_size=STEP))
        choice, _ = _front().last_dispatch()
        assert (choice.path, choice.form, choice.family) == ("rk4", "exact", "tiled"), (choice, choice.form, choice.family)
        generic = native.cdeint(X, func, z0, t_out, method="rk4", options=dict(step_size=STEP), variant="generic")
        choice, _ = _front().last_dispatch()
        assert (choice.path, choice.form, choice.family) == ("rk4", "exact", ""), (choice, choice.form, choice.family)
    assert auto.shape == (B_FULL, len(T_OUT), case[0])
    print("forward: max err vs float64 %.3g (atol %.3g), vs generic %.3g, max|z| %.3g" % (
        (auto.double().cpu() - ref["f64"]["out"]).abs().max().item(), _out_atol(ref), (auto - generic).abs().max().item(),
        ref["f64"]["out"].abs().max().item()))
    _close(auto, ref["f64"]["out"], 1e-4, _out_atol(ref))
    _close(auto, generic, 1e-4, _out_atol(ref))
    assert not torch.equal(auto, generic)            # two different kernels did run


# ------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_affine_wide_control_adjoint_tiled(native, case):
    """K2c + K3c + the factor reduction: out, dL/dz0, dL/dW and dL/db against the oracle's adjoint=True run in float64; a second
    identical call gives the same bits (fixed-order reductions, no float atomics); adjoint_params=(bias,) leaves the weight
    without a gradient and the other two as they were."""
    ref = _reference(case, B_FULL)
    out, z, func, (choice, _) = _train(native, ref)
    assert (choice.path, choice.form, choice.family) == ("rk4", "exact", "tiled"), (choice, choice.form, choice.family)
    assert out.shape == (B_FULL, len(T_OUT), case[0])
    first = _gradients(z, func)
    _check_gradients(ref, out, first, "tiled")
    out2, z2, func2, _ = _train(native, ref)
    second = _gradients(z2, func2)
    assert torch.equal(out, out2)
    for name in ("z",) + NAMES:
        assert torch.equal(first[name], second[name]), name
    X, func3, t_out = _native_inputs(native, ref)
    z3 = ref["z0"].to(DEV).requires_grad_(True)
    out3 = native.cdeint(X, func3, z3, t_out, method="rk4", options=dict(step_size=STEP), adjoint_params=(func3.linear.bias,))
    assert _front().last_dispatch()[0].family == "tiled"
    (out3 * ref["lw"].to(DEV)).sum().backward()
    assert func3.linear.weight.grad is None
    assert torch.equal(z3.grad, first["z"]) and torch.equal(func3.linear.bias.grad, first["bias"])


def test_affine_wide_control_chunked_sweep(native):
    """The full envelope with a factor budget of two RK steps per chunk (ten reverse steps in two segments: at least five
    chunks): the state crosses the chunks through HBM unchanged, so dL/dz0 keeps its bits; the parameter gradients are summed
    chunk by chunk."""
    ref = _reference(CASES[0], B_FULL)
    out, z, func, _ = _train(native, ref)
    whole = _gradients(z, func)
    row_bytes = (2048 + 32) * 4                      # G [row][MP = 32 x 64] and Z [row][32]
    with native.tuning(wide_scratch_bytes=2 * 4 * 48 * row_bytes):
        out_c, z_c, func_c, (choice, _) = _train(native, ref)
    assert choice.family == "tiled"
    assert torch.equal(out_c, out) and torch.equal(z_c.grad, whole["z"])
    _check_gradients(ref, out_c, _gradients(z_c, func_c), "chunked")


def test_affine_wide_control_larger_batch(native):
    """4115 series are 258 tiles: more than 256, so a workgroup holds two waves, each with its own dX slab.  L = 4 (the control
    ends at t = 3, so t = [0, 1.5, 3]); against the VALU kernels: trajectories rtol 1e-4 / atol 5e-6, gradients rtol 1e-3 with
    atol 1e-3 of the largest entry."""
    ref = _reference(CASES[1], 4115, STEP, (0., 1.5, 3.), 4, False)
    runs = {}
    for variant in ("auto", "generic"):
        out, z, func, (choice, _) = _train(native, ref, variant)
        assert choice.family == ("tiled" if variant == "auto" else "")
        runs[variant] = dict(out=out.detach(), **_gradients(z, func))
    _close(runs["auto"]["out"], runs["generic"]["out"], 1e-4, 5e-6)
    for name in ("z",) + NAMES:
        want = runs["generic"][name]
        print("larger batch %s: max diff %.3g of %.3g" % (name, (runs["auto"][name] - want).abs().max().item(),
                                                          want.abs().max().item()))
        _close(runs["auto"][name], want, 1e-3, 1e-3 * want.abs().max().item())
    assert not torch.equal(runs["auto"]["out"], runs["generic"]["out"])


def test_affine_wide_control_time_grid(native):
    """A float64 output-time tensor (the grid and the stage times are formed in float64) and step_size = 0.5 on case 3."""
    ref = _reference(CASES[2], B_FULL, 0.5)
    out, z, func, (choice, _) = _train(native, ref, t_out=ref["t_out"].double().to(DEV))
    assert choice.family == "tiled" and out.dtype == torch.float32
    _check_gradients(ref, out, _gradients(z, func), "float64 times, step 0.5")


# ------------------------------------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("C", [16, 65])
def test_channel_counts_next_to_the_envelope_keep_their_kernels(native, C):
    """C = 16 stays with the wide tile kernels of rk4_wide.hip, C = 65 with the VALU kernels: family "", and the oracle's result."""
    case = (32, C, 3, True, None)
    ref = _reference(case, B_FULL)
    out, z, func, (choice, _) = _train(native, ref)
    assert (choice.path, choice.form, choice.family) == ("rk4", "exact", ""), (choice, choice.form, choice.family)
    _check_gradients(ref, out, _gradients(z, func), "C = %d" % C)


def test_a_float64_field_keeps_the_generic_kernels(native):
    case = CASES[2]
    ref = _reference(case, B_FULL)
    X = native.CubicSpline(ref["coeffs"].double().to(DEV))
    func = _make(case, torch.float64).to(DEV)
    with torch.no_grad():
        out = native.cdeint(X, func, ref["z0"].double().to(DEV), ref["t_out"].double().to(DEV), method="rk4",
                            options=dict(step_size=STEP))
    choice, _ = _front().last_dispatch()
    assert (choice.path, choice.family) == ("rk4", ""), (choice, choice.family)
    _close(out, ref["f64"]["out"], 1e-9, 1e-11)

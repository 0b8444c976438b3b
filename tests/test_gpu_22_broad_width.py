"""The two-layer vector field with an inner layer of 129 to 256 units under rk4 on the GPU: the fused forward (K2mb) and
continuous-adjoint sweep (K3mb, csrc/rk4_mlp_broad.hip) against the float64 oracle and the step-wise path; every other request
at these widths runs step-wise with a reason.

Shapes (H, C, width, degree, final, hidden): the examples' shape at twice the width, every K group full; one unit in the upper
half with ragged rows (scalar W2 loads, linear control); the edge of H CP <= 1024 with four G2 blocks; CP = 24 with a width that
is no multiple of 4; one state unit.  B = 35 (two full 16-series tiles and a ragged one), L = 10, t = [0, 3.5, 9] (two reverse
segments, an output time off the grid), step_size = 1 unless stated.

Bars, as tests/test_gpu_19_wide_control.py.  Trajectories: rtol 1e-4 with atol max(5e-6, 4 x the error of the oracle run in
float32 on the CPU).  Gradients: rtol 1e-3 with atol max(1e-3 max|want|, 4 x the CPU float32 oracle's error), against the
float64 oracle.  With these draws the CPU float32 oracle stays within 6e-6 of the largest entry on every gradient, so no draw
sits on a relu kink and the 1e-3 term is the bar.  Requests outside the envelope: the bars of
test_stepwise_adjoint_in_closed_form_for_recognised_fields (2e-2 of the largest entry).
"""
import functools
import importlib
import warnings

import pytest
import torch
import torch.nn.functional as F

from gpu_common import oracle_cde, oracle_interp, make_series, DEV, _close
from helpers import TwoLayerField

pytestmark = pytest.mark.gpu

CASES = [(32, 8, 256, 3, True, "relu"), (5, 3, 129, 1, False, "softplus"), (32, 32, 200, 3, True, "softplus"),
         (16, 21, 130, 1, True, "relu"), (1, 64, 256, 3, False, "relu")]
IDS = ["H%d_C%d_w%d_deg%d_%s_%s" % (c[:4] + ("tanh" if c[4] else "id", c[5])) for c in CASES]
B_FULL, L, T_OUT, STEP = 35, 10, (0., 3.5, 9.), 1.0
NAMES = ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias")


class BroadField(TwoLayerField):
    """helpers.TwoLayerField with the hidden activation as a choice: relu or torch's default softplus"""

    def __init__(self, H, C, width, dtype=torch.float32, seed=0, final_tanh=True, hidden="relu"):
        super().__init__(H, C, width, dtype, seed, final_tanh)
        self.hidden = hidden

    def forward(self, t, z):
        y = self.linear2((F.softplus if self.hidden == "softplus" else torch.relu)(self.linear1(z)))
        if self.final_tanh:
            y = y.tanh()
        return y.view(*z.shape[:-1], self.H, self.C)


def _grad(module, name):
    layer, kind = name.split(".")
    return getattr(getattr(module, layer), kind).grad


def _front():
    return importlib.import_module("torchcde_amd.cdeint")


@functools.lru_cache(maxsize=None)
def _reference(case, B, step=STEP, t_out=T_OUT):
    """Inputs of one case and the oracle's adjoint=True runs in float64 and in float32 on the CPU (computed once, shared)."""
    H, C, w, degree, final_tanh, hidden = case
    seed = 500 + 7 * H + C
    x = make_series(B, L, C, torch.float32, seed=seed)
    coeffs = oracle_interp.hermite_bdiff_coeffs(x) if degree == 3 else x
    gen = torch.Generator().manual_seed(seed + 1)
    z0 = torch.randn(B, H, generator=gen)
    t = torch.tensor(t_out)
    lw = torch.rand(B, len(t_out), H, generator=gen) + 0.5
    make = functools.partial(BroadField, H, C, w, seed=5, final_tanh=final_tanh, hidden=hidden)
    runs = {}
    for dtype in (torch.float64, torch.float32):
        func = make(dtype=dtype)
        path = (oracle_interp.CubicPath if degree == 3 else oracle_interp.LinearPath)(coeffs.to(dtype))
        z = z0.to(dtype).clone().requires_grad_(True)
        out = oracle_cde.cdeint(path, func, z, t.to(dtype), adjoint=True, method="rk4", options=dict(step_size=step))
        (out * lw.to(dtype)).sum().backward()
        runs[dtype] = dict(out=out.detach(), z=z.grad, **{name: _grad(func, name) for name in NAMES})
    return dict(coeffs=coeffs, z0=z0, t_out=t, lw=lw, make=make, degree=degree, step=step, f64=runs[torch.float64],
                f32=runs[torch.float32])


def _native_inputs(native, ref):
    X = (native.CubicSpline if ref["degree"] == 3 else native.LinearInterpolation)(ref["coeffs"].to(DEV))
    return X, ref["make"]().to(DEV), ref["t_out"].to(DEV)


def _bar(want, cpu32):
    return max(1e-3 * want.abs().max().item(), 4 * (cpu32.double() - want).abs().max().item())


def _out_atol(ref):
    return max(5e-6, 4 * (ref["f32"]["out"].double() - ref["f64"]["out"]).abs().max().item())


def _check_gradients(ref, out, z, func, label):
    want, cpu32 = ref["f64"], ref["f32"]
    report = ["%s out: max err %.3g (bar: rtol 1e-4, atol %.3g), max|z| %.3g" % (
        label, (out.detach().double().cpu() - want["out"]).abs().max().item(), _out_atol(ref), want["out"].abs().max().item())]
    got = dict(z=z.grad, **{name: _grad(func, name) for name in NAMES})
    for name in ("z",) + NAMES:
        err = (got[name].detach().double().cpu() - want[name]).abs().max().item()
        report.append("%s %s: max err %.3g, bar %.3g, max|want| %.3g, cpu32 err %.3g" % (
            label, name, err, _bar(want[name], cpu32[name]), want[name].abs().max().item(),
            (cpu32[name].double() - want[name]).abs().max().item()))
    print("\n".join(report))
    _close(out, want["out"], 1e-4, _out_atol(ref))
    for name in ("z",) + NAMES:
        assert got[name].shape == want[name].shape, name
        _close(got[name], want[name], 1e-3, _bar(want[name], cpu32[name]))


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_broad_inner_layer_forward_fused(native, case):
    """K2mb against the float64 oracle of the same module and against the step-wise run of the user's module."""
    from torchcde_amd import fields
    ref = _reference(case, B_FULL)
    X, func, t_out = _native_inputs(native, ref)
    z0 = ref["z0"].to(DEV)
    found, _ = fields.probe(func, t_out[0], z0)
    assert found is not None and found.kind == "mlp2" and found.linears == (func.linear1, func.linear2)
    with torch.no_grad():
        fused = native.cdeint(X, func, z0, t_out, method="rk4", options=dict(step_size=STEP))
        choice, request = _front().last_dispatch()
        assert choice.path == "mlp_rk4_forward" and request.kind == "mlp2b" and request.tiles_ok, choice
        stepwise = native.cdeint(X, func, z0, t_out, method="rk4", options=dict(step_size=STEP), variant="generic")
        assert _front().last_dispatch()[0].path == "stepwise"
    assert fused.shape == (B_FULL, len(T_OUT), case[0])
    print("forward: max err vs float64 %.3g (atol %.3g), vs step-wise %.3g, max|z| %.3g" % (
        (fused.double().cpu() - ref["f64"]["out"]).abs().max().item(), _out_atol(ref), (fused - stepwise).abs().max().item(),
        ref["f64"]["out"].abs().max().item()))
    _close(fused, ref["f64"]["out"], 1e-4, _out_atol(ref))
    _close(fused, stepwise, 1e-4, _out_atol(ref))
    assert not torch.equal(fused, stepwise)          # two different code paths did run


# ------------------------------------------------------------------------------------------------ training
def _train(native, ref, budget=None, **kw):
    front = _front()
    X, func, t_out = _native_inputs(native, ref)
    z = ref["z0"].to(DEV).requires_grad_(True)
    saved = front._MlpBroadPlan.scratch_budget
    try:
        if budget is not None:
            front._MlpBroadPlan.scratch_budget = budget
        out = native.cdeint(X, func, z, t_out, method="rk4", options=dict(step_size=ref["step"]), **kw)
        verdict = front.last_dispatch()
        (out * ref["lw"].to(DEV)).sum().backward()
    finally:
        front._MlpBroadPlan.scratch_budget = saved
    return out, z, func, verdict


# H no multiple of 4 at the edge of H CP <= 1024: the last unit group's tiles read rows 1020 .. 1199 of the sweep's padded copies
PADDED_ROWS = (17, 60, 130, 3, True, "softplus")
ADJOINT = ([(c, B_FULL, None, STEP, T_OUT) for c in CASES] + [(c, 1, None, STEP, T_OUT) for c in CASES] +
           [(CASES[1], 261, None, STEP, T_OUT), (CASES[2], B_FULL, 1, STEP, T_OUT), (CASES[1], B_FULL, None, 0.7, (0., 1.4, 2.5, 8.)),
            (CASES[1], 4113, None, STEP, T_OUT), (PADDED_ROWS, B_FULL, None, STEP, T_OUT)])
ADJOINT_IDS = (IDS + ["single_series_" + i for i in IDS] +
               ["several_workgroups_B261", "one_step_per_launch", "step_0p7_across_knots_clipped_last_step",
                "two_waves_per_workgroup_B4113", "unit_group_past_H_reads_the_padded_rows"])


@pytest.mark.parametrize("case,B,budget,step,t_out", ADJOINT, ids=ADJOINT_IDS)
def test_broad_inner_layer_adjoint_fused(native, case, B, budget, step, t_out):
    """K2mb + K3mb + the factor reductions per half: out, dL/dz0 and all four parameter gradients against the oracle's
    adjoint=True run in float64.  `budget = 1` forces one RK step per sweep launch (state carried through HBM between launches);
    step 0.7 puts steps across knots, clips the last step of every segment and has outputs on and between grid points; 4113
    series are 258 tiles, the first batch size at which a workgroup holds two waves (each with its own dX slab); 17 x 60 has
    1020 rows and a fifth unit group that runs to row 1199."""
    ref = _reference(case, B, step, t_out)
    out, z, func, (choice, request) = _train(native, ref, budget)
    assert choice.path == "mlp_rk4_adjoint" and request.kind == "mlp2b" and request.tiles_ok, choice
    assert type(out.grad_fn).__name__ == "_FusedMlpBroadRK4Backward"
    assert out.shape == (B, len(t_out), case[0])
    _check_gradients(ref, out, z, func, "fused")


def test_broad_inner_layer_training_call_repeats_bitwise_and_no_grad_gives_its_forward(native):
    """A second identical call: the same bits in the outputs and in every gradient (fixed-order reductions, no float atomics);
    under no_grad the same bits as the forward of the training call."""
    ref = _reference(CASES[2], B_FULL)
    out1, z1, func1, _ = _train(native, ref)
    out2, z2, func2, _ = _train(native, ref)
    assert torch.equal(out1, out2) and torch.equal(z1.grad, z2.grad)
    for name in NAMES:
        assert torch.equal(_grad(func1, name), _grad(func2, name)), name
    X, func, t_out = _native_inputs(native, ref)
    with torch.no_grad():
        plain = native.cdeint(X, func, ref["z0"].to(DEV), t_out, method="rk4", options=dict(step_size=STEP))
    assert _front().last_dispatch()[0].path == "mlp_rk4_forward"
    assert torch.equal(plain, out1.detach())
    # grad mode with nothing to differentiate: the forward kernel alone, no autograd node
    for p in func.parameters():
        p.requires_grad_(False)
    quiet = native.cdeint(X, func, ref["z0"].to(DEV), t_out, method="rk4", options=dict(step_size=STEP))
    assert _front().last_dispatch()[0].path == "mlp_rk4_forward" and quiet.grad_fn is None and torch.equal(quiet, plain)


# ------------------------------------------------------------------------------------------------ outside the envelope
@pytest.mark.parametrize("what", ["default_dopri5", "adjoint_false", "time_gradient", "control_gradient", "three_of_four_params"])
def test_broad_inner_layer_requests_outside_the_envelope_run_stepwise(native, what):
    """Case 2's field with 7 series (on a cubic control, as this test of tests/test_gpu_19_wide_control.py has it): step-wise
    with kind "mlp2b", a reason and one warning per (class, reason), and -- through the closed-form adjoint dynamics -- the
    oracle's result."""
    H, C, w, degree, final_tanh, hidden = CASES[1]
    B = 7

    class Fresh(BroadField):                         # a class of its own per request: warn_once keys on (class, reason)
        pass

    x = make_series(B, L, C, torch.float32, seed=77)
    base = oracle_interp.hermite_bdiff_coeffs(x)
    gen = torch.Generator().manual_seed(78)
    z0 = torch.randn(B, H, generator=gen)
    t_out = torch.tensor(T_OUT)
    lw = torch.rand(B, len(T_OUT), H, generator=gen) + 0.5
    rk4 = dict(method="rk4", options=dict(step_size=STEP))

    def run(cdeint, make_path, func, dtype, device):
        coeffs = base.to(dtype).to(device).clone().requires_grad_(what == "control_gradient")
        z = z0.to(dtype).to(device).clone().requires_grad_(True)
        t = t_out.to(dtype).to(device).clone().requires_grad_(what == "time_gradient")
        X = make_path(coeffs)
        if what == "default_dopri5":
            out = cdeint(X, func, z, t, rtol=1e-5, atol=1e-7)
        elif what == "adjoint_false":
            out = cdeint(X, func, z, t, adjoint=False, **rk4)
        elif what == "time_gradient":
            out = cdeint(X, func, z, t, **rk4)
        elif what == "control_gradient":
            out = cdeint(X, func, z, t, adjoint_params=tuple(func.parameters()) + (coeffs,), **rk4)
        else:
            out = cdeint(X, func, z, t, adjoint_params=tuple(func.parameters())[:3], **rk4)
        return out, z, t, coeffs

    f64 = Fresh(H, C, w, dtype=torch.float64, seed=5, final_tanh=final_tanh, hidden=hidden)
    ref, zo, to, co = run(oracle_cde.cdeint, oracle_interp.CubicPath, f64, torch.float64, "cpu")
    (ref * lw.double()).sum().backward()
    func = Fresh(H, C, w, seed=5, final_tanh=final_tanh, hidden=hidden).to(DEV)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out, z, t, coeffs = run(native.cdeint, native.CubicSpline, func, torch.float32, DEV)
        choice, request = _front().last_dispatch()
        run(native.cdeint, native.CubicSpline, func, torch.float32, DEV)
    assert choice.path == "stepwise" and request.kind == "mlp2b" and request.tiles_ok and choice.reason, (choice, request)
    if what == "default_dopri5":
        assert "inner layer" in choice.reason and "rk4" in choice.reason
    if what == "three_of_four_params":
        assert request.params == "foreign"
    ours = [m for m in caught if "runs step-wise" in str(m.message)]
    assert len(ours) == 1 and "Fresh" in str(ours[0].message), [str(m.message) for m in caught]
    (out * lw.to(DEV)).sum().backward()

    def close(got, want, floor=0.0):
        _close(got, want, 2e-2, 2e-2 * max(floor, want.abs().max().item()))
    close(out, ref)
    close(z.grad, zo.grad)
    for i, (got, p64) in enumerate(zip(func.parameters(), f64.parameters())):
        if what == "three_of_four_params" and i == 3:
            assert got.grad is None and p64.grad is None                      # the parameter left out of adjoint_params
            continue
        close(got.grad, p64.grad, 1e-3)
    if what == "time_gradient":
        close(t.grad, to.grad)
    if what == "control_gradient":
        assert coeffs.grad is not None
        close(coeffs.grad, co.grad)


# ------------------------------------------------------------------------------------------------ boundaries
def test_inner_widths_next_to_the_envelope_keep_their_paths(native):
    """Width 128 stays with the two-layer kernels of the 32 x 8 tiles (kind "mlp2"), 129 is the first broad inner layer, 257 is
    beyond every tile; H = 40 at width 129 is beyond the broad envelope (and beyond the tall-state kernels' width); 21 channels
    at width 128 stay a wide control."""
    for H, C, w, kind, tiles_ok, path in ((8, 8, 128, "mlp2", True, "mlp_rk4_forward"), (8, 8, 129, "mlp2b", True, "mlp_rk4_forward"),
                                          (8, 8, 257, "mlp2", False, "stepwise"), (40, 8, 129, "mlp2", False, "stepwise"),
                                          (8, 21, 128, "mlp2w", True, "mlp_rk4_forward")):
        x = make_series(5, 6, C, torch.float32, seed=40 + C)
        X = native.CubicSpline(oracle_interp.hermite_bdiff_coeffs(x).to(DEV))
        func = BroadField(H, C, w, seed=3).to(DEV)
        z0 = torch.randn(5, H, generator=torch.Generator().manual_seed(41)).to(DEV)
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = native.cdeint(X, func, z0, X.interval, method="rk4", options=dict(step_size=1.0))
            choice, request = _front().last_dispatch()
            assert (request.kind, request.tiles_ok, choice.path) == (kind, tiles_ok, path), (H, C, w, choice, request)
            generic = native.cdeint(X, func, z0, X.interval, method="rk4", options=dict(step_size=1.0), variant="generic")
        _close(out, generic, 1e-4, 5e-6)

"""The three-layer vector field Linear -> hid -> Linear -> hid -> Linear -> act under rk4 on the GPU: the fused forward (K2m3)
and continuous-adjoint sweep (K3m3, csrc/rk4_mlp3.hip) against the float64 oracle and the step-wise path; every other request
of such a module runs step-wise with a reason.

Shapes (H, C, width1, width2, degree, final, hidden): every tile full; everything padded; the ln 2 padding of softplus with H
just above 16; one channel with a first width below one K group; two shapes whose first width is not a multiple of 4 (the
forward kernel then reads Wm element by element instead of as 16-byte rows).  B = 35 (two full 16-series tiles and a ragged one), L = 10,
t = [0, 3.5, 9] (two reverse segments, an output time off the grid), step_size = 1.

Bars.  Forward: the two-layer forward test's (rtol 1e-4, atol 5e-6).  Gradients: the project's own from
test_two_layer_field_adjoint_fused, max(1e-3 max|want|, 4 x the error of the oracle run in float32 on the CPU), measured
against the float64 oracle; on these inputs the CPU float32 run is within 2e-6 max|want| of float64, so the first term decides.
"""
import functools
import importlib
import warnings

import pytest
import torch
import torch.nn.functional as F

from gpu_common import oracle_cde, oracle_interp, make_series, DEV, _close

pytestmark = pytest.mark.gpu

CASES = [(32, 8, 128, 128, 3, True, "relu"), (5, 3, 20, 12, 1, False, "relu"), (17, 8, 100, 36, 3, True, "softplus"),
         (32, 1, 4, 128, 3, True, "relu"),
         # width1 not a multiple of 4: the forward kernel reads the middle layer element by element (its VEC = false forms)
         (5, 3, 22, 13, 1, False, "relu"), (17, 8, 50, 30, 3, True, "softplus")]
B_FULL, L, T_OUT, STEP = 35, 10, (0., 3.5, 9.), 1.0
NAMES = ("first.weight", "first.bias", "middle.weight", "middle.bias", "last.weight", "last.bias")


class ThreeLayerField(torch.nn.Module):
    def __init__(self, H, C, w1, w2, dtype=torch.float32, seed=0, final_tanh=True, hidden="relu"):
        super().__init__()
        self.H, self.C, self.final_tanh, self.hidden = H, C, final_tanh, hidden
        gen = torch.Generator().manual_seed(seed)
        self.first = torch.nn.Linear(H, w1).to(dtype)
        self.middle = torch.nn.Linear(w1, w2).to(dtype)
        self.last = torch.nn.Linear(w2, H * C).to(dtype)
        with torch.no_grad():
            for lin in (self.first, self.middle, self.last):
                bound = 1 / lin.in_features ** 0.5
                lin.weight.copy_((torch.rand(lin.weight.shape, generator=gen, dtype=torch.float64) * 2 - 1) * bound)
                lin.bias.copy_((torch.rand(lin.bias.shape, generator=gen, dtype=torch.float64) * 2 - 1) * bound)

    def forward(self, t, z):
        hid = F.softplus if self.hidden == "softplus" else torch.relu
        y = self.last(hid(self.middle(hid(self.first(z)))))
        if self.final_tanh:
            y = y.tanh()
        return y.view(*z.shape[:-1], self.H, self.C)


def _grad(module, name):
    layer, kind = name.split(".")
    return getattr(getattr(module, layer), kind).grad


@functools.lru_cache(maxsize=None)
def _reference(case, B):
    """Inputs of one case and the oracle's adjoint=True runs in float64 and in float32 on the CPU (computed once per case)."""
    H, C, w1, w2, degree, final_tanh, hidden = case
    seed = 300 + 7 * H + C
    x = make_series(B, L, C, torch.float32, seed=seed)
    coeffs = oracle_interp.hermite_bdiff_coeffs(x) if degree == 3 else x
    gen = torch.Generator().manual_seed(seed + 1)
    z0 = torch.randn(B, H, generator=gen)
    t_out = torch.tensor(T_OUT)
    lw = torch.rand(B, len(T_OUT), H, generator=gen) + 0.5
    make = functools.partial(ThreeLayerField, H, C, w1, w2, seed=5, final_tanh=final_tanh, hidden=hidden)
    runs = {}
    for dtype in (torch.float64, torch.float32):
        func = make(dtype=dtype)
        path = (oracle_interp.CubicPath if degree == 3 else oracle_interp.LinearPath)(coeffs.to(dtype))
        z = z0.to(dtype).clone().requires_grad_(True)
        out = oracle_cde.cdeint(path, func, z, t_out.to(dtype), adjoint=True, method="rk4", options=dict(step_size=STEP))
        (out * lw.to(dtype)).sum().backward()
        runs[dtype] = dict(out=out.detach(), z=z.grad, **{name: _grad(func, name) for name in NAMES})
    return dict(coeffs=coeffs, z0=z0, t_out=t_out, lw=lw, make=make, degree=degree, f64=runs[torch.float64],
                f32=runs[torch.float32])


def _native_inputs(native, ref):
    X = (native.CubicSpline if ref["degree"] == 3 else native.LinearInterpolation)(ref["coeffs"].to(DEV))
    return X, ref["make"]().to(DEV), ref["t_out"].to(DEV)


def _bar(want, cpu32):
    return max(1e-3 * want.abs().max().item(), 4 * (cpu32.double() - want).abs().max().item())


def _check_gradients(ref, out, z, func, label):
    want, cpu32 = ref["f64"], ref["f32"]
    report = ["%s out: max err %.3g (bar: rtol 1e-4, atol %.3g)" % (
        label, (out.detach().double().cpu() - want["out"]).abs().max().item(),
        max(5e-6, 4 * (cpu32["out"].double() - want["out"]).abs().max().item()))]
    got = dict(z=z.grad, **{name: _grad(func, name) for name in NAMES})
    for name in ("z",) + NAMES:
        err = (got[name].detach().double().cpu() - want[name]).abs().max().item()
        report.append("%s %s: max err %.3g, bar %.3g, max|want| %.3g, cpu32 err %.3g" % (
            label, name, err, _bar(want[name], cpu32[name]), want[name].abs().max().item(),
            (cpu32[name].double() - want[name]).abs().max().item()))
    print("\n".join(report))
    _close(out, want["out"], 1e-4, max(5e-6, 4 * (cpu32["out"].double() - want["out"]).abs().max().item()))
    for name in ("z",) + NAMES:
        assert got[name].shape == want[name].shape, name
        _close(got[name], want[name], 1e-3, _bar(want[name], cpu32[name]))


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", CASES, ids=lambda c: "H%d_C%d_w%d_%d_deg%d_%s_%s" % (c[:5] + ("tanh" if c[5] else "id", c[6])))
def test_three_layer_field_forward_fused(native, case):
    """K2m3 against the float64 oracle of the same module and against the step-wise run of the user's module."""
    from torchcde_amd import fields
    ref = _reference(case, B_FULL)
    X, func, t_out = _native_inputs(native, ref)
    z0 = ref["z0"].to(DEV)
    found, _ = fields.probe(func, t_out[0], z0)
    assert found is not None and found.kind == "mlp3" and found.linears == (func.first, func.middle, func.last)
    with torch.no_grad():
        fused = native.cdeint(X, func, z0, t_out, method="rk4", options=dict(step_size=STEP))
        choice, request = _last(native)
        assert choice.path == "mlp_rk4_forward" and request.kind == "mlp3", choice
        stepwise = native.cdeint(X, func, z0, t_out, method="rk4", options=dict(step_size=STEP), variant="generic")
        assert _last(native)[0].path == "stepwise"
    assert fused.shape == (B_FULL, len(T_OUT), case[0])
    print("forward: max err vs float64 %.3g, vs step-wise %.3g" % (
        (fused.double().cpu() - ref["f64"]["out"]).abs().max().item(), (fused - stepwise).abs().max().item()))
    _close(fused, ref["f64"]["out"], 1e-4, 5e-6)
    _close(fused, stepwise, 1e-4, 5e-6)
    assert not torch.equal(fused, stepwise)          # two different code paths did run


def _last(native):
    return importlib.import_module("torchcde_amd.cdeint").last_dispatch()


# ------------------------------------------------------------------------------------------------ training
def _train(native, ref, budget=None, **kw):
    front = importlib.import_module("torchcde_amd.cdeint")
    X, func, t_out = _native_inputs(native, ref)
    z = ref["z0"].to(DEV).requires_grad_(True)
    saved = front._Mlp3Plan.scratch_budget
    try:
        if budget is not None:
            front._Mlp3Plan.scratch_budget = budget
        out = native.cdeint(X, func, z, t_out, method="rk4", options=dict(step_size=STEP), **kw)
        verdict = front.last_dispatch()
        (out * ref["lw"].to(DEV)).sum().backward()
    finally:
        front._Mlp3Plan.scratch_budget = saved
    return out, z, func, verdict


@pytest.mark.parametrize("case,B,budget", [(CASES[0], B_FULL, None), (CASES[1], B_FULL, 1), (CASES[2], B_FULL, None),
                                           (CASES[3], B_FULL, None), (CASES[2], 1, None), (CASES[4], B_FULL, None),
                                           (CASES[5], B_FULL, None)],
                         ids=["full_tiles", "padded_one_step_per_launch", "softplus_padding", "one_channel", "single_series",
                              "width1_22_scalar_loads", "width1_50_scalar_loads_softplus"])
def test_three_layer_field_adjoint_fused(native, case, B, budget):
    """K2m3 + K3m3 + the three factor reductions: out, dL/dz0 and all six parameter gradients against the oracle's adjoint=True
    run in float64.  `budget = 1` forces one RK step per sweep launch (state carried through HBM between launches)."""
    ref = _reference(case, B)
    out, z, func, (choice, request) = _train(native, ref, budget)
    assert choice.path == "mlp_rk4_adjoint" and request.kind == "mlp3", choice
    assert type(out.grad_fn).__name__ == "_FusedMlp3RK4Backward"
    _check_gradients(ref, out, z, func, "fused")


def test_three_layer_fused_gradients_against_the_stepwise_adjoint(native):
    """The same call with variant="generic": torchdiffeq's adjoint stepped from the host with autograd through the user's
    module.  Both meet the oracle at the same bar."""
    ref = _reference(CASES[2], B_FULL)
    out_s, z_s, func_s, (choice, _) = _train(native, ref, variant="generic")
    assert choice.path == "stepwise"
    _check_gradients(ref, out_s, z_s, func_s, "step-wise")
    out, z, func, (choice, _) = _train(native, ref)
    assert choice.path == "mlp_rk4_adjoint"
    _check_gradients(ref, out, z, func, "fused")
    assert not torch.equal(out, out_s)


# ------------------------------------------------------------------------------------------------ step-wise requests
def test_three_layer_requests_outside_rk4_run_stepwise_with_a_reason(native):
    """The default method (dopri5) of a three-layer model: step-wise, one warning that names the three-layer field and what is
    fused for it, and -- through the closed-form adjoint dynamics -- the oracle's result.  float32 at the fused envelope for the
    verdict and the warning; small float64 settings (as test_stepwise_path_arbitrary_func_vs_oracle) for the tight comparison."""
    front = importlib.import_module("torchcde_amd.cdeint")

    class Fresh(ThreeLayerField):                    # a class of its own: warn_once keys on (class, reason)
        pass

    B, C, H = 6, 3, 8
    x = make_series(B, 6, C, torch.float32, seed=17)
    coeffs = oracle_interp.hermite_bdiff_coeffs(x)
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(17))
    X = native.CubicSpline(coeffs.to(DEV))
    func = Fresh(H, C, 16, 12, seed=3).to(DEV)
    z = z0.to(DEV).requires_grad_(True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = native.cdeint(X, func, z, X.interval)
        choice, request = front.last_dispatch()
        native.cdeint(X, func, z, X.interval)
    assert choice.path == "stepwise" and request.kind == "mlp3" and request.tiles_ok
    assert "three-layer" in choice.reason and "rk4" in choice.reason
    ours = [w for w in caught if "runs step-wise" in str(w.message)]
    assert len(ours) == 1 and "three-layer" in str(ours[0].message) and "Fresh" in str(ours[0].message)
    out[:, -1].pow(2).sum().backward()
    # Two tolerance-level adaptive solutions agree only to the global error of an rtol = 1e-4 solve, so both are measured
    # against a finely stepped float64 solution, at the bar of test_two_layer_field_forward_fused: 4 x the error of the
    # oracle's own default solve + 2e-3 of the scale.
    Xo = oracle_interp.CubicPath(coeffs.double())
    runs = {}
    for name, kw in (("fine", dict(method="rk4", options=dict(step_size=0.0625))), ("oracle", {})):
        fo = Fresh(H, C, 16, 12, dtype=torch.float64, seed=3)
        zo = z0.double().requires_grad_(True)
        ref = oracle_cde.cdeint(Xo, fo, zo, Xo.interval, **kw)
        ref[:, -1].pow(2).sum().backward()
        runs[name] = (ref.detach(), zo.grad)
    for what, got, at in (("out", out, 0), ("dL/dz0", z.grad, 1)):
        fine, oracle = runs["fine"][at], runs["oracle"][at]
        scale = fine.abs().max().item()
        err = (got.detach().double().cpu() - fine).abs().max().item()
        err_oracle = (oracle - fine).abs().max().item()
        print("default method, %s: step-wise float32 error %.3g, oracle's dopri5 error %.3g, scale %.3g" % (what, err, err_oracle, scale))
        assert err <= 4 * err_oracle + 2e-3 * scale, (what, err, err_oracle, scale)

    # float64: beyond the fused tiles -- step-wise with the closed form, tight against the oracle
    kw = dict(method="dopri5", rtol=1e-5, atol=1e-7)
    Xo = oracle_interp.CubicPath(coeffs.double())
    for hidden in ("relu", "softplus"):
        fo = ThreeLayerField(H, C, 16, 12, dtype=torch.float64, seed=3, hidden=hidden)
        zo = z0.double().requires_grad_(True)
        ref = oracle_cde.cdeint(Xo, fo, zo, Xo.interval, **kw)
        ref[:, -1].pow(2).sum().backward()
        fd = ThreeLayerField(H, C, 16, 12, dtype=torch.float64, seed=3, hidden=hidden).to(DEV)
        X64 = native.CubicSpline(coeffs.double().to(DEV))
        zd = z0.double().to(DEV).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = native.cdeint(X64, fd, zd, X64.interval, **kw)
        choice, request = front.last_dispatch()
        assert choice.path == "stepwise" and request.kind == "mlp3" and not request.tiles_ok
        out[:, -1].pow(2).sum().backward()
        _close(out, ref, 1e-3, 1e-4)
        _close(zd.grad, zo.grad, 1e-2, 1e-3)
        for pd, po in zip(fd.parameters(), fo.parameters()):
            _close(pd.grad, po.grad, 1e-2, 1e-3 * max(1.0, po.grad.abs().max().item()))


def test_five_of_six_adjoint_params_run_stepwise(native):
    """adjoint_params must name all six parameters or be absent (the sweep produces all six gradients, as K3m all four)."""
    front = importlib.import_module("torchcde_amd.cdeint")
    ref = _reference(CASES[1], B_FULL)
    X, func, t_out = _native_inputs(native, ref)
    params = tuple(func.parameters())
    verdicts = {}
    for label, given in (("five", params[:5]), ("six", params), ("six_reordered", tuple(reversed(params)))):
        func.zero_grad()
        z = ref["z0"].to(DEV).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = native.cdeint(X, func, z, t_out, method="rk4", options=dict(step_size=STEP), adjoint_params=given)
        verdicts[label] = front.last_dispatch()
        (out * ref["lw"].to(DEV)).sum().backward()
        if label == "five":
            assert func.last.bias.grad is None
        else:
            _check_gradients(ref, out, z, func, label)
    assert verdicts["five"][0].path == "stepwise" and verdicts["five"][1].params == "foreign"
    assert "adjoint_params" in verdicts["five"][0].reason or "three-layer" in verdicts["five"][0].reason
    assert verdicts["six"][0].path == verdicts["six_reordered"][0].path == "mlp_rk4_adjoint"

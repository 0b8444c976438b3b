"""The fused fixed-step solves on irregular knots that do not start at zero (tests/irregular_controls.py: knots 2.5 .. 11.5 with
no width equal to 1, output times inside the control's interval, step sizes 0.5 / 0.75 / 2.0 / output-to-output, all dyadic).

Families x shapes x {cubic, linear} x step size, 33 series on the one-layer kernels and 35 on the others (a ragged last tile):
the one-layer field under variant="mfma" and, without an activation, variant="bf16x3" -- K2bd and, under k2b_groups = 1, K2b;
with gradients the K3p pair and, under k3_waves = 1, K3bj -- the two-layer field with a softplus hidden layer on the 32 x 8 and
16 x 16 tiles (forward, adjoint=True, adjoint=False), the three-layer field (K2m3 / K3m3), the wide control (K2mc / K3mc), the
tall state (K2mh / K3mh), the broad inner layer (K2mb / K3mb) and reversible Heun (RHf / RHa).  variant="bf16x3" takes no
tanh field: those rows assert the refusal and run under "mfma" alone.  Every native call is followed by a check of what
last_dispatch() recorded -- path, kind, form and the autograd node: a step-wise fallback would make a case vacuous.

Bars (tests/irregular_controls.py: out_bar, grad_bar; tests/test_host_irregular_knots.py keeps the CPU float32 term below
1e-5 of the largest entry, so on gradients the 1e-3 term decides).
  trajectories    rtol 1e-4, atol max(5e-6, 4 x the CPU float32 oracle's error of the case), against the float64 oracle
  gradients       dL/dz0 and every parameter: rtol 1e-3, atol max(1e-3 max|want|, 4 x the CPU float32 error)
  bf16x3          also: relative error <= 4 x that of variant="mfma" + 1e-7 on the solution and <= 2 x + 1e-7 on dL/dz0; K2bd
                  against K2b within 1e-5 of the largest entry; the pair against k3_waves = 1 bitwise equal in the solution,
                  dL/dz0 and dL/db, dL/dW within 1e-5 of its scale
  reversible Heun rtol 1e-4 / atol 1e-5, the kernel's error <= 4 x the CPU float32 restatement's, gradients rtol 1e-3 / atol
                  1e-3 max|want|; adjoint=False bitwise equal to adjoint=True (one sweep)
  once per family a second identical call, the same call on a leading batch shape (5, 7) / (3, 11), and the same call on views
                  (z0 with strided rows, coefficients and knots as slices at an offset of larger buffers): bitwise equal

Measured on an MI355X, the worst case of each family as a share of its bar (error / (atol + rtol |want|), entry by entry):
                           solution   dL/dz0    parameters
  one-layer, mfma          0.18       0.0006    0.0015
  one-layer, K2bd / K2b    0.16/0.15                        relative error at most 1.12 x / 1.10 x that of mfma (bar 4 x)
  one-layer, K3p and K3bj  0.16       0.0003    0.0016      at most 1.2 x mfma on the solution, 1.5 x on dL/dz0 (bars 4 x, 2 x)
  mlp2, adjoint=True       0.16       0.0037    0.0071
  mlp2, adjoint=False      0.16       0.0025    0.0033
  mlp3                     0.16       0.0003    0.0007
  mlp2w                    0.17       0.0017    0.0035
  mlp2h                    0.18       0.0007    0.0015
  mlp2b                    0.17       0.0006    0.0015
  reversible Heun          0.46       0.0011    0.031       kernel error at most 2.9 x the CPU float32 restatement's (bar 4 x)
Every test prints its figures before it judges them (lines that start with IRR; run with -s).
"""
import pytest
import torch

from gpu_common import DEV, _close, _front
import irregular_controls as ic

pytestmark = pytest.mark.gpu

KIND = {"affine": "affine", "revheun": "affine"}
PATHS = {"affine": ("rk4", "rk4"), "revheun": ("reversible_heun", "reversible_heun")}     # (nothing to differentiate, training)
NODE = {"affine": "_FusedRK4Backward", "revheun": "_FusedReversibleHeunBackward", "mlp2": "_FusedMlpRK4Backward",
        "mlp3": "_FusedMlp3RK4Backward", "mlp2w": "_FusedMlpWideRK4Backward", "mlp2h": "_FusedMlpTallRK4Backward",
        "mlp2b": "_FusedMlpBroadRK4Backward"}


def _native_path(native, case, ref, batch=None, views=False):
    """The control from the native fits on the case's series and knots (bitwise the oracle's coefficients)."""
    x, knots = ref["x"].to(DEV), ic.knots().to(DEV)
    if batch is not None:
        x = x.reshape(*batch, *x.shape[1:])
    fit = native.hermite_cubic_coefficients_with_backward_differences if case.degree == 3 else native.linear_interpolation_coeffs
    coeffs = fit(x, knots)
    assert torch.equal(coeffs.reshape(ref["coeffs"].shape).cpu(), ref["coeffs"])
    if views:
        # rows 1 .. of a buffer with one more row per series (not contiguous, storage offset one row), knots 4 .. 13 of 16
        wide = torch.full((coeffs.size(0), coeffs.size(1) + 1, coeffs.size(2)), 7.0, device=DEV)
        wide[:, 1:] = coeffs
        longer = torch.full((16,), -3.0, device=DEV)
        longer[4:4 + ic.L] = knots
        coeffs, knots = wide[:, 1:], longer[4:4 + ic.L]
        assert not coeffs.is_contiguous() and coeffs.storage_offset() > 0 and knots.storage_offset() == 4
    return (native.CubicSpline if case.degree == 3 else native.LinearInterpolation)(coeffs, knots)


def _solve(native, case, ref, grad=True, batch=None, views=False, expect=None, **kw):
    """One native call of the case: out, and with `grad` dL/dz0 (`z`) and every parameter's gradient by name.  `expect`:
    (path, form, autograd node) instead of the family's."""
    X = _native_path(native, case, ref, batch, views)
    func = ic.make_field(case).to(DEV)
    z0, lw = ref["z0"].to(DEV), ref["lw"].to(DEV)
    if views:
        both = torch.full((z0.size(0), 2 * z0.size(1)), 5.0, device=DEV)
        both[:, ::2] = z0
        z0 = both[:, ::2]
        assert not z0.is_contiguous()
    if batch is not None:
        z0, lw = z0.reshape(*batch, -1), lw.reshape(*batch, *lw.shape[1:])
    z0 = z0.requires_grad_(grad)
    how = (dict(backend="torchsde", method="reversible_heun", dt=case.step) if case.family == "revheun" else
           dict(method="rk4", options=ic.options(case.step)))
    with torch.enable_grad() if grad else torch.no_grad():
        out = native.cdeint(X, func, z0, torch.tensor(ic.T_OUT, device=DEV), **how, **kw)
        choice, request = _front().last_dispatch()
        family = case.family
        path, form, node = expect or (PATHS.get(family, ("mlp_rk4_forward", "mlp_rk4_adjoint"))[grad], "", NODE[family])
        assert choice.path == path and request.kind == KIND.get(family, family) and request.tiles_ok, (choice, request)
        if family == "affine":
            assert choice.form == form, (choice.form, form)
        assert (type(out.grad_fn).__name__ == node) if grad else (out.grad_fn is None), out.grad_fn
        assert out.shape == (batch or (z0.size(0),)) + (len(ic.T_OUT), case.shape[0])
        got = dict(out=out.detach())
        if grad:
            (out * lw).sum().backward()
            got.update(z=z0.grad, **{name: p.grad for name, p in func.named_parameters()})
    return got


def _share(got, want, bar):
    """the largest error as a share of its bar, entry by entry"""
    got, want = got.detach().double().cpu().reshape(want.shape), want.double()
    return ((got - want).abs() / (bar[1] + bar[0] * want.abs())).max().item()


def _gap(got, want):
    return (got.detach().double().cpu().reshape(want.shape) - want).abs().max().item()


def _check(case, ref, got, label):
    """`got` against the float64 oracle: the trajectory and whatever gradients it holds, each printed before it is judged"""
    want = ref["f64"]
    bars = {name: (ic.out_bar(case, ref) if name == "out" else ic.grad_bar(case, ref, name)) for name in got}
    for name in got:
        print("IRR %s %s %s %s: max err %.3g = %.3g of its bar (atol %.3g), max|want| %.3g, cpu32 err %.3g" % (
            case.family, ic.case_id(case), label, name, _gap(got[name], want[name]), _share(got[name], want[name], bars[name]),
            bars[name][1], want[name].abs().max().item(), ic.cpu32_error(ref, name)))
    for name in got:
        assert got[name].numel() == want[name].numel(), name
        _close(got[name].reshape(want[name].shape), want[name], *bars[name])


def _rel(got, want):
    return float((got.double().cpu().reshape(want.shape) - want).abs().max() / want.abs().max())


def _same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert torch.equal(a[name].reshape(b[name].shape), b[name]), "%s: %s differs" % (what, name)


# ------------------------------------------------------------------------------------------------ the one-layer field
FORWARD_SHAPES = [(H, C, tanh) for H, C in ((32, 8), (31, 7), (1, 8)) for tanh in (False, True)]
TRAINING_SHAPES = [(H, C, tanh) for H, C in ((32, 8), (19, 5)) for tanh in (False, True)]


def _refused(native, case, ref):
    with pytest.raises(NotImplementedError, match="identity-activation"):
        _solve(native, case, ref, grad=False, variant="bf16x3")


@pytest.mark.parametrize("case", ic.cases("affine", FORWARD_SHAPES), ids=ic.case_id)
def test_one_layer_forward(native, case):
    """variant="mfma" against the oracle; without an activation K2bd (the default of variant="bf16x3") and K2b as well."""
    ref = ic.reference(case)
    want = ref["f64"]["out"]
    exact = _solve(native, case, ref, grad=False, variant="mfma", expect=("rk4", "exact", None))
    _check(case, ref, exact, "mfma")
    if case.shape[2]:
        return _refused(native, case, ref)
    duo = _solve(native, case, ref, grad=False, variant="bf16x3", expect=("rk4", "bf16x3", None))
    with native.tuning(k2b_groups=1):
        single = _solve(native, case, ref, grad=False, variant="bf16x3", expect=("rk4", "bf16x3", None))
    _check(case, ref, duo, "K2bd")
    _check(case, ref, single, "K2b")
    e_exact = _rel(exact["out"], want)
    for label, got in (("K2bd", duo), ("K2b", single)):
        e = _rel(got["out"], want)
        print("IRR affine %s %s relative error %.3g, mfma %.3g" % (ic.case_id(case), label, e, e_exact))
        assert e <= 4 * e_exact + 1e-7, (label, e, e_exact)
    _close(duo["out"], single["out"], 0.0, 1e-5 * single["out"].abs().max().item())


@pytest.mark.parametrize("case", ic.cases("affine", TRAINING_SHAPES), ids=ic.case_id)
def test_one_layer_training(native, case):
    """variant="mfma" against the oracle's adjoint=True run; without an activation the bf16 forward with the K3p pair (the
    default of variant="bf16x3") and with K3bj (k3_waves = 1)."""
    ref = ic.reference(case)
    want = ref["f64"]
    exact = _solve(native, case, ref, variant="mfma", expect=("rk4", "exact", NODE["affine"]))
    _check(case, ref, exact, "mfma")
    if case.shape[2]:
        return _refused(native, case, ref)
    pair = _solve(native, case, ref, variant="bf16x3", expect=("rk4", "bf16x3", NODE["affine"]))
    with native.tuning(k3_waves=1):
        one_wave = _solve(native, case, ref, variant="bf16x3", expect=("rk4", "bf16x3", NODE["affine"]))
    _check(case, ref, pair, "K3p")
    _check(case, ref, one_wave, "K3bj")
    for label, got in (("K3p", pair), ("K3bj", one_wave)):
        for name, factor in (("out", 4), ("z", 2)):
            e, e_exact = _rel(got[name], want[name]), _rel(exact[name], want[name])
            print("IRR affine %s %s %s relative error %.3g, mfma %.3g" % (ic.case_id(case), label, name, e, e_exact))
            assert e <= factor * e_exact + 1e-7, (label, name, e, e_exact)
    for name in ("out", "z", "linear.bias"):
        assert torch.equal(pair[name], one_wave[name]), "pair against one wave: " + name
    _close(pair["linear.weight"], one_wave["linear.weight"], 0.0, 1e-5 * one_wave["linear.weight"].abs().max().item())


# ------------------------------------------------------------------------------------------------ two and three layers
MLP_CASES = [c for family in ("mlp2", "mlp3", "mlp2w", "mlp2h", "mlp2b") for c in ic.cases(family)]


@pytest.mark.parametrize("case", MLP_CASES, ids=ic.case_id)
def test_layered_fields(native, case):
    """The forward kernel under no_grad and the training call (forward + continuous-adjoint sweep) against the oracle's
    adjoint=True run; the softplus field on the two-layer tiles with adjoint=False as well, against autograd through the
    oracle's steps."""
    ref = ic.reference(case)
    plain = _solve(native, case, ref, grad=False)
    _check(case, ref, plain, "forward")
    trained = _solve(native, case, ref)
    _check(case, ref, trained, "adjoint")
    if case.family == "mlp2":
        through = ic.reference(case, adjoint=False)
        got = _solve(native, case, through, adjoint=False, expect=("mlp_rk4_backprop", "", "_FusedMlpRK4BackpropBackward"))
        _check(case, through, got, "adjoint=False")


# ------------------------------------------------------------------------------------------------ reversible Heun
@pytest.mark.parametrize("case", ic.cases("revheun"), ids=ic.case_id)
def test_reversible_heun(native, case):
    """RHf / RHa against the float64 restatement and autograd through it; adjoint=False takes the same sweep; under no_grad the
    forward kernel alone gives the training call's solution."""
    ref = ic.reference(case)
    got = _solve(native, case, ref)
    _check(case, ref, got, "adjoint")
    err, floor = _gap(got["out"], ref["f64"]["out"]), ic.cpu32_error(ref, "out")
    print("IRR revheun %s kernel error %.3g, CPU float32 restatement %.3g" % (ic.case_id(case), err, floor))
    assert err <= 4 * floor, (err, floor)
    _same(_solve(native, case, ref, adjoint=False), got, "adjoint=False")
    _same(_solve(native, case, ref, grad=False), dict(out=got["out"]), "no_grad")


# ------------------------------------------------------------------------------------------------ riders, one case per family
def _calls(native, case):
    """the family's kinds of call: keywords of _solve"""
    if case.family == "affine" and not case.shape[2]:
        return [dict(grad=False, variant="bf16x3", expect=("rk4", "bf16x3", None)),
                dict(variant="bf16x3", expect=("rk4", "bf16x3", NODE["affine"]))]
    if case.family == "affine":
        return [dict(grad=False, variant="mfma", expect=("rk4", "exact", None)),
                dict(variant="mfma", expect=("rk4", "exact", NODE["affine"]))]
    return [dict(grad=False), dict()]


RIDERS = [ic.Case("affine", (32, 8, False), 1, 0.75), ic.Case("affine", (19, 5, True), 3, 0.5),
          ic.Case("mlp2", (16, 14, 64, "softplus", False), 1, 0.75), ic.Case("mlp3", (5, 3, 20, 33, "softplus", False), 1, 0.5),
          ic.Case("mlp2w", (16, 21, 100, "relu", False), 1, 2.0), ic.Case("mlp2h", (40, 5, 64, "relu", False), 1, None),
          ic.Case("mlp2b", (5, 3, 129, "softplus", False), 1, 0.75), ic.Case("revheun", (6, 3, True), 1, 0.75)]


@pytest.mark.parametrize("case", RIDERS, ids=ic.case_id)
def test_repeat_leading_batch_shape_and_views_keep_the_bits(native, case):
    """The flat call on fresh tensors, then: once more (fixed-order reductions, no float atomics); with the series as a
    (5, 7) / (3, 11) batch; with z0, the coefficients and the knots as views of larger buffers -- the entry points take raw
    pointers, so a plan that forgot to pack a view would read its neighbours.  Outputs and all gradients bitwise equal."""
    assert case in ic.ALL_CASES
    ref = ic.reference(case)
    batch = (3, 11) if ic.FAMILIES[case.family][0] == 33 else (5, 7)
    for call in _calls(native, case):
        flat = _solve(native, case, ref, **call)
        _check(case, ref, flat, "flat")
        _same(_solve(native, case, ref, **call), flat, "second call")
        _same(_solve(native, case, ref, batch=batch, **call), flat, "leading batch shape")
        _same(_solve(native, case, ref, views=True, **call), flat, "views")

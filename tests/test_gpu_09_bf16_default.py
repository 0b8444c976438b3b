"""The headline field's default path on the bf16 matrix pipe (K2b forward, K3p's bf16 form backward): exact piece products
with float32 accumulation.  Bars: agreement with the exact-f32 kernels (variant="mfma") at benchmark size, error against the
float64 oracle within 2x of the exact path's on the same series, run-to-run bit-identical results."""
import sys

import pytest
import torch

from gpu_common import oracle_cde, oracle_interp, LinearField, make_series, DEV, _close

pytestmark = pytest.mark.gpu


def _solve(native, X, z0, H, C, t, variant, weights=None, form=None):
    f = LinearField(H, C, scale=0.25, seed=0).to(DEV)
    z = z0.clone().requires_grad_(True)
    kw = {} if variant is None else dict(variant=variant)
    out = native.cdeint(X, f, z, t, method="rk4", options=dict(step_size=1.0), **kw)
    if form is not None:                                 # the dispatch record names the arithmetic that ran
        choice = sys.modules["torchcde_amd.cdeint"].last_dispatch()[0]
        assert choice.path == "rk4" and choice.form == form, choice
    (out[:, -1].sum() if weights is None else (out * weights).sum()).backward()
    torch.cuda.synchronize()
    return out.detach(), z.grad, f.linear.weight.grad, f.linear.bias.grad


def test_default_path_at_benchmark_size_agrees_with_the_exact_kernels(native):
    B, L, C, H = 32768, 128, 8, 32
    x = make_series(B, L, C, seed=0).to(DEV)
    X = native.CubicSpline(native.hermite_cubic_coefficients_with_backward_differences(x))
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(0)).to(DEV)
    exact = _solve(native, X, z0, H, C, X.interval, "mfma", form="exact")
    first = _solve(native, X, z0, H, C, X.interval, None, form="bf16x3")
    again = _solve(native, X, z0, H, C, X.interval, None, form="bf16x3")
    for a, b in zip(first, again):                       # deterministic: fixed-order partial reduction
        assert torch.equal(a, b)
    for a, b in zip(first, exact):
        assert torch.isfinite(a).all()
        _close(a, b, 1e-5, 1e-5 * b.abs().max().item())
    # the same numbers as the explicit variant; the one-wave form K3bj (k3_waves = 1) forms the J rows in the same order, so
    # the trajectories, dL/dz0 and dL/db are bitwise the pair's; its dL/dW stays on the f32 pipe (float32 rounding apart)
    for a, b in zip(first, _solve(native, X, z0, H, C, X.interval, "bf16x3", form="bf16x3")):
        assert torch.equal(a, b)
    native.set_option("k3_waves", 1)
    one_wave = _solve(native, X, z0, H, C, X.interval, "bf16x3", form="bf16x3")
    native.set_option("k3_waves", 0)
    for i in (0, 1, 3):
        assert torch.equal(first[i], one_wave[i]), i
    _close(first[2], one_wave[2], 1e-5, 1e-5 * one_wave[2].abs().max().item())
    # four 256-series samples of the batch against the float64 oracle: at most 2x the exact path's error
    fo = LinearField(H, C, torch.float64, scale=0.25, seed=0)
    xs = make_series(B, L, C, seed=0)
    for start in (0, 8192, 20000, B - 256):
        sl = slice(start, start + 256)
        Xo = oracle_interp.CubicPath(oracle_interp.hermite_bdiff_coeffs(xs[sl].double()))
        zo = z0[sl].double().cpu().requires_grad_(True)
        fo.zero_grad()
        ref = oracle_cde.cdeint(Xo, fo, zo, Xo.interval, adjoint=True, method="rk4", options=dict(step_size=1.0))
        ref[:, -1].sum().backward()
        e_new = float((first[0][sl].double().cpu() - ref.detach()).abs().max())
        e_f32 = float((exact[0][sl].double().cpu() - ref.detach()).abs().max())
        assert e_new <= 2 * e_f32 + 1e-7, (start, e_new, e_f32)
        g_new = float((first[1][sl].double().cpu() - zo.grad).abs().max())
        g_f32 = float((exact[1][sl].double().cpu() - zo.grad).abs().max())
        assert g_new <= 2 * g_f32 + 1e-7, (start, g_new, g_f32)


@pytest.mark.parametrize("B,L,C,H,degree", [(16500, 12, 8, 32, 3), (16400, 9, 5, 20, 1), (16391, 7, 3, 9, 3)])
def test_default_path_meets_the_float32_parity_bars_with_two_x_the_exact_error(native, B, L, C, H, degree):
    """Ragged, padded and linear-control shapes above the split kernels' batch limit (where the default takes the bf16
    form); three output times.  Errors against the float64 oracle on a 300-series sample: within 2x of the exact path's."""
    x = make_series(B, L, C, seed=5 + B)
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(5))
    t_out = torch.tensor([0., 2.5, float(L - 1)])
    lw = torch.rand(B, 3, H, generator=torch.Generator().manual_seed(6)) + 0.5
    n = 300
    f64 = LinearField(H, C, torch.float64, scale=0.25, seed=0)
    Xo = (oracle_interp.CubicPath(oracle_interp.hermite_bdiff_coeffs(x[:n].double())) if degree == 3
          else oracle_interp.LinearPath(x[:n].double()))
    zo = z0[:n].double().requires_grad_(True)
    ref = oracle_cde.cdeint(Xo, f64, zo, t_out.double(), adjoint=True, method="rk4", options=dict(step_size=1.0))
    (ref * lw[:n].double()).sum().backward()
    X = (native.CubicSpline(native.hermite_cubic_coefficients_with_backward_differences(x.to(DEV))) if degree == 3
         else native.LinearInterpolation(native.linear_interpolation_coeffs(x.to(DEV))))
    errs = {}
    for variant in ("mfma", None):
        out, gz, _, _ = _solve(native, X, z0.to(DEV), H, C, t_out.to(DEV), variant, lw.to(DEV),
                               form="exact" if variant else "bf16x3")
        _close(out[:n], ref.detach(), 1e-4, 1e-6)
        _close(gz[:n], zo.grad, 1e-3, 1e-4 * zo.grad.abs().max().item())
        errs[variant] = [float((out[:n].double().cpu() - ref.detach()).abs().max()),
                         float((gz[:n].double().cpu() - zo.grad).abs().max())]
    for e_new, e_f32 in zip(errs[None], errs["mfma"]):
        assert e_new <= 2 * e_f32 + 1e-7, (errs[None], errs["mfma"])

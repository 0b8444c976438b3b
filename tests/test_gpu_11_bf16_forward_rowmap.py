"""The row <-> (unit, channel) map of the bf16 field tiles (csrc/cde_bf16x3.h: D register r = unit 4 t + 2 (r & 1) + half,
channel r >> 1) at the smallest shapes that reach every branch of it and of its padding: 33 series (one full tile, one
tile with a single live series), full, odd, narrow and one-wide H and C, cubic and linear control, an output time between
two grid points.  K2b forward under no_grad and with the adjoint through K3b (tuning option k3_form = product, the other
user of the field evaluation) and through the one-wave Jacobian form (k3_waves = 1).

Bars are those of test_bf16x3_variant_meets_the_float32_parity_bars: trajectories against the float64 oracle at rtol 1e-4 /
atol 1e-6, gradients at rtol 1e-3 (atol 1e-4 of the largest entry), relative error at most 4x that of variant="mfma" on the
same inputs + 1e-7; and two runs of the same case agree bit for bit."""
import pytest
import torch

from gpu_common import oracle_cde, oracle_interp, LinearField, make_series, DEV, _close

pytestmark = pytest.mark.gpu

B, L = 33, 5
T_OUT = [0., 1.5, 4.]


def _native_run(native, x, z0, lw, H, C, degree, variant, grad=True):
    f = LinearField(H, C, scale=0.3, seed=3).to(DEV)
    X = (native.CubicSpline(native.hermite_cubic_coefficients_with_backward_differences(x.to(DEV))) if degree == 3
         else native.LinearInterpolation(native.linear_interpolation_coeffs(x.to(DEV))))
    t_out = torch.tensor(T_OUT, device=DEV)
    kw = dict(method="rk4", options=dict(step_size=1.0), variant=variant)
    if not grad:
        with torch.no_grad():
            return (native.cdeint(X, f, z0.to(DEV), t_out, **kw),)
    z = z0.to(DEV).requires_grad_(True)
    out = native.cdeint(X, f, z, t_out, **kw)
    (out * lw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), z.grad, f.linear.weight.grad, f.linear.bias.grad


def _rel_errors(got, wants):
    return [float((g.double().cpu() - w).abs().max() / w.abs().max()) for g, w in zip(got, wants)]


def _meets_the_bars(got, wants):
    _close(got[0], wants[0], 1e-4, 1e-6)
    for g, w in zip(got[1:], wants[1:]):
        _close(g, w, 1e-3, 1e-4 * w.abs().max().item())


@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("H,C", [(32, 8), (31, 7), (17, 2), (2, 1), (1, 8)])
def test_bf16_forward_row_map_on_full_and_padded_tiles(native, H, C, degree):
    x = make_series(B, L, C, seed=40 + H)
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(7))
    lw = torch.rand(B, len(T_OUT), H, generator=torch.Generator().manual_seed(8)) + 0.5
    f64 = LinearField(H, C, torch.float64, scale=0.3, seed=3)
    Xo = (oracle_interp.CubicPath(oracle_interp.hermite_bdiff_coeffs(x.double())) if degree == 3
          else oracle_interp.LinearPath(x.double()))
    zo = z0.double().requires_grad_(True)
    ref = oracle_cde.cdeint(Xo, f64, zo, torch.tensor(T_OUT, dtype=torch.float64), adjoint=True, method="rk4",
                            options=dict(step_size=1.0))
    (ref * lw.double()).sum().backward()
    wants = (ref.detach(), zo.grad, f64.linear.weight.grad, f64.linear.bias.grad)

    exact = _native_run(native, x, z0, lw, H, C, degree, "mfma")
    _meets_the_bars(exact, wants)
    e_f32 = _rel_errors(exact, wants)

    # K2b alone
    fwd = _native_run(native, x, z0, lw, H, C, degree, "bf16x3", grad=False)
    again = _native_run(native, x, z0, lw, H, C, degree, "bf16x3", grad=False)
    assert torch.equal(fwd[0], again[0])
    _close(fwd[0], wants[0], 1e-4, 1e-6)
    # K2b + K3b (the field evaluation again, beside the vjp), K2b + K3bj
    for options in (dict(k3_form="product"), dict(k3_waves=1)):
        with native.tuning(**options):
            got = _native_run(native, x, z0, lw, H, C, degree, "bf16x3")
            twice = _native_run(native, x, z0, lw, H, C, degree, "bf16x3")
        for a, b in zip(got, twice):
            assert torch.equal(a, b), options
        assert torch.equal(got[0], fwd[0]), options
        e_new = _rel_errors(got, wants)
        print(H, C, degree, options, "bf16x3", e_new, "mfma", e_f32)
        _meets_the_bars(got, wants)
        for new, f32 in zip(e_new, e_f32):
            assert new <= 4 * f32 + 1e-7, (options, e_new, e_f32)

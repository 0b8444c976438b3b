"""K2b with its weight pieces resident in accumulator registers (csrc/cde_bf16x3.h: bx_load_resident, bx_field_resident):
every wave reads its lane's 48 entries of the staged image once, before the time loop, and keeps them for the whole solve.

(a) the shapes of test_gpu_11_bf16_forward_rowmap.py that reach the padding of the image (full, odd and one-wide H and C),
    33 series, cubic and linear control, an output time between two grid points, float32 and float64 time grids.
(b) 161 series = the same 32 series five times plus one more, 39 steps: two workgroups, every wave slot of the first, and a
    last workgroup whose one live wave has a single live series.  The five copies must agree bit for bit: a wave that did not
    load its own copy of the image, or lost a register of it over 156 stages, shows here.

Bars are those of test_gpu_11: trajectories against the float64 oracle at rtol 1e-4 / atol 1e-6, two runs bit-identical,
relative error at most 4x that of variant="mfma" on the same inputs + 1e-7.

The initial states of (b) are 0.1 x those of (a).  atol 1e-6 is a bar for five steps: over 156 stages float32 round-off
alone passes it on states of size 4 -- the float64 oracle's own arithmetic in float32 on the CPU lands at 4.6e-6 from it,
1.3 x the tolerance, on the inputs of (a) at L = 40, and the exact-f32 kernels likewise.  The error follows the size of
the state (the field is affine); at 0.1 x the same CPU float32 solve lies at 9.4e-7, 0.21 x the tolerance, which leaves
the bar a factor of five above what float32 itself can reach."""
import functools

import pytest
import torch

from gpu_common import oracle_cde, oracle_interp, LinearField, make_series, DEV, _close

pytestmark = pytest.mark.gpu


def _path(module, x, degree, native_side):
    if native_side:
        return (module.CubicSpline(module.hermite_cubic_coefficients_with_backward_differences(x.to(DEV))) if degree == 3
                else module.LinearInterpolation(module.linear_interpolation_coeffs(x.to(DEV))))
    return (oracle_interp.CubicPath(oracle_interp.hermite_bdiff_coeffs(x.double())) if degree == 3
            else oracle_interp.LinearPath(x.double()))


def _solve(native, x, z0, H, C, degree, t_out, variant):
    f = LinearField(H, C, scale=0.3, seed=3).to(DEV)
    with torch.no_grad():
        out = native.cdeint(_path(native, x, degree, True), f, z0.to(DEV), t_out.to(DEV), method="rk4",
                            options=dict(step_size=1.0), variant=variant)
    torch.cuda.synchronize()
    return out


def _inputs(B, L, H, C, z_scale=1.0):
    return make_series(B, L, C, seed=40 + H), z_scale * torch.randn(B, H, generator=torch.Generator().manual_seed(7))


@functools.lru_cache(maxsize=None)
def _oracle(B, L, H, C, degree, t_out, z_scale=1.0):
    """the float64 solution, once per case and shared by the time-grid types"""
    x, z0 = _inputs(B, L, H, C, z_scale)
    f64 = LinearField(H, C, torch.float64, scale=0.3, seed=3)
    with torch.no_grad():
        return oracle_cde.cdeint(_path(None, x, degree, False), f64, z0.double(), torch.tensor(t_out, dtype=torch.float64),
                                 adjoint=False, method="rk4", options=dict(step_size=1.0))


def _rel_error(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _meets_the_bars(native, x, z0, H, C, degree, t_out, want):
    exact = _solve(native, x, z0, H, C, degree, t_out, "mfma")
    got = _solve(native, x, z0, H, C, degree, t_out, "bf16x3")
    again = _solve(native, x, z0, H, C, degree, t_out, "bf16x3")
    assert torch.equal(got, again)
    e_new, e_f32 = _rel_error(got, want), _rel_error(exact, want)
    print(H, C, degree, t_out.dtype, "bf16x3", e_new, "mfma", e_f32)
    _close(got, want, 1e-4, 1e-6)
    assert e_new <= 4 * e_f32 + 1e-7, (e_new, e_f32)
    return got


@pytest.mark.parametrize("time_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("H,C", [(32, 8), (31, 7), (2, 1)])
def test_resident_weights_on_full_and_padded_tiles(native, H, C, degree, time_dtype):
    B, L, t_out = 33, 5, (0., 1.5, 4.)
    x, z0 = _inputs(B, L, H, C)
    _meets_the_bars(native, x, z0, H, C, degree, torch.tensor(t_out, dtype=time_dtype), _oracle(B, L, H, C, degree, t_out))


@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("H,C", [(32, 8), (31, 7)])
def test_every_wave_holds_its_own_copy_of_the_weights(native, H, C, degree):
    L, t_out = 40, (0., 17.5, 39.)
    x33, z33 = _inputs(33, L, H, C, 0.1)
    rows = list(range(32)) * 5 + [32]                                    # B = 161: tiles 0-3 in workgroup 0, 4 and 5 in workgroup 1
    x, z0 = x33[rows].contiguous(), z33[rows].contiguous()
    want = _oracle(33, L, H, C, degree, t_out, 0.1)[rows]
    got = _meets_the_bars(native, x, z0, H, C, degree, torch.tensor(t_out), want)
    assert got.shape[0] == 161
    for k in range(1, 5):
        assert torch.equal(got[32 * k:32 * k + 32], got[:32]), "tile %d differs from tile 0" % k

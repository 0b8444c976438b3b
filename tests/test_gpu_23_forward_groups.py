"""K2bd, the bf16 rk4 forward with the wave's 32 series as two interleaved groups of 16 (csrc/rk4_bf16x3_duo.hip,
csrc/cde_bf16x3_duo.h): the field on v_mfma_f32_16x16x32_bf16, lane (n, q) of a wave keeping units 8 q .. 8 q + 7 of series
16 g + n of its tile for both groups g, the control slopes formed two channels per lane and exchanged through LDS.

(1) the row map and the padding: full, odd, narrow and one-wide H and C, cubic and linear control, an output time between two
    grid points, 17 series (group A full, group B with one live series) and 33 (a second tile whose group A has one live
    series and whose group B has none), float32 and float64 time grids at the two widest shapes.
(2) the groups are independent and every wave holds its own image: case (b) of test_gpu_14_bf16_forward_resident_weights.py
    on the same inputs (161 series = the same 32 five times plus one, 39 steps), then once more with the rows of every block
    of 32 rotated by 16, so that each series sits in the other group: the five copies agree bit for bit, and the rotated run
    equals the first series by series, bit for bit.
(3) dispatch: the default call above the split kernels' batch limit records the bf16 form and meets the second test of
    test_gpu_09_bf16_default.py on the solution and dL/dz0, under tuning(k2b_groups=1) (K2b) as well, and the two solutions
    agree at 1e-5 of the largest entry.

Bars are those of test_gpu_11 / test_gpu_14: trajectories against the float64 oracle at rtol 1e-4 / atol 1e-6, two runs
bit-identical, relative error at most 4x that of variant="mfma" on the same inputs + 1e-7.  (2) runs at 0.1 x the states of
(1), for the reason test_gpu_14 gives: atol 1e-6 is a bar for five steps, not for 156 stages on states of size 4."""
import functools
import sys

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
    """the float64 solution, once per case and shared by the batch sizes and time-grid types (a prefix of 33 series)"""
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
    print(H, C, degree, t_out.dtype, tuple(got.shape), "bf16x3", e_new, "mfma", e_f32)
    _close(got, want, 1e-4, 1e-6)
    assert e_new <= 4 * e_f32 + 1e-7, (e_new, e_f32)
    return got


_SHAPES = [(32, 8), (31, 7), (17, 2), (2, 1), (1, 8)]
_CASES = [(H, C, torch.float32) for H, C in _SHAPES] + [(32, 8, torch.float64), (31, 7, torch.float64)]


@pytest.mark.parametrize("B", [17, 33])
@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("H,C,time_dtype", _CASES)
def test_row_map_and_padding(native, H, C, time_dtype, degree, B):
    L, t_out = 5, (0., 1.5, 4.)
    x, z0 = _inputs(33, L, H, C)                          # B = 17: the first 17 of the 33 series the oracle solved
    want = _oracle(33, L, H, C, degree, t_out)[:B]
    _meets_the_bars(native, x[:B].contiguous(), z0[:B].contiguous(), H, C, degree, torch.tensor(t_out, dtype=time_dtype), want)


@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("H,C", [(32, 8), (31, 7)])
def test_groups_are_independent_and_every_wave_holds_its_own_image(native, H, C, degree):
    L, t_out = 40, (0., 17.5, 39.)
    x33, z33 = _inputs(33, L, H, C, 0.1)
    rows = list(range(32)) * 5 + [32]                     # B = 161: tiles 0-3 in workgroup 0, 4 and 5 in workgroup 1
    x, z0 = x33[rows].contiguous(), z33[rows].contiguous()
    want = _oracle(33, L, H, C, degree, t_out, 0.1)[rows]
    got = _meets_the_bars(native, x, z0, H, C, degree, torch.tensor(t_out), want)
    assert got.shape[0] == 161
    for k in range(1, 5):
        assert torch.equal(got[32 * k:32 * k + 32], got[:32]), "tile %d differs from tile 0" % k
    # every series in the other group: position p of a block of 32 takes the series that sat at (p + 16) % 32
    perm = [32 * (p // 32) + (p % 32 + 16) % 32 for p in range(160)] + [160]
    rotated = _solve(native, x[perm].contiguous(), z0[perm].contiguous(), H, C, degree, torch.tensor(t_out), "bf16x3")
    assert torch.equal(rotated, got[perm]), "a series' result depends on the group it sits in"


def _solve_with_grad(native, X, z0, H, C, t, variant, weights):
    f = LinearField(H, C, scale=0.25, seed=0).to(DEV)
    z = z0.clone().requires_grad_(True)
    kw = {} if variant is None else dict(variant=variant)
    out = native.cdeint(X, f, z, t, method="rk4", options=dict(step_size=1.0), **kw)
    choice = sys.modules["torchcde_amd.cdeint"].last_dispatch()[0]
    assert choice.path == "rk4" and choice.form == ("exact" if variant else "bf16x3"), choice
    (out * weights).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), z.grad


def test_default_dispatch_and_the_adjoint_from_the_new_forward(native):
    B, L, C, H = 16400, 9, 5, 20
    x = make_series(B, L, C, seed=5 + B)
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(5))
    t_out = torch.tensor([0., 2.5, float(L - 1)])
    lw = torch.rand(B, 3, H, generator=torch.Generator().manual_seed(6)) + 0.5
    n = 300
    f64 = LinearField(H, C, torch.float64, scale=0.25, seed=0)
    Xo = oracle_interp.LinearPath(x[:n].double())
    zo = z0[:n].double().requires_grad_(True)
    ref = oracle_cde.cdeint(Xo, f64, zo, t_out.double(), adjoint=True, method="rk4", options=dict(step_size=1.0))
    (ref * lw[:n].double()).sum().backward()
    X = native.LinearInterpolation(native.linear_interpolation_coeffs(x.to(DEV)))

    def errors(variant):
        out, gz = _solve_with_grad(native, X, z0.to(DEV), H, C, t_out.to(DEV), variant, lw.to(DEV))
        _close(out[:n], ref.detach(), 1e-4, 1e-6)
        _close(gz[:n], zo.grad, 1e-3, 1e-4 * zo.grad.abs().max().item())
        return out, [float((out[:n].double().cpu() - ref.detach()).abs().max()),
                     float((gz[:n].double().cpu() - zo.grad).abs().max())]

    _, e_f32 = errors("mfma")
    new, e_new = errors(None)
    with native.tuning(k2b_groups=1):
        old, e_old = errors(None)
    print("errors (solution, dL/dz0): exact", e_f32, "two groups", e_new, "K2b", e_old)
    for e in (e_new, e_old):
        for e_bf, e_ex in zip(e, e_f32):
            assert e_bf <= 2 * e_ex + 1e-7, (e, e_f32)
    _close(new, old, 1e-5, 1e-5 * old.abs().max().item())

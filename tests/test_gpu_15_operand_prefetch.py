"""Round 11 moved LDS requests ahead of the instructions that wait for them in K2b and K3p.  Nothing about the values may
change: the same reads of the same addresses reach the same consumers.  What was kept is the helper wave of K3p's bf16 form
(csrc/rk4_adjoint_pair.hip: the weighted control derivative of block (g, c + 1), and the next K block's z / a rows, requested
before the MFMAs of block (g, c); the stage's first block before the wave forms a later stage's derivative).  K2b's bias
tiles a pair ahead and the chain wave's first row images ahead of the stage barrier were built and not kept; their cases
stay, because they pin behaviour that must not change, and pass on the build before this round too.

(a) K2b: one RK step (L = 2) and two (L = 3), full and padded tiles, cubic and linear control, with and without an output
    time between two grid points.
(b) K2b with a field that is its bias alone: zero weight, bias entry h C + c = 1 + (h C + c) / (H C), z0 = 0.  The solution
    is then sum_c b[h, c] (X_c(t) - X_c(0)); a tile, half or register of the bias table taken from a neighbouring slot
    moves it by about 1 / (H C) of its size.  The test first checks on the CPU that exchanging two rows of the bias moves
    the oracle's output by more than ten times the tolerance.
(c) K3p: the pair run against the one-wave run (k3_waves = 1) and the float64 oracle, on 33 series and on 161 (the same 32
    five times plus one: the last workgroup has one live tile with one live series and two dead tiles that keep pace with
    the barriers), one and four RK steps, one and two segments (two: the helper's requests cross a segment boundary and the
    chain wave's re-seed from z_saved), full and padded tiles.  The one-wave kernel forms dL/db in the same order, so a
    helper that took an operand of another block shows as a differing bit there, and beyond rounding in dL/dW.

Bars of (a), (b): test_gpu_14's -- the float64 oracle at rtol 1e-4 / atol 1e-6, two runs bit-identical, relative error at
most 4x that of variant="mfma" + 1e-7.  Bars of (c): test_gpu_09's -- the pair equals the one-wave run bit for bit on the
solution, dL/dz0 and dL/db and within 1e-5 of its scale on dL/dW; oracle at 1e-4 / 1e-6 on the solution, 1e-3 / 1e-4 max
on dL/dz0."""
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


def _field(H, C, dtype=torch.float32, bias_only=False, swap_rows=None):
    f = LinearField(H, C, dtype, scale=0.3, seed=3)
    if bias_only:
        with torch.no_grad():
            f.linear.weight.zero_()
            b = 1 + torch.arange(H * C, dtype=torch.float64) / (H * C)
            if swap_rows is not None:
                b = b.view(H, C)
                b[list(swap_rows)] = b[list(reversed(swap_rows))]
                b = b.reshape(-1)
            f.linear.bias.copy_(b)
    return f


def _inputs(B, L, H, C, bias_only=False):
    x = make_series(B, L, C, seed=40 + H)
    z0 = torch.zeros(B, H) if bias_only else torch.randn(B, H, generator=torch.Generator().manual_seed(7))
    return x, z0


@functools.lru_cache(maxsize=None)
def _oracle(B, L, H, C, degree, t_out, bias_only=False, swap_rows=None):
    """the float64 forward solution, once per case"""
    x, z0 = _inputs(B, L, H, C, bias_only)
    with torch.no_grad():
        return oracle_cde.cdeint(_path(None, x, degree, False), _field(H, C, torch.float64, bias_only, swap_rows), z0.double(),
                                 torch.tensor(t_out, dtype=torch.float64), adjoint=False, method="rk4", options=dict(step_size=1.0))


def _forward(native, x, z0, H, C, degree, t_out, variant, bias_only):
    with torch.no_grad():
        out = native.cdeint(_path(native, x, degree, True), _field(H, C, bias_only=bias_only).to(DEV), z0.to(DEV),
                            torch.tensor(t_out).to(DEV), method="rk4", options=dict(step_size=1.0), variant=variant)
    torch.cuda.synchronize()
    return out


def _rel_error(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _forward_meets_the_bars(native, B, L, H, C, degree, t_out, bias_only=False):
    x, z0 = _inputs(B, L, H, C, bias_only)
    want = _oracle(B, L, H, C, degree, t_out, bias_only)
    exact = _forward(native, x, z0, H, C, degree, t_out, "mfma", bias_only)
    got = _forward(native, x, z0, H, C, degree, t_out, "bf16x3", bias_only)
    again = _forward(native, x, z0, H, C, degree, t_out, "bf16x3", bias_only)
    assert torch.equal(got, again)
    e_new, e_f32 = _rel_error(got, want), _rel_error(exact, want)
    print(B, L, H, C, degree, t_out, "bf16x3", e_new, "mfma", e_f32)
    _close(got, want, 1e-4, 1e-6)
    assert e_new <= 4 * e_f32 + 1e-7, (e_new, e_f32)


@pytest.mark.parametrize("three_times", [False, True])
@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("H,C", [(32, 8), (31, 7)])
@pytest.mark.parametrize("L", [2, 3])
def test_forward_over_one_and_two_steps(native, L, H, C, degree, three_times):
    t_out = (0., 0.5, L - 1.) if three_times else (0., L - 1.)
    _forward_meets_the_bars(native, 33, L, H, C, degree, t_out)


@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("H,C", [(32, 8), (31, 7)])
def test_forward_that_only_the_bias_reaches(native, H, C, degree):
    B, L, t_out = 33, 5, (0., 1.5, 4.)
    want = _oracle(B, L, H, C, degree, t_out, True)
    moved = (_oracle(B, L, H, C, degree, t_out, True, (0, 1)) - want).abs().max().item()
    bar = 1e-6 + 1e-4 * want.abs().max().item()
    print(H, C, degree, "two bias rows exchanged move the oracle by", moved, "bar", bar)
    assert moved > 10 * bar, (moved, bar)            # the inputs can tell a misplaced bias row from rounding
    _forward_meets_the_bars(native, B, L, H, C, degree, t_out, bias_only=True)


# ------------------------------------------------------------------------------------------------ (c) K3p
ROWS161 = list(range(32)) * 5 + [32]


def _adjoint_inputs(L, H, C, n_times):
    x, z0 = _inputs(33, L, H, C)
    lw = torch.rand(33, n_times, H, generator=torch.Generator().manual_seed(6)) + 0.5
    return x, z0, lw


@functools.lru_cache(maxsize=None)
def _adjoint_oracle(L, H, C, degree, t_out):
    """float64 solution and dL/dz0 of the 33 series, shared by B = 33 and B = 161 (per-series quantities)"""
    x, z0, lw = _adjoint_inputs(L, H, C, len(t_out))
    zo = z0.double().requires_grad_(True)
    ref = oracle_cde.cdeint(_path(None, x, degree, False), _field(H, C, torch.float64), zo, torch.tensor(t_out, dtype=torch.float64),
                            adjoint=True, method="rk4", options=dict(step_size=1.0))
    (ref * lw.double()).sum().backward()
    return ref.detach(), zo.grad


def _backward(native, X, z0, lw, H, C, t):
    f = _field(H, C).to(DEV)
    z = z0.clone().requires_grad_(True)
    out = native.cdeint(X, f, z, t, method="rk4", options=dict(step_size=1.0), variant="bf16x3")
    choice = sys.modules["torchcde_amd.cdeint"].last_dispatch()[0]
    assert choice.form == "bf16x3", choice
    (out * lw).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), z.grad, f.linear.weight.grad, f.linear.bias.grad


@pytest.mark.parametrize("three_times", [False, True])
@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("H,C", [(32, 8), (20, 5)])
@pytest.mark.parametrize("L", [2, 5])
@pytest.mark.parametrize("B", [33, 161])
def test_adjoint_pair_against_one_wave_and_oracle(native, B, L, H, C, degree, three_times):
    t_out = (0., 0.5, L - 1.) if three_times else (0., L - 1.)
    x, z0, lw = _adjoint_inputs(L, H, C, len(t_out))
    want, want_gz = _adjoint_oracle(L, H, C, degree, t_out)
    if B == 161:
        x, z0, lw, want, want_gz = (v[ROWS161].contiguous() for v in (x, z0, lw, want, want_gz))
    X, t = _path(native, x, degree, True), torch.tensor(t_out).to(DEV)
    pair = _backward(native, X, z0.to(DEV), lw.to(DEV), H, C, t)
    native.set_option("k3_waves", 1)
    try:
        one_wave = _backward(native, X, z0.to(DEV), lw.to(DEV), H, C, t)
    finally:
        native.set_option("k3_waves", 0)
    for i in (0, 1, 3):
        assert torch.equal(pair[i], one_wave[i]), i
    _close(pair[2], one_wave[2], 1e-5, 1e-5 * one_wave[2].abs().max().item())
    _close(pair[0], want, 1e-4, 1e-6)
    _close(pair[1], want_gz, 1e-3, 1e-4 * want_gz.abs().max().item())
    if B == 161:
        for k in range(1, 5):
            assert torch.equal(pair[0][32 * k:32 * k + 32], pair[0][:32]), "solution: tile %d differs from tile 0" % k
            assert torch.equal(pair[1][32 * k:32 * k + 32], pair[1][:32]), "dL/dz0: tile %d differs from tile 0" % k

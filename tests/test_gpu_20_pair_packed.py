"""K3p's bf16 form (csrc/rk4_adjoint_pair.hip, `rk4_adjoint_jacobian_pair<..., BX = true>`) takes its chain wave's f32 vector
work -- the J-row consume `f_h += J[h][.] . z`, `vs += a_h J[h][.]` -- as v_pk_fma_f32 on adjacent register pairs.  A packed
instruction rounds each element as the scalar instruction does, and the scalar code already summed in the packed order
(four partial sums, `(p0 + q0) + (p1 + q1)`), so nothing about the values may change.  This file pins that: it passes on the
build before the change too.

Cases: variant="bf16x3", rk4, step_size = 1; 33 series (a ragged last tile) and 129 (the 32 first series four times plus
one: a second workgroup with one live tile of one live series and three dead tiles that keep pace with the barriers); one
and three RK steps (L = 2, 4); full tiles (32 hidden units x 8 channels) and padded ones (19 x 5); cubic and linear control;
and, once per control, three output times (two segments: the chain wave's re-seed from z_saved, the helper's cursor across a
segment boundary).

Bars (test_gpu_15's for this kernel): dL/dz0, dL/db and the solution bitwise equal to the one-wave run (k3_waves = 1, K3bj:
the same row sums, the same dL/db fma order), dL/dW within 1e-5 of its scale of that run; the float64 oracle at rtol 1e-4 /
atol 1e-6 on the solution, 1e-3 / 1e-4 max on dL/dz0 and, as smoke() asks of dL/dW, 1e-3 / 1e-3 max on dL/dW and dL/db; a
repeated run bit-identical on all four."""
import functools
import sys

import pytest
import torch

from gpu_common import oracle_cde, oracle_interp, LinearField, make_series, DEV, _close

pytestmark = pytest.mark.gpu

ROWS = {33: list(range(33)), 129: list(range(32)) * 4 + [32]}
CASES = [(B, L, H, C, degree, False) for B in (33, 129) for L in (2, 4) for H, C in ((32, 8), (19, 5)) for degree in (3, 1)]
CASES += [(129, 4, 19, 5, 3, True), (33, 4, 32, 8, 1, True)]


def _path(module, x, degree, native_side):
    if native_side:
        return (module.CubicSpline(module.hermite_cubic_coefficients_with_backward_differences(x.to(DEV))) if degree == 3
                else module.LinearInterpolation(module.linear_interpolation_coeffs(x.to(DEV))))
    return (oracle_interp.CubicPath(oracle_interp.hermite_bdiff_coeffs(x.double())) if degree == 3
            else oracle_interp.LinearPath(x.double()))


def _field(H, C, dtype=torch.float32):
    return LinearField(H, C, dtype, scale=0.3, seed=3)


@functools.lru_cache(maxsize=None)
def _inputs(B, L, H, C, n_times):
    x = make_series(33, L, C, seed=60 + H)
    z0 = torch.randn(33, H, generator=torch.Generator().manual_seed(9))
    lw = torch.rand(33, n_times, H, generator=torch.Generator().manual_seed(8)) + 0.5
    return tuple(v[ROWS[B]].contiguous() for v in (x, z0, lw))


@functools.lru_cache(maxsize=None)
def _oracle(B, L, H, C, degree, t_out):
    """float64 solution, dL/dz0, dL/dW and dL/db, once per case"""
    x, z0, lw = _inputs(B, L, H, C, len(t_out))
    f = _field(H, C, torch.float64)
    zo = z0.double().requires_grad_(True)
    ref = oracle_cde.cdeint(_path(None, x, degree, False), f, zo, torch.tensor(t_out, dtype=torch.float64), adjoint=True,
                            method="rk4", options=dict(step_size=1.0))
    (ref * lw.double()).sum().backward()
    return ref.detach(), zo.grad, f.linear.weight.grad, f.linear.bias.grad


def _backward(native, X, z0, lw, H, C, t):
    f = _field(H, C).to(DEV)
    z = z0.clone().requires_grad_(True)
    out = native.cdeint(X, f, z, t, method="rk4", options=dict(step_size=1.0), variant="bf16x3")
    choice = sys.modules["torchcde_amd.cdeint"].last_dispatch()[0]
    assert choice.form == "bf16x3", choice
    (out * lw).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), z.grad, f.linear.weight.grad, f.linear.bias.grad


@pytest.mark.parametrize("B,L,H,C,degree,three_times", CASES)
def test_pair_keeps_its_bits(native, B, L, H, C, degree, three_times):
    t_out = (0., 0.5, L - 1.) if three_times else (0., L - 1.)
    x, z0, lw = _inputs(B, L, H, C, len(t_out))
    want = _oracle(B, L, H, C, degree, t_out)
    X, t = _path(native, x, degree, True), torch.tensor(t_out).to(DEV)
    pair = _backward(native, X, z0.to(DEV), lw.to(DEV), H, C, t)
    again = _backward(native, X, z0.to(DEV), lw.to(DEV), H, C, t)
    native.set_option("k3_waves", 1)
    try:
        one_wave = _backward(native, X, z0.to(DEV), lw.to(DEV), H, C, t)
    finally:
        native.set_option("k3_waves", 0)
    for i in range(4):
        assert torch.equal(pair[i], again[i]), "run to run, output %d" % i
    for i in (0, 1, 3):
        assert torch.equal(pair[i], one_wave[i]), "pair against one wave, output %d" % i
    _close(pair[2], one_wave[2], 1e-5, 1e-5 * one_wave[2].abs().max().item())
    _close(pair[0], want[0], 1e-4, 1e-6)
    _close(pair[1], want[1], 1e-3, 1e-4 * want[1].abs().max().item())
    _close(pair[2].view_as(want[2]), want[2], 1e-3, 1e-3 * want[2].abs().max().item())
    _close(pair[3].view_as(want[3]), want[3], 1e-3, 1e-3 * want[3].abs().max().item())
    if B == 129:
        for k in range(1, 4):
            assert torch.equal(pair[0][32 * k:32 * k + 32], pair[0][:32]), "solution: tile %d differs from tile 0" % k
            assert torch.equal(pair[1][32 * k:32 * k + 32], pair[1][:32]), "dL/dz0: tile %d differs from tile 0" % k

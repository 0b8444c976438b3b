"""GPU tests of the launch branches of the interpolation host layer (csrc/interp_kernels.hip) that tests/test_gpu_07_interp.py
does not reach: K1's one-value-per-lane kernel chosen for alignment alone, the checked fit's own entry point, and the
float64 kernels of cde_path_eval_backward.  Smallest shapes that take each branch.
"""
import pytest
import torch

from gpu_common import oracle_interp, make_series, DEV, _close

pytestmark = pytest.mark.gpu


def test_hermite_fit_of_an_input_off_the_16_byte_grid_takes_the_scalar_kernel(native):
    """K1 fits one 16-byte vector per lane only when `x` and the coefficients start on a 16-byte boundary.  Four float32
    channels read from a storage offset of one element are a multiple of the vector width but 4 bytes past the boundary:
    the one-value-per-lane kernel runs instead.  The front end hands such a view through without a copy.  Same floats as
    the fit of an aligned clone: through the fit without a NaN scan (x requires a gradient), through the scanning fit,
    and through the gated fill + refit (data with a gap)."""
    fit = native.hermite_cubic_coefficients_with_backward_differences
    flat = make_series(1, 1, 2 * 5 * 4 + 1, seed=17).reshape(-1).to(DEV)
    for gap in (False, True):
        if gap:
            flat[1 + (1 * 5 + 2) * 4 + 3] = float("nan")              # series 1, knot 2, channel 3
        view = flat[1:].view(2, 5, 4)
        aligned = view.clone()
        assert view.is_contiguous() and view.contiguous().data_ptr() == view.data_ptr()
        assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
        want = fit(aligned)
        assert torch.equal(want.cpu(), oracle_interp.hermite_bdiff_coeffs(aligned.cpu()))
        assert torch.equal(fit(view), want)
        if not gap:
            assert torch.equal(fit(view.detach().requires_grad_(True)).detach(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_checked_hermite_entry_point_fits_and_raises_its_flag(native, dtype):
    """cde_hermite_bdiff_coeffs_checked (the fit with the NaN scan, no repair; nothing in the front end calls it): the
    floats of the plain fit, the flag left alone on clean data and raised to 1 by a NaN -- vectorised (4 channels) and
    one value per lane (3 channels)."""
    from torchcde_amd import _lib
    lib = _lib.load()
    for C in (4, 3):
        x = make_series(2, 5, C, dtype=dtype, seed=C).to(DEV)
        knots = torch.linspace(0, 4, 5, dtype=dtype, device=DEV)
        want = native.hermite_cubic_coefficients_with_backward_differences(x)
        for expect in (0, 1):
            out = torch.empty_like(want)
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            _lib.check(lib.cde_hermite_bdiff_coeffs_checked(_lib.ptr(x), _lib.ptr(knots), _lib.ptr(out), 2, 5, C,
                                                            _lib.dtype_enum(dtype), _lib.ptr(flag), _lib.stream_ptr(x.device)),
                       "cde_hermite_bdiff_coeffs_checked")
            assert flag.item() == expect
            if expect == 0:
                assert torch.equal(out, want)
                x[1, 2, C - 1] = float("nan")


@pytest.mark.parametrize("degree", [3, 1])
def test_float64_path_evaluation_gradient_wrt_the_coefficients(native, degree):
    """cde_path_eval_backward in float64, value and derivative of both controls (the golden gradients are float32):
    against autograd through the oracle's paths, which evaluate the same expressions."""
    gen = torch.Generator().manual_seed(61 + degree)
    B, L, C = 2, 5, 3
    x = torch.randn(B, L, C, generator=gen, dtype=torch.float64)
    t = (torch.rand(L, generator=gen, dtype=torch.float64) + 0.3).cumsum(0)
    tq = t[0] + torch.rand(7, generator=gen, dtype=torch.float64) * (t[-1] - t[0])
    w = torch.randn(B, 7, C, generator=gen, dtype=torch.float64)
    coeffs = oracle_interp.hermite_bdiff_coeffs(x, t) if degree == 3 else x
    for what in ("evaluate", "derivative"):
        co = coeffs.clone().requires_grad_(True)
        Xo = oracle_interp.CubicPath(co, t) if degree == 3 else oracle_interp.LinearPath(co, t)
        (getattr(Xo, what)(tq) * w).sum().backward()
        cd = coeffs.to(DEV).requires_grad_(True)
        Xd = native.CubicSpline(cd, t.to(DEV)) if degree == 3 else native.LinearInterpolation(cd, t.to(DEV))
        (getattr(Xd, what)(tq.to(DEV)) * w.to(DEV)).sum().backward()
        _close(cd.grad, co.grad, 1e-12, 1e-12 * max(1.0, co.grad.abs().max().item()))

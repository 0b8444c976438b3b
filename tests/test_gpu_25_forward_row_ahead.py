"""K2bd's control rows requested a phase ahead (csrc/rk4_bf16x3_duo.hip): the coefficient row of stage s + 2 is requested
at the head of the phase that forms the slopes of stage s + 1, into the registers that slope write has just read, where it used
to be requested behind the phase's vector work.  What can go wrong is the hand-over -- a row overwritten before its slopes are
formed, or paired with the wrong stage's fraction or width, the request made before the loop, the table's clamp at the last
step -- and it shows only where the interval index moves relative to the stages.  So, forward only, variant="bf16x3":

  grids (step, first time)  on unit knots 0 .. 11: (1, 0) the index moves at stage 1 of every step; (1, 0.25) at stage 3;
                            (0.5, 0) every other step; (0.3, 0.25) every third or fourth step, at any stage; (1.5, 0.25) one
                            or two intervals per step; (3, 0.25) three intervals per step, rows skipped.  On the knots of
                            tests/irregular_controls.py (2.5 .. 11.5, no width 1) the same five steps from 2.8125.
                            The stages of the 3/8 rule stand at t, t + h / 3, t + 2 h / 3 and t + h (no half step).  On the
                            two unit-knot grids that start at 0 every stage time that meets a knot is a grid point, dyadic and
                            exact in both precisions; on every other grid the stage times are first + m h / 3 and none comes
                            within 0.0125 of a knot (test_no_stage_time_near_a_knot), so the float32 and float64 grids and
                            the oracle choose the same intervals.
  short solves              one and two RK steps: the request made before the loop, the table's clamp (entries 4 n - 1 and
                            beyond)
  shapes (H, C)             (32, 8) every lane has both its channels; (31, 7) lane q = 3 has channel 6 alone; (17, 2) lanes
                            q >= 1 load nothing and hold zeros; (1, 1) one channel on one lane
  series                    33 (a second tile: group A with one live series, group B dead, clamped to series 32 -- the last
                            row of the tensor); 17 and 32 on one grid
  controls, time grids      cubic and linear; float32, and float64 on one grid per knot set
  output times              three: the first time, one strictly inside a step, the end of the last step

Bars, for every case: the relative error against the float64 oracle is at most 4 x that of variant="mfma" on the same call
+ 1e-7 (test_gpu_23_forward_groups.py), where the exact kernel itself is within 1e-4 of the oracle's largest entry (the
project's rtol: the comparison means something); two calls bit-identical; K2b (tuning(k2b_groups=1)) agrees within 1e-5 of the
largest entry (that file's tolerance: the two sum K = 32 in a different order).  Every case prints its figures (RA ...)
before it judges them."""
import functools

import pytest
import torch

from gpu_common import oracle_cde, oracle_interp, LinearField, make_series, DEV, _close
import irregular_controls as ic

pytestmark = pytest.mark.gpu

UNIT_KNOTS = 12
# knot set -> (step, first time, number of steps); the last time is first + steps * step, inside the knots
GRIDS = {"unit": [(1.0, 0.0, 11), (1.0, 0.25, 10), (0.5, 0.0, 22), (0.3, 0.25, 30), (1.5, 0.25, 7), (3.0, 0.25, 3)],
         "irregular": [(1.0, 2.8125, 8), (0.5, 2.8125, 17), (0.3, 2.8125, 28), (1.5, 2.8125, 5), (3.0, 2.8125, 2)]}
SHAPES = [(32, 8), (31, 7), (17, 2), (1, 1)]
SERIES = 33


def _knots(kind, dtype=torch.float32):
    return torch.arange(UNIT_KNOTS, dtype=dtype) if kind == "unit" else ic.knots(dtype)


def _times(step, first, n):
    """three output times: the first, one strictly inside a step (the middle one's 0.625), the end of step n"""
    return (first, first + (n // 2 + 0.625) * step, first + n * step)


@functools.lru_cache(maxsize=None)
def _inputs(kind, H, C):
    x = make_series(SERIES, len(_knots(kind)), C, seed=70 + H)
    z0 = torch.randn(SERIES, H, generator=torch.Generator().manual_seed(11))
    return x, z0


@functools.lru_cache(maxsize=None)
def _oracle(kind, H, C, degree, step, t_out):
    """the float64 solution of the 33 series, once per case (17 and 32 series are its leading rows)"""
    x, z0 = _inputs(kind, H, C)
    knots = _knots(kind, torch.float64)
    path = (oracle_interp.CubicPath(oracle_interp.hermite_bdiff_coeffs(x.double(), knots), knots) if degree == 3
            else oracle_interp.LinearPath(x.double(), knots))
    f64 = LinearField(H, C, torch.float64, scale=0.3, seed=3)
    with torch.no_grad():
        return oracle_cde.cdeint(path, f64, z0.double(), torch.tensor(t_out, dtype=torch.float64), adjoint=False, method="rk4",
                                 options=dict(step_size=step))


def solve(native, kind, H, C, degree, step, t_out, time_dtype, B, variant):
    """one native forward solve of the first B series of the case"""
    x, z0 = _inputs(kind, H, C)
    x, z0, knots = x[:B].contiguous().to(DEV), z0[:B].contiguous().to(DEV), _knots(kind).to(DEV)
    X = (native.CubicSpline(native.hermite_cubic_coefficients_with_backward_differences(x, knots), knots) if degree == 3
         else native.LinearInterpolation(native.linear_interpolation_coeffs(x, knots), knots))
    f = LinearField(H, C, scale=0.3, seed=3).to(DEV)
    with torch.no_grad():
        out = native.cdeint(X, f, z0, torch.tensor(t_out, dtype=time_dtype, device=DEV), method="rk4",
                            options=dict(step_size=step), variant=variant)
    torch.cuda.synchronize()
    return out


def _rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _judge(native, kind, H, C, degree, step, first, n, time_dtype=torch.float32, B=SERIES):
    t_out = _times(step, first, n)
    want = _oracle(kind, H, C, degree, step, t_out)[:B]
    args = (native, kind, H, C, degree, step, t_out, time_dtype, B)
    exact, got, again = solve(*args, "mfma"), solve(*args, "bf16x3"), solve(*args, "bf16x3")
    with native.tuning(k2b_groups=1):
        single = solve(*args, "bf16x3")
    e_new, e_old, e_f32 = _rel(got, want), _rel(single, want), _rel(exact, want)
    gap = float((got - single).abs().max() / single.abs().max())
    print("RA %s H%d C%d deg%d step %s from %s x%d %s B%d: K2bd %.3g K2b %.3g mfma %.3g, K2bd - K2b %.3g of max|z| %.3g" % (
        kind, H, C, degree, step, first, n, str(time_dtype)[6:], B, e_new, e_old, e_f32, gap, want.abs().max().item()))
    assert got.shape == (B, 3, H) and torch.isfinite(got).all()
    assert torch.equal(got, again)
    assert e_f32 <= 1e-4, e_f32
    assert e_new <= 4 * e_f32 + 1e-7, (e_new, e_f32)
    _close(got, single, 1e-5, 1e-5 * single.abs().max().item())


HAND_OVER = [(kind,) + grid for kind in GRIDS for grid in GRIDS[kind]]


def test_no_stage_time_near_a_knot():
    """what the module's docstring says of its grids: off the two dyadic ones, every stage time keeps 0.012 from every knot"""
    for kind, grids in GRIDS.items():
        knots = _knots(kind, torch.float64)
        for step, first, n in grids:
            if first == 0.0:
                assert (step * 4).is_integer() and kind == "unit"          # dyadic: grid points are exact
                continue
            times = torch.tensor([first + k * step + j * step / 3 for k in range(n) for j in range(4)], dtype=torch.float64)
            gap = (times[:, None] - knots[None, :]).abs().min().item()
            print("RA", kind, step, first, "nearest stage time to a knot:", gap)
            assert gap >= 0.012, (kind, step, first, gap)


@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("H,C", SHAPES)
@pytest.mark.parametrize("kind,step,first,n", HAND_OVER)
def test_rows_and_tables_are_handed_over_where_the_index_moves(native, kind, step, first, n, H, C, degree):
    _judge(native, kind, H, C, degree, step, first, n)


@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("H,C", SHAPES)
@pytest.mark.parametrize("kind,step,first", [("unit", 1.0, 0.0), ("irregular", 1.5, 2.8125)])
@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_steps(native, n, kind, step, first, H, C, degree):
    _judge(native, kind, H, C, degree, step, first, n)


@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("H,C", SHAPES)
@pytest.mark.parametrize("kind,step,first,n,B,time_dtype", [
    ("unit", 0.3, 0.25, 30, 17, torch.float32), ("unit", 0.3, 0.25, 30, 32, torch.float32),
    ("unit", 0.3, 0.25, 30, 17, torch.float64), ("unit", 0.3, 0.25, 30, 32, torch.float64),
    ("unit", 0.3, 0.25, 30, 33, torch.float64), ("irregular", 1.5, 2.8125, 5, 33, torch.float64)])
def test_series_counts_and_time_grids(native, kind, step, first, n, B, time_dtype, H, C, degree):
    _judge(native, kind, H, C, degree, step, first, n, time_dtype, B)
